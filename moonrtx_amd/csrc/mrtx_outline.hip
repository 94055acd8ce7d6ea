// mrtx_outline.hip -- the region outlines (mrtx_regions_outline; DESIGN.md sections 3.23, 4.29): the boundary sides of a label
// table, compacted in ascending side id, their successor map, and its cycles (the rings) found and ranked by pointer jumping:
// over every side (jump), or over the chains of sides inside a tile of nodes, walked first and handed their results after
// (contract).
// All integer work; every atomic is an integer sum, so no byte depends on a schedule.
#include "mrtx_outline.h"
#include "mrtx_lattice_dev.h"

namespace mrtx_ol {
using u64 = unsigned long long;
using namespace mrtx_lat;       // label_ok, add2, block_scan

// the label of node (i, j): -1 outside the lattice (a column past either end is the other end's with wrap) and for a bad entry.
// *v receives the node's index when it lies inside.
__device__ __forceinline__ int32_t label_at(const OutlineC& q, int32_t i, int32_t j, int32_t* v) {
    if (i < 0 || i >= q.rows) return -1;
    if (j < 0 || j >= q.cols) {
        if (!q.wrap) return -1;
        j = j < 0 ? q.cols - 1 : 0;
    }
    *v = i * q.cols + j;
    const int32_t l = q.labels[*v];
    return label_ok(q.n_regions, l) ? l : -1;
}

// travel and outward direction of side k
__device__ __forceinline__ int32_t t_y(int k) { return k == 1 ? 1 : k == 3 ? -1 : 0; }
__device__ __forceinline__ int32_t t_x(int k) { return k == 0 ? 1 : k == 2 ? -1 : 0; }
__device__ __forceinline__ int32_t d_y(int k) { return k == 0 ? -1 : k == 2 ? 1 : 0; }
__device__ __forceinline__ int32_t d_x(int k) { return k == 1 ? 1 : k == 3 ? -1 : 0; }

// the boundary bits of node n and the check of its label
__device__ __forceinline__ uint32_t node_bits(const OutlineC& q, int32_t n, uint32_t* nbad) {
    const int32_t l = q.labels[n];
    if (!label_ok(q.n_regions, l)) {
        if (l != -1) (*nbad)++;
        return 0;
    }
    const int32_t i = n / q.cols, j = n - i * q.cols;
    uint32_t bits = 0;
    for (int k = 0; k < 4; k++) {
        int32_t v;
        if (label_at(q, i + d_y(k), j + d_x(k), &v) != l) bits |= 1u << k;
    }
    return bits;
}

__global__ void __launch_bounds__(256) mark_kernel(const OutlineC q) {
    __shared__ uint2 sh[4];
    const int32_t N = q.rows * q.cols;
    const int64_t n0 = (int64_t)blockIdx.x * MRTX_OL_CHUNK + threadIdx.x * 8;
    uint32_t cnt = 0, nbad = 0;
    for (int e = 0; e < 8; e++) {
        const int64_t n = n0 + e;
        if (n >= N) break;
        const uint32_t bits = node_bits(q, (int32_t)n, &nbad);
        q.bits[n] = (uint8_t)bits;
        cnt += __popc(bits);
    }
    if (nbad) atomicAdd(q.bad, nbad);
    uint2 total;
    block_scan(make_uint2(cnt, 0), sh, &total);
    if (threadIdx.x == 0) q.node_sums[blockIdx.x] = total;
}

// One block: the chunks' sums become their exclusive prefix sums in place; totals[0], totals[1] receive the grand totals.
__global__ void __launch_bounds__(1024) scan_chunks_kernel(uint2* sums, uint32_t n, u64* totals) {
    __shared__ uint2 sh[16];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint2 carry = make_uint2(0, 0);
    for (uint32_t at = 0; at < n; at += 1024) {             // the trip count is the block's
        const uint32_t idx = at + threadIdx.x;
        const uint2 v = idx < n ? sums[idx] : make_uint2(0, 0);
        uint2 inc = v;
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t ax = __shfl_up(inc.x, d), ay = __shfl_up(inc.y, d);
            if (lane >= d) { inc.x += ax; inc.y += ay; }
        }
        __syncthreads();
        if (lane == 63) sh[w] = inc;
        __syncthreads();
        uint2 off = carry, tot = make_uint2(0, 0);
        for (int k = 0; k < 16; k++) {
            const uint2 s = sh[k];
            if (k < w) off = add2(off, s);
            tot = add2(tot, s);
        }
        if (idx < n) sums[idx] = make_uint2(off.x + inc.x - v.x, off.y + inc.y - v.y);
        carry = add2(carry, tot);
    }
    if (threadIdx.x == 0) { totals[0] = carry.x; totals[1] = carry.y; }
}

__global__ void __launch_bounds__(256) base_kernel(const OutlineC q) {
    __shared__ uint2 sh[4];
    const int32_t N = q.rows * q.cols;
    const int64_t n0 = (int64_t)blockIdx.x * MRTX_OL_CHUNK + threadIdx.x * 8;
    uint32_t cnt = 0;
    for (int e = 0; e < 8; e++)
        if (n0 + e < N) cnt += __popc((uint32_t)q.bits[n0 + e]);
    uint2 total;
    uint32_t at = q.node_sums[blockIdx.x].x + block_scan(make_uint2(cnt, 0), sh, &total).x;
    for (int e = 0; e < 8; e++)
        if (n0 + e < N) {
            q.base[n0 + e] = at;
            at += __popc((uint32_t)q.bits[n0 + e]);
        }
}

// the compact index of side k of node v, one of its boundary sides
__device__ __forceinline__ uint32_t compact(const OutlineC& q, int32_t v, int k) {
    return q.base[v] + __popc((uint32_t)q.bits[v] & ((1u << k) - 1u));
}

// One thread per node: the side ids and successors of its boundary sides, and the vertex flag of each successor (a side has
// one predecessor, so every flag has one writer).
__global__ void __launch_bounds__(256) succ_kernel(const OutlineC q) {
    const int32_t N = q.rows * q.cols;
    const int64_t n64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n64 >= N) return;
    const int32_t n = (int32_t)n64;
    const uint32_t bits = q.bits[n];
    if (!bits) return;
    const int32_t l = q.labels[n];                              // in range: the node has boundary sides
    const int32_t i = n / q.cols, j = n - i * q.cols;
    uint32_t c = q.base[n];
    for (int k = 0; k < 4; k++) {
        if (!(bits >> k & 1u)) continue;
        const int32_t ai = i + t_y(k), aj = j + t_x(k);
        int32_t av = -1, bv = -1;
        const bool la = label_at(q, ai, aj, &av) == l;
        const bool lb = label_at(q, ai + d_y(k), aj + d_x(k), &bv) == l;
        int32_t sv;
        int sk;
        if (lb && (la || q.conn8)) { sv = bv; sk = (k + 3) & 3; }   // a left turn, or through the saddle
        else if (la) { sv = av; sk = k; }                           // straight on
        else { sv = n; sk = (k + 1) & 3; }                          // a right turn
        uint32_t s = compact(q, sv, sk);
        if (!((uint32_t)q.bits[sv] >> sk & 1u) || s >= q.B) {       // never: the successor is a boundary side.  Counted, and the
            atomicAdd(q.bad + 1, 1u);                               // host fails the call; the index stays inside the tables
            if (s >= q.B) s = q.B - 1;
        }
        q.sid[c] = 4 * n + k;
        q.next[c] = (int32_t)s;
        q.flag[s] = q.all || sk != k;
        if (q.contract) {
            // bit 0: the ring enters the successor's tile here; bit 1: the successor's index is below its predecessor's
            const int32_t si = sv / q.cols, sj = sv - si * q.cols;
            const bool entry = (si >> MRTX_OL_TILE_H_SHIFT) != (i >> MRTX_OL_TILE_H_SHIFT) ||
                               (sj >> MRTX_OL_TILE_W_SHIFT) != (j >> MRTX_OL_TILE_W_SHIFT);
            q.jflag[s] = (uint8_t)((entry ? 1u : 0u) | (s < c ? 2u : 0u));
        }
        c++;
    }
}

__device__ __forceinline__ OutlineJump load_jump(const OutlineJump* p) {
    const int4 a = reinterpret_cast<const int4*>(p)[0], b = reinterpret_cast<const int4*>(p)[1];
    OutlineJump v;
    v.jump = a.x; v.mn = a.y; v.d = a.z; v.sf = a.w; v.sx = b.x; v.tf = b.y; v.tx = b.z; v.tl = b.w;
    return v;
}
__device__ __forceinline__ void store_jump(OutlineJump* p, const OutlineJump& v) {
    reinterpret_cast<int4*>(p)[0] = make_int4(v.jump, v.mn, v.d, v.sf);
    reinterpret_cast<int4*>(p)[1] = make_int4(v.sx, v.tf, v.tx, v.tl);
}

// jump: every side is an element of its own
__global__ void __launch_bounds__(256) jump_init_kernel(const OutlineC q) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= q.B) return;
    OutlineJump v;
    v.jump = q.next[c]; v.mn = (int32_t)c; v.d = 0; v.sf = 0; v.sx = 0;
    v.tf = q.flag[c]; v.tx = t_x(q.sid[c] & 3); v.tl = 1;
    store_jump(q.jump[0] + c, v);
}

// One round: a window and the one after it become one.  The earlier window keeps the least index at a tie, so that d is the
// distance to its first occurrence once a window goes round its ring more than once; its totals are used only before that, and
// are added without sign so that they may wrap afterwards.  *count: the number of elements.
__global__ void __launch_bounds__(256) jump_kernel(const OutlineJump* __restrict__ src, OutlineJump* __restrict__ dst,
                                                   const u64* __restrict__ count) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= (int64_t)*count) return;
    OutlineJump a = load_jump(src + c);
    const OutlineJump b = load_jump(src + a.jump);
    if (b.mn < a.mn) { a.mn = b.mn; a.d = a.tl + b.d; a.sf = a.tf + b.sf; a.sx = a.tx + b.sx; }
    a.tf = (int32_t)((uint32_t)a.tf + (uint32_t)b.tf);
    a.tx = (int32_t)((uint32_t)a.tx + (uint32_t)b.tx);
    a.tl = (int32_t)((uint32_t)a.tl + (uint32_t)b.tl);
    a.jump = b.jump;
    store_jump(dst + c, a);
}

// ---- contract: chains of boundary sides inside a tile of nodes become one element each.
// A side starts a chain when its ring enters its tile there, or when its index is below its predecessor's and its successor's.
// A ring's head, its least index, is such a local minimum, so every ring has a chain that starts at its head; a chain stays
// inside one tile, so it has at most MRTX_OL_CHAIN_MAX sides.
__global__ void __launch_bounds__(256) chain_sum_kernel(const OutlineC q) {
    __shared__ uint2 sh[4];
    const int64_t c0 = (int64_t)blockIdx.x * MRTX_OL_CHUNK + threadIdx.x * 8;
    uint32_t cnt = 0;
    for (int e = 0; e < 8; e++) {
        const int64_t c = c0 + e;
        if (c >= q.B) break;
        const uint32_t f = q.jflag[c];
        const bool starts = (f & 1u) || ((f & 2u) && c < (int64_t)q.next[c]);
        q.jflag[c] = starts;                                    // its own byte: nobody else reads it in this launch
        cnt += starts;
    }
    uint2 total;
    block_scan(make_uint2(cnt, 0), sh, &total);
    if (threadIdx.x == 0) q.side_sums[blockIdx.x] = total;
}

__global__ void __launch_bounds__(256) chain_index_kernel(const OutlineC q) {
    __shared__ uint2 sh[4];
    const int64_t c0 = (int64_t)blockIdx.x * MRTX_OL_CHUNK + threadIdx.x * 8;
    uint32_t cnt = 0;
    for (int e = 0; e < 8; e++)
        if (c0 + e < q.B) cnt += q.jflag[c0 + e];
    uint2 total;
    uint32_t at = q.side_sums[blockIdx.x].x + block_scan(make_uint2(cnt, 0), sh, &total).x;
    for (int e = 0; e < 8; e++)
        if (c0 + e < q.B && q.jflag[c0 + e]) q.jidx[c0 + e] = at++;
}

// what a walk along one chain sums up; end: the side after the chain, the first of the next one
struct Chain {
    int32_t tl, tf, tx, end;
};
__device__ __forceinline__ Chain walk_chain(const OutlineC& q, int32_t c) {
    Chain w;
    w.tl = 0; w.tf = 0; w.tx = 0; w.end = -1;
    int32_t t = c;
    for (int step = 0; step < MRTX_OL_CHAIN_MAX; step++) {
        w.tl++; w.tf += q.flag[t]; w.tx += t_x(q.sid[t] & 3);
        const int32_t n = q.next[t];
        if (q.jflag[n]) { w.end = n; break; }
        t = n;
    }
    return w;
}

// a thread per side: the element of the chain that starts there
__global__ void __launch_bounds__(256) chain_init_kernel(const OutlineC q) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= q.B || !q.jflag[c]) return;
    const Chain w = walk_chain(q, (int32_t)c);
    if (w.end < 0) atomicAdd(q.bad + 1, 1u);                    // never: a chain longer than a tile has sides
    OutlineJump v;
    v.jump = (int32_t)q.jidx[w.end < 0 ? c : w.end]; v.mn = (int32_t)c; v.d = 0; v.sf = 0; v.sx = 0;
    v.tf = w.tf; v.tx = w.tx; v.tl = w.tl;
    store_jump(q.jump[0] + q.jidx[c], v);
}

// A thread per side: a chain's first side hands its element's result down the chain, into the other jump buffer.  The head's
// own chain lies after the head: its sides get the ring's totals, which the element after it holds less the chain's own, less
// what lies between the head and them.
__global__ void __launch_bounds__(256) chain_down_kernel(const OutlineC q) {
    const int64_t c64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c64 >= q.B || !q.jflag[c64]) return;
    const int32_t c = (int32_t)c64;
    const OutlineJump* el = q.jump[q.rounds & 1];
    OutlineJump* out = q.jump[(q.rounds & 1) ^ 1];
    const OutlineJump e = load_jump(el + q.jidx[c]);
    const bool head = e.mn == c;
    int32_t d = e.d, sf = e.sf, sx = e.sx;
    if (head) {
        const Chain w = walk_chain(q, c);
        const OutlineJump after = load_jump(el + q.jidx[w.end < 0 ? c : w.end]);
        d = after.d + w.tl; sf = after.sf + w.tf; sx = after.sx + w.tx;     // the ring's length, vertex flags and column steps
    }
    int32_t t = c;
    OutlineJump v;
    v.jump = 0; v.tf = 0; v.tx = 0; v.tl = 0; v.mn = e.mn;
    for (int step = 0; step < MRTX_OL_CHAIN_MAX; step++) {
        const bool first = head && step == 0;
        v.d = first ? 0 : d; v.sf = first ? 0 : sf; v.sx = first ? 0 : sx;
        store_jump(out + t, v);
        d--; sf -= q.flag[t]; sx -= t_x(q.sid[t] & 3);
        const int32_t n = q.next[t];
        if (q.jflag[n]) break;
        t = n;
    }
}

// (1, its ring's vertices) at a ring's head, (0, 0) elsewhere.  The side after the head sees every other side of the ring before
// it meets the head again; a ring without a flagged side contributes its head's start corner.
__device__ __forceinline__ uint2 head_value(const OutlineC& q, const OutlineJump* fin, int64_t c) {
    if (fin[c].mn != (int32_t)c) return make_uint2(0, 0);
    const uint32_t tf = (uint32_t)q.flag[c] + (uint32_t)fin[q.next[c]].sf;
    return make_uint2(1, tf ? tf : 1);
}

__global__ void __launch_bounds__(256) heads_sum_kernel(const OutlineC q) {
    __shared__ uint2 sh[4];
    const OutlineJump* fin = q.fin;
    const int64_t c0 = (int64_t)blockIdx.x * MRTX_OL_CHUNK + threadIdx.x * 8;
    uint2 v = make_uint2(0, 0);
    for (int e = 0; e < 8; e++)
        if (c0 + e < q.B) v = add2(v, head_value(q, fin, c0 + e));
    uint2 total;
    block_scan(v, sh, &total);
    if (threadIdx.x == 0) q.side_sums[blockIdx.x] = total;
}

// the ring records, all but the two areas, and every head's ring number
__global__ void __launch_bounds__(256) heads_write_kernel(const OutlineC q) {
    __shared__ uint2 sh[4];
    const OutlineJump* fin = q.fin;
    const int64_t c0 = (int64_t)blockIdx.x * MRTX_OL_CHUNK + threadIdx.x * 8;
    uint2 v = make_uint2(0, 0);
    for (int e = 0; e < 8; e++)
        if (c0 + e < q.B) v = add2(v, head_value(q, fin, c0 + e));
    uint2 total;
    uint2 at = add2(q.side_sums[blockIdx.x], block_scan(v, sh, &total));
    for (int e = 0; e < 8; e++) {
        const int64_t c = c0 + e;
        if (c >= q.B) break;
        const uint2 h = head_value(q, fin, c);
        if (!h.x) continue;
        const int32_t s = q.sid[c];
        const OutlineJump after = fin[q.next[c]];
        RingRec r;
        r.area = 0; r.warea = 0;
        r.first = at.y;
        r.n_sides = 1u + (uint32_t)after.d;
        r.n_vertices = h.y;
        r.label = q.labels[s >> 2];
        r.head = s;
        r.wind = (t_x(s & 3) + after.sx) / q.cols;
        r.reserved = 0;
        q.rings[at.x] = r;
        q.ringno[c] = at.x;
        at = add2(at, h);
    }
}

// One thread per side: its ring's areas, summed in the wave per ring before the atomics, and its vertex.
__global__ void __launch_bounds__(256) sides_kernel(const OutlineC q) {
    const OutlineJump* fin = q.fin;
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int32_t key = -1;                                           // the ring, while this side still has an area to add
    long long a = 0, wa = 0;
    bool ok = c < q.B;
    OutlineJump me;
    if (ok) {
        // never: a side whose head is no head, or which lies further from it than its ring is long.  Counted (the host fails the
        // call) and left out, so that no index leaves the tables.
        me = load_jump(fin + c);
        ok = (uint32_t)me.mn < q.B && fin[(uint32_t)me.mn < q.B ? me.mn : 0].mn == me.mn;
        if (ok) {
            const RingRec* r = q.rings + q.ringno[me.mn];
            ok = me.mn == (int32_t)c || ((uint32_t)me.sf <= r->n_vertices && (uint32_t)me.d < r->n_sides);
        }
        if (!ok) atomicAdd(q.bad + 1, 1u);
    }
    if (ok) {
        const uint32_t ring = q.ringno[me.mn];
        const int32_t s = q.sid[c], k = s & 3, n = s >> 2;
        const int32_t i = n / q.cols;
        if (k == 0) { a = -(long long)i; if (q.cw) wa = -(long long)q.cw[i]; key = (int32_t)ring; }
        if (k == 2) { a = (long long)i + 1; if (q.cw) wa = (long long)q.cw[i + 1]; key = (int32_t)ring; }
        const RingRec* r = q.rings + ring;
        const bool head = me.mn == (int32_t)c;
        const uint32_t nv = r->n_vertices;
        if ((q.flag[c] && (head || me.sf > 0)) || (head && !q.flag[c] && fin[q.next[c]].sf == 0)) {
            const int32_t hs = r->head, hk = hs & 3, hj = (hs >> 2) % q.cols;
            const int32_t x0 = hj + (hk == 1 || hk == 2);
            // what lies between the head and this side is the whole ring less what lies from this side to the head
            const u64 at = r->first + (head ? 0u : nv - (uint32_t)me.sf);
            const int32_t x = head ? x0 : x0 + r->wind * q.cols - me.sx;
            q.vertices[2 * at] = i + (k >= 2);
            q.vertices[2 * at + 1] = x;
        }
    }
    u64 left = __ballot(key >= 0);
    while (left) {                                              // the trip count is the wave's
        const int first = __ffsll((long long)left) - 1;
        const int32_t kk = __shfl(key, first);
        const bool mine = key == kk;
        const u64 m = __ballot(mine);
        long long sa = mine ? a : 0, sw = mine ? wa : 0;
        if (__popcll(m) > 1)
            for (int d = 32; d >= 1; d >>= 1) { sa += __shfl_xor(sa, d); sw += __shfl_xor(sw, d); }
        if (lane == first) {
            RingRec* r = q.rings + kk;
            if (sa) atomicAdd(reinterpret_cast<u64*>(&r->area), (u64)sa);
            if (sw) atomicAdd(reinterpret_cast<u64*>(&r->warea), (u64)sw);
        }
        if (mine) key = -1;
        left &= ~m;
    }
}

// without row weights every row weighs 1
__global__ void __launch_bounds__(256) unweighted_kernel(RingRec* rings, u64 n_rings) {
    const u64 r = (u64)blockIdx.x * 256 + threadIdx.x;
    if (r < n_rings) rings[r].warea = rings[r].area;
}

}  // namespace mrtx_ol

static unsigned outline_grid(size_t n, size_t per_block) { return (unsigned)((n + per_block - 1) / per_block); }

hipError_t mrtx_launch_outline_mark(const OutlineC& q, hipStream_t st, uint32_t* launches) {
    if (q.rows < 1 || q.cols < 1 || (int64_t)q.rows * q.cols > MRTX_OL_MAX_NODES || !q.labels || !q.bits || !q.base || !q.node_sums ||
        !q.bad || !q.totals)
        return hipErrorInvalidValue;
    const size_t N = (size_t)q.rows * (size_t)q.cols;
    const unsigned chunks = outline_grid(N, MRTX_OL_CHUNK);
    hipLaunchKernelGGL(mrtx_ol::mark_kernel, dim3(chunks), dim3(256), 0, st, q);
    hipLaunchKernelGGL(mrtx_ol::scan_chunks_kernel, dim3(1), dim3(1024), 0, st, q.node_sums, chunks, q.totals);
    hipLaunchKernelGGL(mrtx_ol::base_kernel, dim3(chunks), dim3(256), 0, st, q);
    if (launches) *launches += 3;
    return hipGetLastError();
}

hipError_t mrtx_launch_outline_trace(const OutlineC& q, hipStream_t st, uint32_t* launches) {
    if (!q.B || q.B > 4 * (uint64_t)q.rows * (uint64_t)q.cols || q.rounds != outline_rounds(q.B) || !q.sid || !q.next || !q.flag ||
        !q.side_sums || !q.jump[0] || !q.jump[1] || (q.contract && (!q.jflag || !q.jidx)) ||
        q.fin != q.jump[(q.rounds & 1) ^ (q.contract ? 1 : 0)])
        return hipErrorInvalidValue;
    const size_t N = (size_t)q.rows * (size_t)q.cols;
    const unsigned gb = outline_grid(q.B, 256), chunks = outline_grid(q.B, MRTX_OL_CHUNK);
    hipLaunchKernelGGL(mrtx_ol::succ_kernel, dim3(outline_grid(N, 256)), dim3(256), 0, st, q);
    // The rounds follow from B in both variants, so that the number of launches depends on nothing else about the labels;
    // contract's elements are fewer, and the blocks beyond them leave at once.
    const unsigned long long* count = q.totals;
    if (q.contract) {
        hipLaunchKernelGGL(mrtx_ol::chain_sum_kernel, dim3(chunks), dim3(256), 0, st, q);
        hipLaunchKernelGGL(mrtx_ol::scan_chunks_kernel, dim3(1), dim3(1024), 0, st, q.side_sums, chunks, q.totals + 4);
        hipLaunchKernelGGL(mrtx_ol::chain_index_kernel, dim3(chunks), dim3(256), 0, st, q);
        hipLaunchKernelGGL(mrtx_ol::chain_init_kernel, dim3(gb), dim3(256), 0, st, q);
        count = q.totals + 4;
    } else {
        hipLaunchKernelGGL(mrtx_ol::jump_init_kernel, dim3(gb), dim3(256), 0, st, q);
    }
    for (int32_t r = 0; r < q.rounds; r++)
        hipLaunchKernelGGL(mrtx_ol::jump_kernel, dim3(gb), dim3(256), 0, st, q.jump[r & 1], q.jump[(r & 1) ^ 1], count);
    if (q.contract) hipLaunchKernelGGL(mrtx_ol::chain_down_kernel, dim3(gb), dim3(256), 0, st, q);
    hipLaunchKernelGGL(mrtx_ol::heads_sum_kernel, dim3(chunks), dim3(256), 0, st, q);
    hipLaunchKernelGGL(mrtx_ol::scan_chunks_kernel, dim3(1), dim3(1024), 0, st, q.side_sums, chunks, q.totals + 2);
    if (launches) *launches += (q.contract ? 8u : 4u) + (uint32_t)q.rounds;
    return hipGetLastError();
}

hipError_t mrtx_launch_outline_fill(const OutlineC& q, uint64_t n_rings, hipStream_t st, uint32_t* launches) {
    if (!q.B || !q.rings || !q.vertices || !q.ringno || !n_rings) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mrtx_ol::heads_write_kernel, dim3(outline_grid(q.B, MRTX_OL_CHUNK)), dim3(256), 0, st, q);
    hipLaunchKernelGGL(mrtx_ol::sides_kernel, dim3(outline_grid(q.B, 256)), dim3(256), 0, st, q);
    if (!q.cw) hipLaunchKernelGGL(mrtx_ol::unweighted_kernel, dim3(outline_grid(n_rings, 256)), dim3(256), 0, st, q.rings, n_rings);
    if (launches) *launches += q.cw ? 2 : 3;
    return hipGetLastError();
}
