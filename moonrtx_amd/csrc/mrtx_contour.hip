// mrtx_contour.hip -- the contour lines (mrtx_contours; DESIGN.md sections 3.26, 4.32): the crossings of a lattice of integer
// heights with a table of levels, compacted in ascending (edge, level), their partial successor map, and its paths (open
// lines) and cycles (closed lines) found and ranked by pointer jumping along the predecessors.
// All integer work; every atomic is an integer count of something that never happens or of a bad input, so no byte depends on
// a schedule.
#include "mrtx_contour.h"
#include "mrtx_lattice_dev.h"

namespace mrtx_ct {
using u64 = unsigned long long;
using namespace mrtx_lat;       // add2, block_scan

// the number of levels <= z: the node is above level l iff l < rank.  MRTX_CT_NORANK for a void node and for a height outside
// the range, which *nbad (if given) counts.
template <typename T>
__device__ __forceinline__ uint32_t rank_of(T tab, int32_t n_levels, int32_t z, uint32_t* nbad) {
    if (z < -MRTX_CT_ZMAX || z > MRTX_CT_ZMAX) {
        if (z != MRTX_CT_VOID && nbad) (*nbad)++;
        return MRTX_CT_NORANK;
    }
    int32_t lo = 0, hi = n_levels;              // tab[l] <= z for l < lo, tab[l] > z for l >= hi
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (tab[mid] <= z) lo = mid + 1; else hi = mid;
    }
    return (uint32_t)lo;
}

// the node at the other end of edge k of node v = (i, j), or -1 where the edge is absent
__device__ __forceinline__ int32_t other_end(const ContourC& q, int32_t v, int32_t i, int32_t j, int k) {
    if (k == 0) return j + 1 < q.cols ? v + 1 : q.wrap ? v - j : -1;
    return i + 1 < q.rows ? v + q.cols : -1;
}

__device__ __forceinline__ uint32_t crossings(uint32_t ra, uint32_t rb) {
    if (ra == MRTX_CT_NORANK || rb == MRTX_CT_NORANK) return 0;
    return ra > rb ? ra - rb : rb - ra;
}

// One thread per node, eight nodes a thread: its rank, the check of its height and the number of levels that cross its two
// edges, left in base[] for base_kernel; the chunk's sum.
template <bool LDS>
__global__ void __launch_bounds__(256) count_kernel(const ContourC q) {
    __shared__ int32_t lv[LDS ? MRTX_CT_LDS_LEVELS : 1];
    __shared__ u64 sh[4];
    if (LDS) {
        for (int32_t l = threadIdx.x; l < q.n_levels; l += 256) lv[l] = q.levels[l];
        __syncthreads();
    }
    const int32_t N = q.rows * q.cols;
    uint32_t sum = 0, nbad = 0;
    for (int e = 0; e < 8; e++) {
        const int64_t n64 = (int64_t)blockIdx.x * MRTX_CT_CHUNK + e * 256 + threadIdx.x;
        if (n64 >= N) break;
        const int32_t n = (int32_t)n64, i = n / q.cols, j = n - i * q.cols;
        const int32_t ev = other_end(q, n, i, j, 0), sv = other_end(q, n, i, j, 1);
        const int32_t z = q.z[n], ze = ev >= 0 ? q.z[ev] : MRTX_CT_VOID, zs = sv >= 0 ? q.z[sv] : MRTX_CT_VOID;
        uint32_t r, re, rs;
        if (LDS) {
            r = rank_of(lv, q.n_levels, z, &nbad); re = rank_of(lv, q.n_levels, ze, nullptr); rs = rank_of(lv, q.n_levels, zs, nullptr);
        } else {
            r = rank_of(q.levels, q.n_levels, z, &nbad); re = rank_of(q.levels, q.n_levels, ze, nullptr);
            rs = rank_of(q.levels, q.n_levels, zs, nullptr);
        }
        const uint32_t c0 = crossings(r, re), c1 = crossings(r, rs);
        q.rank[n] = r;
        reinterpret_cast<uint2*>(q.base)[n] = make_uint2(c0, c1);
        sum += c0 + c1;
    }
    if (nbad) atomicAdd(q.bad, nbad);
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d);    // at most 2^28 a chunk
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) q.node_sums[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

// One block: the chunks' sums become their exclusive prefix sums in place; *total receives the grand total.  64-bit: the
// number of elements may exceed 2^32, which the host then refuses.
__global__ void __launch_bounds__(1024) scan_nodes_kernel(u64* sums, uint32_t n, u64* total) {
    __shared__ u64 sh[16];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    u64 carry = 0;
    for (uint32_t at = 0; at < n; at += 1024) {                 // the trip count is the block's
        const uint32_t idx = at + threadIdx.x;
        const u64 v = idx < n ? sums[idx] : 0;
        u64 inc = v;
        for (int d = 1; d < 64; d <<= 1) {
            const u64 a = __shfl_up(inc, d);
            if (lane >= d) inc += a;
        }
        __syncthreads();
        if (lane == 63) sh[w] = inc;
        __syncthreads();
        u64 off = carry, tot = 0;
        for (int k = 0; k < 16; k++) {
            const u64 s = sh[k];
            if (k < w) off += s;
            tot += s;
        }
        if (idx < n) sums[idx] = off + inc - v;
        carry += tot;
    }
    if (threadIdx.x == 0) *total = carry;
}

// the same over pairs of 32-bit sums (the heads and their vertices: both below 2^31); totals[0], totals[1] receive the totals
__global__ void __launch_bounds__(1024) scan_chunks_kernel(uint2* sums, uint32_t n, u64* totals) {
    __shared__ uint2 sh[16];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint2 carry = make_uint2(0, 0);
    for (uint32_t at = 0; at < n; at += 1024) {                 // the trip count is the block's
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

// Eight nodes in a row per thread: the counts in base[] become the exclusive prefix sums.  Modulo 2^32: the host refuses a
// total of 2^31 or more before anything reads them.
__global__ void __launch_bounds__(256) base_kernel(const ContourC q) {
    __shared__ uint2 sh[4];
    const int32_t N = q.rows * q.cols;
    const int64_t n0 = (int64_t)blockIdx.x * MRTX_CT_CHUNK + threadIdx.x * 8;
    uint2* const base2 = reinterpret_cast<uint2*>(q.base);
    uint2 c[8];
    uint32_t cnt = 0;
    for (int e = 0; e < 8; e++) {
        c[e] = n0 + e < N ? base2[n0 + e] : make_uint2(0, 0);
        cnt += c[e].x + c[e].y;
    }
    uint2 total;
    uint32_t at = (uint32_t)q.node_sums[blockIdx.x] + block_scan(make_uint2(cnt, 0), sh, &total).x;
    for (int e = 0; e < 8; e++)
        if (n0 + e < N) {
            base2[n0 + e] = make_uint2(at, at + c[e].x);
            at += c[e].x + c[e].y;
        }
}

// One thread per edge: the edge id of each of its elements.  An edge has at most n_levels of them, and most have none or one.
__global__ void __launch_bounds__(256) expand_kernel(const ContourC q) {
    const int64_t E = 2 * (int64_t)q.rows * q.cols;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const uint32_t a = q.base[e], b = e + 1 < E ? q.base[e + 1] : q.B;
    if (a > b || b > q.B || b - a > (uint32_t)q.n_levels) {     // never: the prefix sums ascend to B
        atomicAdd(q.bad + 1, 1u);
        return;
    }
    for (uint32_t k = a; k < b; k++) q.eid[k] = (int32_t)e;
}

__device__ __forceinline__ int32_t sel4(int32_t a0, int32_t a1, int32_t a2, int32_t a3, int k) {
    return k == 0 ? a0 : k == 1 ? a1 : k == 2 ? a2 : a3;
}

// The element paired with side s of cell (ci, cj) at level index l, as a compact index: the exit that belongs to the entry s
// (entering) or the entry that belongs to the exit s.  -1 when the cell does not exist or has a void corner.  Sides clockwise:
// 0 N (NW -> NE), 1 E (NE -> SE), 2 S (SE -> SW), 3 W (SW -> NW); corner k is where side k starts.
__device__ __forceinline__ int32_t partner(const ContourC& q, int32_t ci, int32_t cj, int s, uint32_t l, bool entering, uint32_t* nbad) {
    if (ci < 0 || ci >= q.rows - 1) return -1;
    if (cj < 0) {
        if (!q.wrap) return -1;
        cj = q.cols - 1;
    }
    int32_t cj1 = cj + 1;
    if (cj1 >= q.cols) {
        if (!q.wrap) return -1;
        cj1 = 0;
    }
    const int32_t v0 = ci * q.cols + cj, v1 = ci * q.cols + cj1, v2 = v1 + q.cols, v3 = v0 + q.cols;
    const uint32_t r0 = q.rank[v0], r1 = q.rank[v1], r2 = q.rank[v2], r3 = q.rank[v3];
    if (r0 == MRTX_CT_NORANK || r1 == MRTX_CT_NORANK || r2 == MRTX_CT_NORANK || r3 == MRTX_CT_NORANK) return -1;
    const uint32_t ab = (l < r0 ? 1u : 0u) | (l < r1 ? 2u : 0u) | (l < r2 ? 4u : 0u) | (l < r3 ? 8u : 0u);
    const uint32_t rot = ((ab >> 1) | (ab << 3)) & 15u;         // bit k: the corner where side k ends is above
    const uint32_t ent = ab & ~rot & 15u, ext = ~ab & rot & 15u;
    if (!((entering ? ent : ext) >> s & 1u)) {                  // never: the element crosses side s the way it was said to
        (*nbad)++;
        return -1;
    }
    int t;
    if (__popc(ent) == 2) {
        // the saddle: the integer centre test, in int64
        const long long c = q.levels[l];
        const long long sum = (long long)q.z[v0] + q.z[v1] + q.z[v2] + q.z[v3];
        const bool centre = sum >= 4 * c - 2;
        t = centre == entering ? (s + 1) & 3 : (s + 3) & 3;
    } else {
        t = __ffs((int)(entering ? ext : ent)) - 1;
    }
    const int32_t e = t == 0 ? 2 * v0 : t == 1 ? 2 * v1 + 1 : t == 2 ? 2 * v3 : 2 * v0 + 1;
    const uint32_t ra = sel4((int32_t)r0, (int32_t)r1, (int32_t)r2, (int32_t)r3, t);
    const uint32_t rb = sel4((int32_t)r1, (int32_t)r2, (int32_t)r3, (int32_t)r0, t);
    const uint32_t lo = ra < rb ? ra : rb;
    const uint32_t at = q.base[e] + (l - lo);
    if (l < lo || at >= q.B || q.eid[at] != e) {                // never: the partner is a crossed edge.  Counted, and the host
        (*nbad)++;                                              // fails the call; the line ends here, inside the tables
        return -1;
    }
    return (int32_t)at;
}

// One thread per element: its successor, and its predecessor as the first window of the pointer jumping.  The rule is
// symmetric, so each entry has one writer.
__global__ void __launch_bounds__(256) succ_kernel(const ContourC q) {
    const int64_t k64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k64 >= q.B) return;
    const int32_t k = (int32_t)k64;
    const int32_t N = q.rows * q.cols;
    const int32_t e = q.eid[k];
    uint32_t nbad = 0;
    int32_t su = -1, pr = -1;
    bool ok = (uint32_t)e < 2u * (uint32_t)N;
    if (ok) {
        const int32_t v = e >> 1, d = e & 1, i = v / q.cols, j = v - i * q.cols;
        const int32_t o = other_end(q, v, i, j, d);
        const uint32_t ra = q.rank[v], rb = o >= 0 ? q.rank[o] : MRTX_CT_NORANK;
        const uint32_t lo = ra < rb ? ra : rb, l = lo + ((uint32_t)k - q.base[e]);
        // never: an element that is no crossing of its edge
        ok = crossings(ra, rb) != 0 && (uint32_t)k >= q.base[e] && l < (ra < rb ? rb : ra) && l < (uint32_t)q.n_levels;
        if (ok) {
            const bool own = l < ra;                            // the edge's own node is above, the other end below
            int32_t ei, ej, xi, xj;                             // the cell it enters and the cell it leaves
            int es, xs;
            if (d == 0) {       // N side of cell (i, j), NW -> NE; S side of cell (i - 1, j), SE -> SW
                ei = own ? i : i - 1; ej = j; es = own ? 0 : 2;
                xi = own ? i - 1 : i; xj = j; xs = own ? 2 : 0;
            } else {            // E side of cell (i, j - 1), NE -> SE; W side of cell (i, j), SW -> NW
                ei = i; ej = own ? j - 1 : j; es = own ? 1 : 3;
                xi = i; xj = own ? j : j - 1; xs = own ? 3 : 1;
            }
            su = partner(q, ei, ej, es, l, true, &nbad);
            pr = partner(q, xi, xj, xs, l, false, &nbad);
        }
    }
    if (!ok) nbad++;
    if (nbad) atomicAdd(q.bad + 1, nbad);
    q.succ[k] = su;
    q.jump[0][k] = make_int4(pr, k, 0, 1);
}

// One round: a window and the one before it become one.  A window that holds a start keeps it and stops.  Else the nearer
// window keeps the least index at a tie, so that z stays the distance from its first occurrence once a window goes round its
// cycle more than once; its length is used only before that, and is added without sign so that it may wrap afterwards.
__global__ void __launch_bounds__(256) jump_kernel(const ContourJump* __restrict__ src, ContourJump* __restrict__ dst, uint32_t B) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= B) return;
    int4 a = src[c];
    if ((uint32_t)a.x < B) {
        const int4 b = src[a.x];
        if (b.x < 0 || b.y < a.y) { a.y = b.y; a.z = (int32_t)((uint32_t)a.w + (uint32_t)b.z); }
        a.w = (int32_t)((uint32_t)a.w + (uint32_t)b.w);
        a.x = b.x;
    }
    dst[c] = a;
}

// One thread per element: the last element of a line (it has no successor, or its successor is the head) hands the line's
// length and itself to the head.  One writer per head.
__global__ void __launch_bounds__(256) tails_kernel(const ContourC q) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= q.B) return;
    const int4 me = q.fin[k];
    const int32_t su = q.succ[k];
    if ((uint32_t)me.y >= q.B || (uint32_t)me.z >= q.B) {       // never
        atomicAdd(q.bad + 1, 1u);
        return;
    }
    if (su < 0 || su == me.y) {
        q.len[me.y] = (uint32_t)me.z + 1u;
        q.tailat[me.y] = (int32_t)k;
    }
}

// (1, its line's vertices) at a line's head, (0, 0) elsewhere
__device__ __forceinline__ uint2 head_value(const ContourC& q, int64_t k) {
    if (q.fin[k].y != (int32_t)k) return make_uint2(0, 0);
    return make_uint2(1, q.len[k]);
}

__global__ void __launch_bounds__(256) heads_sum_kernel(const ContourC q) {
    __shared__ uint2 sh[4];
    const int64_t k0 = (int64_t)blockIdx.x * MRTX_CT_CHUNK + threadIdx.x * 8;
    uint2 v = make_uint2(0, 0);
    for (int e = 0; e < 8; e++)
        if (k0 + e < q.B) v = add2(v, head_value(q, k0 + e));
    uint2 total;
    block_scan(v, sh, &total);
    if (threadIdx.x == 0) q.side_sums[blockIdx.x] = total;
}

// the line records and every head's line number
__global__ void __launch_bounds__(256) heads_write_kernel(const ContourC q, uint32_t n_lines) {
    __shared__ uint2 sh[4];
    const int32_t N = q.rows * q.cols;
    const int64_t k0 = (int64_t)blockIdx.x * MRTX_CT_CHUNK + threadIdx.x * 8;
    uint2 v = make_uint2(0, 0);
    for (int e = 0; e < 8; e++)
        if (k0 + e < q.B) v = add2(v, head_value(q, k0 + e));
    uint2 total;
    uint2 at = add2(q.side_sums[blockIdx.x], block_scan(v, sh, &total));
    for (int e = 0; e < 8; e++) {
        const int64_t k = k0 + e;
        if (k >= q.B) break;
        const uint2 h = head_value(q, k);
        if (!h.x) continue;
        const int32_t ed = q.eid[k], ta = q.tailat[k];
        // never: more heads than were counted, a head on no edge, at no level or without a tail.  Counted, and left out.
        bool ok = at.x < n_lines && (uint32_t)ed < 2u * (uint32_t)N && (uint32_t)ta < q.B;
        uint32_t l = 0;
        if (ok) {
            const int32_t vv = ed >> 1, i = vv / q.cols, j = vv - i * q.cols, o = other_end(q, vv, i, j, ed & 1);
            const uint32_t ra = q.rank[vv], rb = o >= 0 ? q.rank[o] : MRTX_CT_NORANK;
            l = (ra < rb ? ra : rb) + ((uint32_t)k - q.base[ed]);
            ok = l < (uint32_t)q.n_levels;
        }
        if (ok) {
            ContourLineRec r;
            r.first = at.y;
            r.n_vertices = h.y;
            r.level_index = (int32_t)l;
            r.level = q.levels[l];
            r.head = ed;
            r.tail = q.eid[ta];
            r.closed = q.fin[k].x >= 0 ? 1u : 0u;
            q.lines[at.x] = r;
            q.lineno[k] = at.x;
        } else {
            atomicAdd(q.bad + 1, 1u);
            q.lineno[k] = 0xFFFFFFFFu;
        }
        at = add2(at, h);
    }
}

// One thread per element: its edge id at its line's first vertex plus its distance from the head
__global__ void __launch_bounds__(256) vertices_kernel(const ContourC q, uint32_t n_lines) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= q.B) return;
    // never: an element whose head is no head, or which lies further from it than its line is long.  Counted (the host fails the
    // call) and left out, so that no index leaves the tables.
    const int4 me = q.fin[k];
    bool ok = (uint32_t)me.y < q.B && q.fin[(uint32_t)me.y < q.B ? me.y : 0].y == me.y;
    u64 at = 0;
    if (ok) {
        const uint32_t line = q.lineno[me.y];
        ok = line < n_lines;
        if (ok) {
            const ContourLineRec* r = q.lines + line;
            at = r->first + (uint32_t)me.z;
            ok = (uint32_t)me.z < r->n_vertices && at < q.B;
        }
    }
    if (ok) q.vertices[at] = q.eid[k];
    else atomicAdd(q.bad + 1, 1u);
}

}  // namespace mrtx_ct

static unsigned contour_grid(size_t n, size_t per_block) { return (unsigned)((n + per_block - 1) / per_block); }

hipError_t mrtx_launch_contour_count(const ContourC& q, hipStream_t st, uint32_t* launches) {
    if (q.rows < 1 || q.cols < 1 || (int64_t)q.rows * q.cols > MRTX_CT_MAX_NODES || q.n_levels < 1 || q.n_levels > MRTX_CT_MAX_LEVELS ||
        !q.z || !q.levels || !q.rank || !q.base || !q.node_sums || !q.bad || !q.totals)
        return hipErrorInvalidValue;
    const size_t N = (size_t)q.rows * (size_t)q.cols;
    const unsigned chunks = contour_grid(N, MRTX_CT_CHUNK);
    if (q.n_levels <= MRTX_CT_LDS_LEVELS) hipLaunchKernelGGL(mrtx_ct::count_kernel<true>, dim3(chunks), dim3(256), 0, st, q);
    else hipLaunchKernelGGL(mrtx_ct::count_kernel<false>, dim3(chunks), dim3(256), 0, st, q);
    hipLaunchKernelGGL(mrtx_ct::scan_nodes_kernel, dim3(1), dim3(1024), 0, st, q.node_sums, chunks, q.totals);
    hipLaunchKernelGGL(mrtx_ct::base_kernel, dim3(chunks), dim3(256), 0, st, q);
    if (launches) *launches += 3;
    return hipGetLastError();
}

hipError_t mrtx_launch_contour_trace(const ContourC& q, hipStream_t st, uint32_t* launches) {
    if (!q.B || q.B >= ((uint32_t)1 << 31) || q.rounds != contour_rounds(q.B) || !q.eid || !q.succ || !q.len || !q.tailat ||
        !q.side_sums || !q.jump[0] || !q.jump[1] || q.fin != q.jump[q.rounds & 1])
        return hipErrorInvalidValue;
    const size_t N = (size_t)q.rows * (size_t)q.cols;
    const unsigned gb = contour_grid(q.B, 256), chunks = contour_grid(q.B, MRTX_CT_CHUNK);
    hipLaunchKernelGGL(mrtx_ct::expand_kernel, dim3(contour_grid(2 * N, 256)), dim3(256), 0, st, q);
    hipLaunchKernelGGL(mrtx_ct::succ_kernel, dim3(gb), dim3(256), 0, st, q);
    // the rounds follow from B, so that the number of launches depends on nothing else about the heights
    for (int32_t r = 0; r < q.rounds; r++)
        hipLaunchKernelGGL(mrtx_ct::jump_kernel, dim3(gb), dim3(256), 0, st, q.jump[r & 1], q.jump[(r & 1) ^ 1], q.B);
    hipLaunchKernelGGL(mrtx_ct::tails_kernel, dim3(gb), dim3(256), 0, st, q);
    hipLaunchKernelGGL(mrtx_ct::heads_sum_kernel, dim3(chunks), dim3(256), 0, st, q);
    hipLaunchKernelGGL(mrtx_ct::scan_chunks_kernel, dim3(1), dim3(1024), 0, st, q.side_sums, chunks, q.totals + 2);
    if (launches) *launches += 5u + (uint32_t)q.rounds;
    return hipGetLastError();
}

hipError_t mrtx_launch_contour_fill(const ContourC& q, uint64_t n_lines, hipStream_t st, uint32_t* launches) {
    if (!q.B || !q.lines || !q.vertices || !q.lineno || !n_lines || n_lines > q.B) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mrtx_ct::heads_write_kernel, dim3(contour_grid(q.B, MRTX_CT_CHUNK)), dim3(256), 0, st, q, (uint32_t)n_lines);
    hipLaunchKernelGGL(mrtx_ct::vertices_kernel, dim3(contour_grid(q.B, 256)), dim3(256), 0, st, q, (uint32_t)n_lines);
    if (launches) *launches += 2;
    return hipGetLastError();
}
