// mrtx_traverse.hip -- gfx950 kernels of the traverse stage: mrtx_traverse (DESIGN.md sections 3.13 and 4.14) and
// mrtx_traverse_timed (sections 3.19 and 4.22), one tile scheme over two fields (section 4.24).
//
// A field over a window of the DEM's texel lattice, the least fixed point of x[v] = min(src[v], min_u g_uv(x[u])) with every
// g_uv non-decreasing and g_uv(x) >= x, found by one tile scheme:
//   init    the unreachable value everywhere; checks a device penalty table
//   seed    the (host-reduced) sources and the tiles they activate
//   relax   one 64-lane workgroup per active tile: x, D and P of the tile and its one-node halo into LDS, the tile's
//           incoming edges precomputed there, then directional Gauss-Seidel sweeps (down + up, right + left) until a round
//           of them lowers nothing; its own nodes written back, the neighbour tiles whose shared edge or corner changed
//           flagged for the next launch
//   pred    one lane per node: the predecessor code; source_pred: code 8 for the sources that kept their start
// The two fields are instances of it, with a kernel name per step and field:
//   CostField     traverse_{init,seed,relax,pred,source_pred}_kernel(TraverseC): float64 costs, g_uv(x) = x + w(u -> v) with
//                 the float32 edge weight w staged per edge
//   ArrivalField  timed_{init,seed,relax,pred,source_pred}_kernel(TraverseTimedC): uint64 arrival ticks, g_uv the earliest
//                 arrival over the edge under the availability table; the edge's duration in ticks and the node indices
//                 (the table's rows) staged
// init, seed, pred and source_pred are written once over a field description; the two relax kernels keep a text each (the
// shared form measured 1 to 2 % slower, section 4.24) and share the tile-flag store and the boundary mask.
// Beside them traverse_heights_kernel: one lane per node, its D (mrtx_traverse_heights, for routes).
// Memory rule: correctness never depends on seeing, within a launch, what another workgroup of that launch wrote.  The halo
// loads and the stores of x that another workgroup may read in the same launch are relaxed agent-scope 64-bit atomics (no torn
// value); a stale read only costs another launch.  Only kernel boundaries order anything.
//
// Own translation unit: the kernels of mrtx_kernels.hip and mrtx_terrain.hip are compiled exactly as before.  Build flags as there
// (-ffp-contract=off, correctly rounded /): the edge weight is the spec's float32 expression operation by operation.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mrtx_device.h"

namespace mrtx_tr {

__device__ constexpr int kDi[8] = {-1, -1, 0, 1, 1, 1, 0, -1};   // N, NE, E, SE, S, SW, W, NW: the step from v to u
__device__ constexpr int kDj[8] = {0, 1, 1, 1, 0, -1, -1, -1};

// Is window node (i, j) inside the window?  j is wrapped into [0, cols) when the window wraps.
__device__ __forceinline__ bool in_window(const TraverseC& q, int64_t i, int64_t& j) {
    if (i < 0 || i >= q.rows) return false;
    if (j < 0 || j >= q.cols) {
        if (!q.wrap) return false;
        j = j < 0 ? j + q.cols : j - q.cols;
    }
    return true;
}

// D of window node (i, j): texel (row0 + i stride, (col0 + j stride) mod W), read directly; 64-bit element offsets
__device__ __forceinline__ float node_D(const TraverseC& q, int64_t i, int64_t j) {
    const int64_t r = (int64_t)q.row0 + i * q.stride;
    const int64_t c = ((int64_t)q.col0 + j * q.stride) % q.dem_w;
    const uint64_t e = (uint64_t)(r + 2) * (uint64_t)q.dem_pitch + (uint64_t)(c + 2);
    return q.dem[e * (MRTX_DEM_ELEM_BYTES / 4)];
}

// The length of the edge between row i and row i + di (di = -1, 0, 1), dj != 0 for a diagonal: its upper row's entry
__device__ __forceinline__ float edge_len(const TraverseC& q, int64_t i, int di, int dj) {
    if (di == 0) return q.len[3 * i];
    const int64_t r = di < 0 ? i - 1 : i;
    return q.len[3 * r + (dj == 0 ? 1 : 2)];
}

// w(u -> v) in float32, in the spec's order; +inf = not driven (too steep, or an infinite penalty)
__device__ __forceinline__ float edge_w(const TraverseC& q, float Du, float Dv, float Pu, float Pv, float L) {
    const float dh = (Dv - Du) * q.rm;
    const float g = dh / L;
    if (fabsf(g) > q.gmax) return __builtin_huge_valf();
    const float c = (L + q.a_up * fmaxf(dh, 0.0f)) + q.a_dn * fmaxf(-dh, 0.0f);
    const float m = q.pen ? 0.5f * (Pu + Pv) : 1.0f;
    return c * m;
}

__device__ __forceinline__ bool penalty_ok(float p) {
    return (p >= 1e-3f && p <= 1e6f) || p == __builtin_huge_valf();
}

// Flag tile (y, x) for a relaxation launch; x wraps with the window, a tile outside the grid is none
__device__ __forceinline__ void flag_tile(const TraverseC& c, uint32_t* flags, int y, int x) {
    if (y < 0 || y >= c.tiles_y) return;
    if (x < 0 || x >= c.tiles_x) {
        if (!c.wrap) return;
        x = x < 0 ? x + c.tiles_x : x - c.tiles_x;
    }
    __hip_atomic_store(&flags[(int64_t)y * c.tiles_x + x], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Node (a, b) of a th x tw tile: the neighbour tiles that hold it in their halo (bit k = direction k)
__device__ __forceinline__ uint32_t halo_mask(int a, int b, int th, int tw) {
    const bool n_ = a == 0, s_ = a == th - 1, w_ = b == 0, e_ = b == tw - 1;
    return (n_ ? 1u : 0u) | (n_ && e_ ? 2u : 0u) | (e_ ? 4u : 0u) | (s_ && e_ ? 8u : 0u) | (s_ ? 16u : 0u) |
           (s_ && w_ ? 32u : 0u) | (w_ ? 64u : 0u) | (n_ && w_ ? 128u : 0u);
}

// The grid-stride loop of the one-lane-per-node kernels: fn(n) for the nodes of this lane
template <class Fn>
__device__ __forceinline__ void for_nodes(const TraverseC& c, Fn fn) {
    const int64_t n_nodes = (int64_t)c.rows * c.cols;
    for (int64_t n = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; n < n_nodes; n += (int64_t)gridDim.x * blockDim.x) fn(n);
}

// ---- The arrival field's own pieces (mrtx_traverse_timed, DESIGN.md sections 3.19 and 4.22) ---------------------------------
// Arrival ticks in place of costs: A[v] = min(src[v], min_u g_uv(A[u])) with g_uv(a) = start(u, v, a) + q, q the edge's
// duration in ticks and start the first tick >= a from which the q ticks of the drive lie in epochs available at both ends.
// Waiting is free, so g_uv is non-decreasing and g_uv(a) >= a + q: every store strictly lowers a uint64, and the fixed point
// does not depend on the order of the relaxations.
constexpr unsigned long long kNever = ~0ull;     // unreachable
constexpr uint32_t kNoDrive = 0u;                 // the duration sentinel: a driven edge lasts >= 1 tick

// q of an edge of weight w: x = (double)w * ticks_per_cost (one product, never contracted); 1 if x <= 1, else ceil(x); not
// driven if w is infinite or x > 2^31
__device__ __forceinline__ uint32_t edge_ticks(float w, double tpc) {
    if (w == __builtin_huge_valf()) return kNoDrive;
    const double x = (double)w * tpc;
    if (!(x <= 2147483648.0)) return kNoDrive;
    return x <= 1.0 ? 1u : (uint32_t)ceil(x);
}

// word wd of the epochs available at both nodes; the bits from epoch n_epochs on are 0 (the table ends)
__device__ __forceinline__ unsigned long long both_word(const TraverseTimedC& q, const unsigned long long* ru,
                                                        const unsigned long long* rv, int wd) {
    unsigned long long w = ru[wd] & rv[wd];
    if (wd == q.w64 - 1 && (q.n_epochs & 63)) w &= (1ull << (q.n_epochs & 63)) - 1ull;
    return w;
}

// t / d: ticks below 2^32 (every table of up to 2^32 ticks) divide in 32 bits
__device__ __forceinline__ unsigned long long div_ticks(unsigned long long t, uint32_t d) {
    return (t >> 32) ? t / d : (unsigned long long)((uint32_t)t / d);
}

// g_uv(a) for nodes nu, nv and a duration dq >= 1, or kNever.  The drive starts in the first available epoch e0 at or after
// a's; it fits if the run of available epochs from e0 reaches the epoch of its last tick.  If not, no later tick of that run
// fits either (the last tick only moves on), so the search goes on behind the first unavailable epoch.  The scan for an
// available epoch stops at word w64, the scan for an unavailable one at the word of the drive's last tick.
__device__ __forceinline__ unsigned long long timed_arrive(const TraverseTimedC& q, uint32_t nu, uint32_t nv,
                                                            unsigned long long a, uint32_t dq) {
    const unsigned long long* const ru = q.avail + (uint64_t)nu * (uint64_t)q.w64;
    const unsigned long long* const rv = q.avail + (uint64_t)nv * (uint64_t)q.w64;
    const uint32_t tpe = (uint32_t)q.tpe;
    unsigned long long t = a;
    for (;;) {
        const unsigned long long ea = div_ticks(t, tpe);
        if (ea >= (unsigned long long)q.n_epochs) return kNever;
        int e0 = (int)ea;
        // the first available epoch at or after e0 (ctz on the word)
        int wd = e0 >> 6;
        unsigned long long w = both_word(q, ru, rv, wd) & (~0ull << (e0 & 63));
        while (!w) {
            if (++wd >= q.w64) return kNever;
            w = both_word(q, ru, rv, wd);
        }
        const int e1 = (wd << 6) + (int)__builtin_ctzll(w);
        if (e1 > e0) { t = (unsigned long long)e1 * tpe; e0 = e1; }
        // the drive's last tick must lie inside the table: if it does not, no later start does either
        const unsigned long long el = div_ticks(t + dq - 1ull, tpe);
        if (el >= (unsigned long long)q.n_epochs) return kNever;
        const int last = (int)el;
        // the first unavailable epoch in e0 .. last (ctz on the complement), if any
        w = ~both_word(q, ru, rv, wd) & (~0ull << (e0 & 63));
        int z = -1;
        for (;;) {
            if (w) {
                const int c = (wd << 6) + (int)__builtin_ctzll(w);
                if (c <= last) z = c;
                break;
            }
            if (++wd > (last >> 6)) break;
            w = ~both_word(q, ru, rv, wd);
        }
        if (z < 0) return t + dq;
        t = ((unsigned long long)z + 1ull) * tpe;
    }
}

// one incoming edge of v: the arrival over it if that lowers `best`.  The test au + dq < best needs LDS only; the
// availability words are read (from global memory) only behind it.
__device__ __forceinline__ unsigned long long timed_try(const TraverseTimedC& q, unsigned long long best, unsigned long long au,
                                                         uint32_t dq, uint32_t nu, uint32_t nv) {
    if (dq == kNoDrive || au == kNever || au + dq >= best) return best;
    const unsigned long long g = q.avail ? timed_arrive(q, nu, nv, au, dq) : au + dq;
    return g < best ? g : best;
}

// ---- The two field descriptions -------------------------------------------------------------------------------------------
// What init, seed, pred and source_pred need of a field: C the kernels' constant block and win() its window; V the value type
// and kNever its "unreachable"; val() the values and start() the sources' starts; reaches(): does the edge of weight w from
// node u (value xu) to node n explain n's value xv.
struct CostField {
    using C = TraverseC;
    using V = double;
    static constexpr V kNever = __builtin_huge_val();
    static __device__ __forceinline__ const TraverseC& win(const C& q) { return q; }
    static __device__ __forceinline__ V* val(const C& q) { return q.d; }
    static __device__ __forceinline__ const V* start(const C& q) { return q.src_cost; }
    static __device__ __forceinline__ bool reaches(const C&, V xu, float w, int64_t, int64_t, V xv) {
        return w != __builtin_huge_valf() && xu + (double)w == xv;
    }
};

struct ArrivalField {
    using C = TraverseTimedC;
    using V = unsigned long long;
    static constexpr V kNever = mrtx_tr::kNever;
    static __device__ __forceinline__ const TraverseC& win(const C& q) { return q.t; }
    static __device__ __forceinline__ V* val(const C& q) { return q.arr; }
    static __device__ __forceinline__ const V* start(const C& q) { return q.src_tick; }
    static __device__ __forceinline__ bool reaches(const C& q, V xu, float w, int64_t u, int64_t n, V xv) {
        const uint32_t dq = edge_ticks(w, q.tpc);
        if (dq == kNoDrive || xu + dq > xv) return false;
        return (q.avail ? timed_arrive(q, (uint32_t)u, (uint32_t)n, xu, dq) : xu + dq) == xv;
    }
};

// ---- The steps written once over a field ---------------------------------------------------------------------------------
template <class F>
__device__ __forceinline__ void init_body(const typename F::C& q) {
    const TraverseC& c = F::win(q);
    unsigned long long bad = 0;
    for_nodes(c, [&](int64_t n) {
        F::val(q)[n] = F::kNever;
        if (c.pen && !penalty_ok(c.pen[n])) bad++;
    });
    if (bad) atomicAdd(&c.visits[1], bad);
}

// one lane per source: its start, and the 3 x 3 tiles around its own (a source on a tile's edge sits in its neighbours' halos)
template <class F>
__device__ __forceinline__ void seed_body(const typename F::C& q) {
    const TraverseC& c = F::win(q);
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= c.n_src) return;
    const int64_t n = c.src_node[s];
    F::val(q)[n] = F::start(q)[s];
    const int ty = (int)(n / c.cols) / c.tile, tx = (int)(n % c.cols) / c.tile;
    for (int a = -1; a <= 1; a++)
        for (int b = -1; b <= 1; b++) flag_tile(c, c.flag_in, ty + a, tx + b);
}

// one lane per node: 255 unreachable; else the first direction k whose neighbour u has x[u] < x[v], a driven edge and
// g_uv(x[u]) == x[v]; 254 if none (the sources get code 8 from source_pred afterwards)
template <class F>
__device__ __forceinline__ void pred_body(const typename F::C& q) {
    const TraverseC& c = F::win(q);
    for_nodes(c, [&](int64_t n) {
        const int64_t i = n / c.cols, j = n % c.cols;
        const typename F::V xv = F::val(q)[n];
        uint8_t code = 255;
        if (xv != F::kNever) {
            code = 254;
            const float Dv = node_D(c, i, j), Pv = c.pen ? c.pen[n] : 1.0f;
            for (int k = 0; k < 8; k++) {
                const int64_t ui = i + kDi[k];
                int64_t uj = j + kDj[k];
                if (!in_window(c, ui, uj)) continue;
                const int64_t u = ui * c.cols + uj;
                const typename F::V xu = F::val(q)[u];
                if (!(xu < xv)) continue;
                const float w = edge_w(c, node_D(c, ui, uj), Dv, c.pen ? c.pen[u] : 1.0f, Pv, edge_len(c, i, kDi[k], kDj[k]));
                if (F::reaches(q, xu, w, u, n, xv)) { code = (uint8_t)k; break; }
            }
        }
        c.pred[n] = code;
    });
}

template <class F>
__device__ __forceinline__ void source_pred_body(const typename F::C& q) {
    const TraverseC& c = F::win(q);
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= c.n_src) return;
    const int64_t n = c.src_node[s];
    if (F::val(q)[n] == F::start(q)[s]) c.pred[n] = 8;
}

// ---- The kernels: a name per step and field --------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) traverse_init_kernel(const TraverseC q) { init_body<CostField>(q); }
__global__ void __launch_bounds__(64) traverse_seed_kernel(const TraverseC q) { seed_body<CostField>(q); }
// the cost field's relaxation, written out (see the file comment); timed_relax_kernel below follows it step for step
template <int TS>
__global__ void __launch_bounds__(64) traverse_relax_kernel(const TraverseC q) {
    constexpr int HP = TS + 2;      // pitch of the staged D and P: the tile and its halo
    constexpr int DP = TS + 3;      // pitch of the staged costs (odd in 8-byte words: fewer bank conflicts down a column)
    constexpr int WP = TS + 1;      // pitch of the weights (odd: a column's lanes hit distinct banks)
    __shared__ double sd[HP * DP];
    __shared__ float sD[HP * HP], sP[HP * HP];
    __shared__ float sw[8 * TS * WP];
    __shared__ uint32_t s_mask;

    const int64_t t = blockIdx.x;
    if (q.flag_in[t] == 0u) return;          // not active in this launch (wave-uniform)
    const int lane = threadIdx.x;
    if (lane == 0) {
        q.flag_in[t] = 0u;                   // only this workgroup touches flag_in[t] in this launch
        s_mask = 0u;
        atomicAdd(&q.visits[0], 1ull);
    }
    const int ty = (int)(t / q.tiles_x), tx = (int)(t % q.tiles_x);
    const int64_t i0 = (int64_t)ty * TS, j0 = (int64_t)tx * TS;
    const int th = (int)min((int64_t)TS, q.rows - i0), tw = (int)min((int64_t)TS, q.cols - j0);

    // stage d, D, P of the tile and its halo (the halo's far row / column right after the tile's last one)
    for (int p = lane; p < (th + 2) * (tw + 2); p += 64) {
        const int a = p / (tw + 2) - 1, b = p % (tw + 2) - 1;
        const int64_t gi = i0 + a;
        int64_t gj = j0 + b;
        double dv = __builtin_huge_val();
        float Dv = 0.0f, Pv = 1.0f;
        if (in_window(q, gi, gj)) {
            const int64_t n = gi * q.cols + gj;
            dv = __hip_atomic_load(&q.d[n], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            Dv = node_D(q, gi, gj);
            if (q.pen) Pv = q.pen[n];
        }
        sd[(a + 1) * DP + (b + 1)] = dv;
        sD[(a + 1) * HP + (b + 1)] = Dv;
        sP[(a + 1) * HP + (b + 1)] = Pv;
    }
    __syncthreads();
    // the tile's incoming edge weights: sw[k][a][b] = w(u -> v), u = v + step k, +inf where u is no node or not driven
    for (int p = lane; p < th * tw; p += 64) {
        const int a = p / tw, b = p % tw;
        const int vi = (a + 1) * HP + (b + 1);
        for (int k = 0; k < 8; k++) {
            const int64_t gi = i0 + a + kDi[k];
            int64_t gj = j0 + b + kDj[k];
            float w = __builtin_huge_valf();
            if (in_window(q, gi, gj)) {
                const int ui = (a + 1 + kDi[k]) * HP + (b + 1 + kDj[k]);
                w = edge_w(q, sD[ui], sD[vi], sP[ui], sP[vi], edge_len(q, i0 + a, kDi[k], kDj[k]));
            }
            sw[k * TS * WP + a * WP + b] = w;
        }
    }
    __syncthreads();

    // sweeps: lanes 0-31 run down (from row a - 1: N, NE, NW) then right (from column b - 1: W, NW, SW), lanes 32-63 at the
    // same time up (S, SE, SW) then left (E, NE, SE); a lowered cost is an LDS atomic min (non-negative doubles order as
    // their bits), so the two halves never lose each other's update where they meet
    const int half = lane >> 5, x = lane & 31;
    for (;;) {
        int ch = 0;
        for (int s = 0; s < th; s++) {
            if (x < tw) {
                const int a = half ? th - 1 - s : s, da = half ? 1 : -1;
                const int kc = half ? 4 : 0, kl = half ? 5 : 7, kr = half ? 3 : 1;
                double* v = &sd[(a + 1) * DP + (x + 1)];
                const double* u = &sd[(a + 1 + da) * DP + (x + 1)];
                const int wi = a * WP + x;
                const double dv = *v;
                double c = u[0] + (double)sw[kc * TS * WP + wi];
                c = fmin(c, u[-1] + (double)sw[kl * TS * WP + wi]);
                c = fmin(c, u[1] + (double)sw[kr * TS * WP + wi]);
                if (c < dv) {
                    atomicMin(reinterpret_cast<unsigned long long*>(v), (unsigned long long)__double_as_longlong(c));
                    ch = 1;
                }
            }
            __syncthreads();
        }
        for (int s = 0; s < tw; s++) {
            if (x < th) {
                const int b = half ? tw - 1 - s : s, db = half ? 1 : -1;
                const int kc = half ? 2 : 6, ku = half ? 1 : 7, kd = half ? 3 : 5;
                double* v = &sd[(x + 1) * DP + (b + 1)];
                const double* u = v + db;
                const int wi = x * WP + b;
                const double dv = *v;
                double c = u[0] + (double)sw[kc * TS * WP + wi];
                c = fmin(c, u[-DP] + (double)sw[ku * TS * WP + wi]);
                c = fmin(c, u[DP] + (double)sw[kd * TS * WP + wi]);
                if (c < dv) {
                    atomicMin(reinterpret_cast<unsigned long long*>(v), (unsigned long long)__double_as_longlong(c));
                    ch = 1;
                }
            }
            __syncthreads();
        }
        if (!__syncthreads_or(ch)) break;
    }

    // write back what was lowered; note which neighbour tiles see a changed node in their halo (bit k = direction k)
    uint32_t mask = 0u;
    bool lowered = false;
    for (int p = lane; p < th * tw; p += 64) {
        const int a = p / tw, b = p % tw;
        const int64_t n = (i0 + a) * q.cols + (j0 + b);
        const double nv = sd[(a + 1) * DP + (b + 1)];
        if (nv < q.d[n]) {                   // only this workgroup writes its own nodes
            __hip_atomic_store(&q.d[n], nv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            lowered = true;
            mask |= halo_mask(a, b, th, tw);
        }
    }
    if (mask) atomicOr(&s_mask, mask);
    const int any = __syncthreads_or(lowered ? 1 : 0);
    if (lane == 0 && any) {
        atomicAdd(&q.changed[q.slot], 1u);
        const uint32_t m = s_mask;
        for (int k = 0; k < 8; k++)
            if (m & (1u << k)) flag_tile(q, q.flag_out, ty + kDi[k], tx + kDj[k]);
    }
}

__global__ void __launch_bounds__(256) traverse_pred_kernel(const TraverseC q) { pred_body<CostField>(q); }
__global__ void __launch_bounds__(64) traverse_source_pred_kernel(const TraverseC q) { source_pred_body<CostField>(q); }

__global__ void __launch_bounds__(256) timed_init_kernel(const TraverseTimedC q) { init_body<ArrivalField>(q); }
__global__ void __launch_bounds__(64) timed_seed_kernel(const TraverseTimedC q) { seed_body<ArrivalField>(q); }
// the arrival field's relaxation: traverse_relax_kernel's steps over uint64 ticks, durations and the staged node indices
template <int TS>
__global__ void __launch_bounds__(64) timed_relax_kernel(const TraverseTimedC q) {
    constexpr int HP = TS + 2;      // pitch of the staged D, P and node indices: the tile and its halo
    constexpr int DP = TS + 3;      // pitch of the staged arrivals (odd in 8-byte words: fewer bank conflicts down a column)
    constexpr int WP = TS + 1;      // pitch of the durations (odd: a column's lanes hit distinct banks)
    __shared__ unsigned long long sa[HP * DP];
    __shared__ float sD[HP * HP], sP[HP * HP];
    __shared__ uint32_t sn[HP * HP];
    __shared__ uint32_t sq[8 * TS * WP];
    __shared__ uint32_t s_mask;

    const TraverseC& c = q.t;
    const int64_t t = blockIdx.x;
    if (c.flag_in[t] == 0u) return;          // not active in this launch (wave-uniform)
    const int lane = threadIdx.x;
    if (lane == 0) {
        c.flag_in[t] = 0u;                   // only this workgroup touches flag_in[t] in this launch
        s_mask = 0u;
        atomicAdd(&c.visits[0], 1ull);
    }
    const int ty = (int)(t / c.tiles_x), tx = (int)(t % c.tiles_x);
    const int64_t i0 = (int64_t)ty * TS, j0 = (int64_t)tx * TS;
    const int th = (int)min((int64_t)TS, c.rows - i0), tw = (int)min((int64_t)TS, c.cols - j0);

    // stage A, D, P and the node index of the tile and its halo
    for (int p = lane; p < (th + 2) * (tw + 2); p += 64) {
        const int a = p / (tw + 2) - 1, b = p % (tw + 2) - 1;
        const int64_t gi = i0 + a;
        int64_t gj = j0 + b;
        unsigned long long av = kNever;
        float Dv = 0.0f, Pv = 1.0f;
        uint32_t nn = 0u;
        if (in_window(c, gi, gj)) {
            const int64_t n = gi * c.cols + gj;
            av = __hip_atomic_load(&q.arr[n], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            Dv = node_D(c, gi, gj);
            if (c.pen) Pv = c.pen[n];
            nn = (uint32_t)n;
        }
        sa[(a + 1) * DP + (b + 1)] = av;
        sD[(a + 1) * HP + (b + 1)] = Dv;
        sP[(a + 1) * HP + (b + 1)] = Pv;
        sn[(a + 1) * HP + (b + 1)] = nn;
    }
    __syncthreads();
    // the tile's incoming durations: sq[k][a][b] = q(u -> v), u = v + step k, kNoDrive where u is no node or not driven
    for (int p = lane; p < th * tw; p += 64) {
        const int a = p / tw, b = p % tw;
        const int vi = (a + 1) * HP + (b + 1);
        for (int k = 0; k < 8; k++) {
            const int64_t gi = i0 + a + kDi[k];
            int64_t gj = j0 + b + kDj[k];
            uint32_t dq = kNoDrive;
            if (in_window(c, gi, gj)) {
                const int ui = (a + 1 + kDi[k]) * HP + (b + 1 + kDj[k]);
                dq = edge_ticks(edge_w(c, sD[ui], sD[vi], sP[ui], sP[vi], edge_len(c, i0 + a, kDi[k], kDj[k])), q.tpc);
            }
            sq[k * TS * WP + a * WP + b] = dq;
        }
    }
    __syncthreads();

    // sweeps as in traverse_relax_kernel: lanes 0-31 down then right, lanes 32-63 up then left; a lowered arrival is an LDS
    // atomic min on the uint64, so the two halves never lose each other's update where they meet
    const int half = lane >> 5, x = lane & 31;
    for (;;) {
        int ch = 0;
        for (int s = 0; s < th; s++) {
            if (x < tw) {
                const int a = half ? th - 1 - s : s, da = half ? 1 : -1;
                const int kc = half ? 4 : 0, kl = half ? 5 : 7, kr = half ? 3 : 1;
                unsigned long long* v = &sa[(a + 1) * DP + (x + 1)];
                const unsigned long long* u = &sa[(a + 1 + da) * DP + (x + 1)];
                const uint32_t* nu = &sn[(a + 1 + da) * HP + (x + 1)];
                const uint32_t nv = sn[(a + 1) * HP + (x + 1)];
                const int wi = a * WP + x;
                const unsigned long long av = *v;
                unsigned long long g = timed_try(q, av, u[0], sq[kc * TS * WP + wi], nu[0], nv);
                g = timed_try(q, g, u[-1], sq[kl * TS * WP + wi], nu[-1], nv);
                g = timed_try(q, g, u[1], sq[kr * TS * WP + wi], nu[1], nv);
                if (g < av) {
                    atomicMin(v, g);
                    ch = 1;
                }
            }
            __syncthreads();
        }
        for (int s = 0; s < tw; s++) {
            if (x < th) {
                const int b = half ? tw - 1 - s : s, db = half ? 1 : -1;
                const int kc = half ? 2 : 6, ku = half ? 1 : 7, kd = half ? 3 : 5;
                unsigned long long* v = &sa[(x + 1) * DP + (b + 1)];
                const unsigned long long* u = v + db;
                const uint32_t* nu = &sn[(x + 1) * HP + (b + 1 + db)];
                const uint32_t nv = sn[(x + 1) * HP + (b + 1)];
                const int wi = x * WP + b;
                const unsigned long long av = *v;
                unsigned long long g = timed_try(q, av, u[0], sq[kc * TS * WP + wi], nu[0], nv);
                g = timed_try(q, g, u[-DP], sq[ku * TS * WP + wi], nu[-HP], nv);
                g = timed_try(q, g, u[DP], sq[kd * TS * WP + wi], nu[HP], nv);
                if (g < av) {
                    atomicMin(v, g);
                    ch = 1;
                }
            }
            __syncthreads();
        }
        if (!__syncthreads_or(ch)) break;
    }

    // write back what was lowered; note which neighbour tiles see a changed node in their halo (bit k = direction k)
    uint32_t mask = 0u;
    bool lowered = false;
    for (int p = lane; p < th * tw; p += 64) {
        const int a = p / tw, b = p % tw;
        const int64_t n = (i0 + a) * c.cols + (j0 + b);
        const unsigned long long nv = sa[(a + 1) * DP + (b + 1)];
        if (nv < q.arr[n]) {                 // only this workgroup writes its own nodes
            __hip_atomic_store(&q.arr[n], nv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            lowered = true;
            mask |= halo_mask(a, b, th, tw);
        }
    }
    if (mask) atomicOr(&s_mask, mask);
    const int any = __syncthreads_or(lowered ? 1 : 0);
    if (lane == 0 && any) {
        atomicAdd(&c.changed[c.slot], 1u);
        const uint32_t m = s_mask;
        for (int k = 0; k < 8; k++)
            if (m & (1u << k)) flag_tile(c, c.flag_out, ty + kDi[k], tx + kDj[k]);
    }
}

__global__ void __launch_bounds__(256) timed_pred_kernel(const TraverseTimedC q) { pred_body<ArrivalField>(q); }
__global__ void __launch_bounds__(64) timed_source_pred_kernel(const TraverseTimedC q) { source_pred_body<ArrivalField>(q); }

// one lane per node: its D, for the heights along a route (mrtx_traverse_heights)
__global__ void __launch_bounds__(256) traverse_heights_kernel(const TraverseC q, float* __restrict__ out) {
    const int64_t n_nodes = (int64_t)q.rows * q.cols;
    for (int64_t n = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; n < n_nodes; n += (int64_t)gridDim.x * blockDim.x)
        out[n] = node_D(q, n / q.cols, n % q.cols);
}

}  // namespace mrtx_tr

// ---- The launchers: one implementation per step, over either field's block Q ---------------------------------------------
static unsigned traverse_grid(int64_t n, int per_block) {
    const int64_t b = (n + per_block - 1) / per_block;
    return (unsigned)(b < 1 ? 1 : b > 65536 ? 65536 : b);
}

static const TraverseC& window_of(const TraverseC& q) { return q; }
static const TraverseC& window_of(const TraverseTimedC& q) { return q.t; }
// the field's own members: the values and the starts; the tick scales and the table's shape
static bool field_ok(const TraverseC& q) { return q.d && q.src_cost; }
static bool field_ok(const TraverseTimedC& q) {
    return q.arr && q.src_tick && q.tpe >= 1 && q.tpc > 0.0 &&
           (!q.avail || (q.n_epochs >= 1 && q.n_epochs <= (1 << 24) && q.w64 == (q.n_epochs + 63) / 64));
}

// the unreachable value everywhere, the device penalty check (into visits[1]), then the sources and their tiles (into flag_in)
template <class Q>
static hipError_t launch_init(const Q& q, void (*init)(Q), void (*seed)(Q), hipStream_t st) {
    const TraverseC& c = window_of(q);
    if (c.rows < 1 || c.cols < 1 || c.n_src < 1 || !c.visits || !c.flag_in || !c.src_node || !field_ok(q)) return hipErrorInvalidValue;
    const int64_t n = (int64_t)c.rows * c.cols;
    hipLaunchKernelGGL(init, dim3(traverse_grid(n, 256)), dim3(256), 0, st, q);
    hipLaunchKernelGGL(seed, dim3((unsigned)((c.n_src + 63) / 64)), dim3(64), 0, st, q);
    return hipGetLastError();
}

// one relaxation launch over every tile (the inactive ones return at once)
template <class Q>
static hipError_t launch_relax(const Q& q, void (*relax8)(Q), void (*relax16)(Q), void (*relax32)(Q), hipStream_t st) {
    const TraverseC& c = window_of(q);
    const int64_t tiles = (int64_t)c.tiles_x * c.tiles_y;
    if (tiles < 1 || tiles > 0xFFFFFFFFll || !c.flag_in || !c.flag_out || !c.changed || !c.len || !field_ok(q)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)tiles), block(64);
    switch (c.tile) {
        case 8: hipLaunchKernelGGL(relax8, grid, block, 0, st, q); break;
        case 16: hipLaunchKernelGGL(relax16, grid, block, 0, st, q); break;
        case 32: hipLaunchKernelGGL(relax32, grid, block, 0, st, q); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

template <class Q>
static hipError_t launch_pred(const Q& q, void (*pred)(Q), void (*source_pred)(Q), hipStream_t st) {
    const TraverseC& c = window_of(q);
    if (c.rows < 1 || c.cols < 1 || !c.pred || !c.len || !c.src_node || !field_ok(q)) return hipErrorInvalidValue;
    const int64_t n = (int64_t)c.rows * c.cols;
    hipLaunchKernelGGL(pred, dim3(traverse_grid(n, 256)), dim3(256), 0, st, q);
    hipLaunchKernelGGL(source_pred, dim3((unsigned)((c.n_src + 63) / 64)), dim3(64), 0, st, q);
    return hipGetLastError();
}

hipError_t mrtx_launch_traverse_init(const TraverseC& q, hipStream_t st) {
    return launch_init(q, mrtx_tr::traverse_init_kernel, mrtx_tr::traverse_seed_kernel, st);
}
hipError_t mrtx_launch_traverse_relax(const TraverseC& q, hipStream_t st) {
    return launch_relax(q, mrtx_tr::traverse_relax_kernel<8>, mrtx_tr::traverse_relax_kernel<16>, mrtx_tr::traverse_relax_kernel<32>, st);
}
hipError_t mrtx_launch_traverse_pred(const TraverseC& q, hipStream_t st) {
    return launch_pred(q, mrtx_tr::traverse_pred_kernel, mrtx_tr::traverse_source_pred_kernel, st);
}
hipError_t mrtx_launch_timed_init(const TraverseTimedC& q, hipStream_t st) {
    return launch_init(q, mrtx_tr::timed_init_kernel, mrtx_tr::timed_seed_kernel, st);
}
hipError_t mrtx_launch_timed_relax(const TraverseTimedC& q, hipStream_t st) {
    return launch_relax(q, mrtx_tr::timed_relax_kernel<8>, mrtx_tr::timed_relax_kernel<16>, mrtx_tr::timed_relax_kernel<32>, st);
}
hipError_t mrtx_launch_timed_pred(const TraverseTimedC& q, hipStream_t st) {
    return launch_pred(q, mrtx_tr::timed_pred_kernel, mrtx_tr::timed_source_pred_kernel, st);
}

hipError_t mrtx_launch_traverse_heights(const TraverseC& q, float* out, hipStream_t st) {
    if (q.rows < 1 || q.cols < 1 || !q.dem || !out) return hipErrorInvalidValue;
    const int64_t n = (int64_t)q.rows * q.cols;
    hipLaunchKernelGGL(mrtx_tr::traverse_heights_kernel, dim3(traverse_grid(n, 256)), dim3(256), 0, st, q, out);
    return hipGetLastError();
}
