// mrtx_traverse.hip -- gfx950 kernels of the least-cost traverse stage (mrtx_traverse, DESIGN.md sections 3.13 and 4.14).
//
// A cost field over a window of the DEM's texel lattice, the least fixed point of d[v] = min(src[v], min_u d[u] + w(u -> v)):
//   traverse_init_kernel   +inf everywhere; checks a device penalty table
//   traverse_seed_kernel   the (host-reduced) sources and the tiles they activate
//   traverse_relax_kernel  one 64-lane workgroup per active tile: d, D and P of the tile and its one-node halo into LDS, the
//                          tile's incoming edge weights precomputed there, then directional Gauss-Seidel sweeps (down + up,
//                          right + left) until a round of them lowers nothing; its own nodes written back, the neighbour tiles
//                          whose shared edge or corner changed flagged for the next launch
//   traverse_pred_kernel   one lane per node: the predecessor code
//   traverse_heights_kernel  one lane per node: its D (mrtx_traverse_heights, for routes)
// Memory rule: correctness never depends on seeing, within a launch, what another workgroup of that launch wrote.  The halo
// loads and the stores of d that another workgroup may read in the same launch are relaxed agent-scope 64-bit atomics (no torn
// double); a stale read only costs another launch.  Only kernel boundaries order anything.
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

__device__ __forceinline__ double load_d(const double* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(256) traverse_init_kernel(const TraverseC q) {
    const int64_t n_nodes = (int64_t)q.rows * q.cols;
    unsigned long long bad = 0;
    for (int64_t n = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; n < n_nodes; n += (int64_t)gridDim.x * blockDim.x) {
        q.d[n] = __builtin_huge_val();
        if (q.pen && !penalty_ok(q.pen[n])) bad++;
    }
    if (bad) atomicAdd(&q.visits[1], bad);
}

// one lane per source: its cost, and the 3 x 3 tiles around its own (a source on a tile's edge sits in its neighbours' halos)
__global__ void __launch_bounds__(64) traverse_seed_kernel(const TraverseC q) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= q.n_src) return;
    const int64_t n = q.src_node[s];
    q.d[n] = q.src_cost[s];
    const int ty = (int)(n / q.cols) / q.tile, tx = (int)(n % q.cols) / q.tile;
    for (int a = -1; a <= 1; a++)
        for (int b = -1; b <= 1; b++) {
            int y = ty + a, x = tx + b;
            if (y < 0 || y >= q.tiles_y) continue;
            if (x < 0 || x >= q.tiles_x) {
                if (!q.wrap) continue;
                x = x < 0 ? x + q.tiles_x : x - q.tiles_x;
            }
            __hip_atomic_store(&q.flag_in[(int64_t)y * q.tiles_x + x], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
}

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
            dv = load_d(&q.d[n]);
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
            const bool n_ = a == 0, s_ = a == th - 1, w_ = b == 0, e_ = b == tw - 1;
            mask |= (n_ ? 1u : 0u) | (n_ && e_ ? 2u : 0u) | (e_ ? 4u : 0u) | (s_ && e_ ? 8u : 0u) | (s_ ? 16u : 0u) |
                    (s_ && w_ ? 32u : 0u) | (w_ ? 64u : 0u) | (n_ && w_ ? 128u : 0u);
        }
    }
    if (mask) atomicOr(&s_mask, mask);
    const int any = __syncthreads_or(lowered ? 1 : 0);
    if (lane == 0 && any) {
        atomicAdd(&q.changed[q.slot], 1u);
        const uint32_t m = s_mask;
        for (int k = 0; k < 8; k++) {
            if (!(m & (1u << k))) continue;
            const int y = ty + kDi[k];
            int xx = tx + kDj[k];
            if (y < 0 || y >= q.tiles_y) continue;
            if (xx < 0 || xx >= q.tiles_x) {
                if (!q.wrap) continue;
                xx = xx < 0 ? xx + q.tiles_x : xx - q.tiles_x;
            }
            __hip_atomic_store(&q.flag_out[(int64_t)y * q.tiles_x + xx], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// one lane per node: 255 unreachable; else the first direction k whose neighbour u has d[u] < d[v], a driven edge and
// d[u] + w == d[v]; 254 if none (the sources get code 8 from traverse_source_pred_kernel afterwards)
__global__ void __launch_bounds__(256) traverse_pred_kernel(const TraverseC q) {
    const int64_t n_nodes = (int64_t)q.rows * q.cols;
    for (int64_t n = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; n < n_nodes; n += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = n / q.cols, j = n % q.cols;
        const double dv = q.d[n];
        uint8_t code = 255;
        if (dv != __builtin_huge_val()) {
            code = 254;
            const float Dv = node_D(q, i, j), Pv = q.pen ? q.pen[n] : 1.0f;
            for (int k = 0; k < 8; k++) {
                const int64_t ui = i + kDi[k];
                int64_t uj = j + kDj[k];
                if (!in_window(q, ui, uj)) continue;
                const int64_t u = ui * q.cols + uj;
                const double du = q.d[u];
                if (!(du < dv)) continue;
                const float w = edge_w(q, node_D(q, ui, uj), Dv, q.pen ? q.pen[u] : 1.0f, Pv, edge_len(q, i, kDi[k], kDj[k]));
                if (w != __builtin_huge_valf() && du + (double)w == dv) { code = (uint8_t)k; break; }
            }
        }
        q.pred[n] = code;
    }
}

__global__ void __launch_bounds__(64) traverse_source_pred_kernel(const TraverseC q) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= q.n_src) return;
    const int64_t n = q.src_node[s];
    if (q.d[n] == q.src_cost[s]) q.pred[n] = 8;
}

// one lane per node: its D, for the heights along a route (mrtx_traverse_heights)
__global__ void __launch_bounds__(256) traverse_heights_kernel(const TraverseC q, float* __restrict__ out) {
    const int64_t n_nodes = (int64_t)q.rows * q.cols;
    for (int64_t n = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; n < n_nodes; n += (int64_t)gridDim.x * blockDim.x)
        out[n] = node_D(q, n / q.cols, n % q.cols);
}

}  // namespace mrtx_tr

static unsigned traverse_grid(int64_t n, int per_block) {
    const int64_t b = (n + per_block - 1) / per_block;
    return (unsigned)(b < 1 ? 1 : b > 65536 ? 65536 : b);
}

// +inf costs, the device penalty check (into q.visits[1]), then the sources and their tiles (into q.flag_in)
hipError_t mrtx_launch_traverse_init(const TraverseC& q, hipStream_t st) {
    if (q.rows < 1 || q.cols < 1 || q.n_src < 1 || !q.d || !q.visits || !q.flag_in || !q.src_node || !q.src_cost)
        return hipErrorInvalidValue;
    const int64_t n = (int64_t)q.rows * q.cols;
    hipLaunchKernelGGL(mrtx_tr::traverse_init_kernel, dim3(traverse_grid(n, 256)), dim3(256), 0, st, q);
    hipLaunchKernelGGL(mrtx_tr::traverse_seed_kernel, dim3((unsigned)((q.n_src + 63) / 64)), dim3(64), 0, st, q);
    return hipGetLastError();
}

// one relaxation launch over every tile (the inactive ones return at once)
hipError_t mrtx_launch_traverse_relax(const TraverseC& q, hipStream_t st) {
    const int64_t tiles = (int64_t)q.tiles_x * q.tiles_y;
    if (tiles < 1 || tiles > 0xFFFFFFFFll || !q.flag_in || !q.flag_out || !q.changed || !q.d || !q.len) return hipErrorInvalidValue;
    const dim3 grid((unsigned)tiles), block(64);
    switch (q.tile) {
        case 8: hipLaunchKernelGGL(mrtx_tr::traverse_relax_kernel<8>, grid, block, 0, st, q); break;
        case 16: hipLaunchKernelGGL(mrtx_tr::traverse_relax_kernel<16>, grid, block, 0, st, q); break;
        case 32: hipLaunchKernelGGL(mrtx_tr::traverse_relax_kernel<32>, grid, block, 0, st, q); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t mrtx_launch_traverse_pred(const TraverseC& q, hipStream_t st) {
    if (q.rows < 1 || q.cols < 1 || !q.d || !q.pred || !q.len) return hipErrorInvalidValue;
    const int64_t n = (int64_t)q.rows * q.cols;
    hipLaunchKernelGGL(mrtx_tr::traverse_pred_kernel, dim3(traverse_grid(n, 256)), dim3(256), 0, st, q);
    hipLaunchKernelGGL(mrtx_tr::traverse_source_pred_kernel, dim3((unsigned)((q.n_src + 63) / 64)), dim3(64), 0, st, q);
    return hipGetLastError();
}

hipError_t mrtx_launch_traverse_heights(const TraverseC& q, float* out, hipStream_t st) {
    if (q.rows < 1 || q.cols < 1 || !q.dem || !out) return hipErrorInvalidValue;
    const int64_t n = (int64_t)q.rows * q.cols;
    hipLaunchKernelGGL(mrtx_tr::traverse_heights_kernel, dim3(traverse_grid(n, 256)), dim3(256), 0, st, q, out);
    return hipGetLastError();
}
