// mrtx_fill.hip -- gfx950 kernels of the terrain depressions: mrtx_fill and mrtx_fill_basins (DESIGN.md sections 3.24, 4.30).
//
// The fill W over a lattice of int32 heights z is the least fixed point of W[v] = min(src[v], max(z[v], min_u W[u])), src = z at
// the outlets and INT32_MAX elsewhere, u the neighbours of v: the minimax path value to the nearest outlet.  Every step only
// lowers an int32 and the value is defined by paths alone, so no byte depends on the order of the relaxations.
//   fill_init_kernel       W = src, the heights beyond the bound counted, the tiles that hold or touch an outlet flagged
//   fill_relax_kernel<TS>  traverse_relax_kernel's scheme (mrtx_traverse.hip) over (min, max) in int32: one 64-lane workgroup per
//                          flagged tile, W and z of the tile and its one-node halo in LDS, directional sweeps (lanes 0-31 down
//                          then right, lanes 32-63 up then left) with LDS atomicMin until a round lowers nothing; the lowered
//                          nodes written back, the neighbour tiles whose shared edge or corner changed flagged for the next launch
//   fill_sweep_kernel      MOONRT_FILL=sweep, the yardstick: one Jacobi step over the whole lattice from one table into another
//   basins_init_kernel, basins_sum_kernel, basins_finish_kernel
//                          the catalogue of a label table over a fill: one pass with per-region integer atomics, the pour point and
//                          the deepest node as packed 64-bit keys under atomicMin / atomicMax; every label bound-checked; the
//                          lanes of a wave that carry one label are summed in the wave first
// Memory rule as in mrtx_traverse.hip: correctness never depends on seeing, within a launch, what another workgroup of that
// launch wrote.  The halo loads and the stores of W that another workgroup may read in the same launch are relaxed agent-scope
// atomics; a stale read only costs another launch.  Only kernel boundaries order anything.
// A height beyond +-MRTX_FILL_ZMAX is clamped wherever it is read, so a bad device table cannot make a depth overflow.
// Own translation unit: the existing kernels are compiled exactly as before.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mrtx_fill.h"
#include "mrtx_lattice_dev.h"

namespace mrtx_fl {

typedef unsigned long long u64;
using namespace mrtx_lat;       // label_ok, xor64

constexpr int32_t kNone = 0x7FFFFFFF;                             // MRTX_FILL_NONE: no outlet reached (yet)

__device__ constexpr int kDi[8] = {-1, -1, 0, 1, 1, 1, 0, -1};   // N, NE, E, SE, S, SW, W, NW
__device__ constexpr int kDj[8] = {0, 1, 1, 1, 0, -1, -1, -1};

__device__ __forceinline__ int32_t clamp_z(int32_t z) { return z < -MRTX_FILL_ZMAX ? -MRTX_FILL_ZMAX : z > MRTX_FILL_ZMAX ? MRTX_FILL_ZMAX : z; }

// Is node (i, j) in the lattice?  j is wrapped into [0, cols) when the lattice wraps.
__device__ __forceinline__ bool in_lattice(int rows, int cols, int wrap, int64_t i, int64_t& j) {
    if (i < 0 || i >= rows) return false;
    if (j < 0 || j >= cols) {
        if (!wrap) return false;
        j = j < 0 ? j + cols : j - cols;
    }
    return true;
}

__device__ __forceinline__ bool is_outlet(const FillC& q, int64_t i, int64_t j, int64_t n) {
    if (q.edge_outlets && (i == 0 || i == q.rows - 1 || (!q.wrap && (j == 0 || j == q.cols - 1)))) return true;
    return q.outlet && q.outlet[n] != 0;
}

// Flag tile (y, x) for a relaxation launch; x wraps with the lattice, a tile outside the grid is none
__device__ __forceinline__ void flag_tile(const FillC& c, uint32_t* flags, int y, int x) {
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

// one lane per node: W = z at the outlets, kNone elsewhere.  TILES: an outlet flags its tile and the tiles that hold it in
// their halo.
template <bool TILES>
__global__ void __launch_bounds__(256) fill_init_kernel(const FillC q) {
    constexpr int TS = MRTX_FILL_TS;
    const int64_t N = (int64_t)q.rows * q.cols;
    uint32_t bad = 0;
    for (int64_t n = blockIdx.x * (int64_t)256 + threadIdx.x; n < N; n += (int64_t)gridDim.x * 256) {
        const int64_t i = n / q.cols, j = n % q.cols;
        const int32_t z = q.z[n];
        bad += z < -MRTX_FILL_ZMAX || z > MRTX_FILL_ZMAX;
        const bool o = is_outlet(q, i, j, n);
        q.w[n] = o ? clamp_z(z) : kNone;
        if (TILES && o) {
            const int ty = (int)(i / TS), tx = (int)(j / TS);
            const int th = (int)min((int64_t)TS, q.rows - (int64_t)ty * TS), tw = (int)min((int64_t)TS, q.cols - (int64_t)tx * TS);
            flag_tile(q, q.flag_in, ty, tx);
            const uint32_t m = halo_mask((int)(i - (int64_t)ty * TS), (int)(j - (int64_t)tx * TS), th, tw);
            for (int k = 0; k < 8; k++)
                if (m & (1u << k)) flag_tile(q, q.flag_in, ty + kDi[k], tx + kDj[k]);
        }
    }
    if (bad) atomicAdd(q.bad, bad);
}

template <int TS>
__global__ void __launch_bounds__(64) fill_relax_kernel(const FillC q) {
    static_assert(TS == 32, "the sweeps give each half of the wave one row or column of the tile");
    constexpr int P = TS + 3;       // pitch of the staged W and z, the tile and its halo (odd: a column's lanes hit distinct banks)
    __shared__ int32_t sW[(TS + 2) * P];
    __shared__ int32_t sz[(TS + 2) * P];
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

    // stage W and z of the tile and its halo (the halo's far row / column right after the tile's last one); what lies outside
    // the lattice is kNone, which no max() lowers
    for (int p = lane; p < (th + 2) * (tw + 2); p += 64) {
        const int a = p / (tw + 2) - 1, b = p % (tw + 2) - 1;
        const int64_t gi = i0 + a;
        int64_t gj = j0 + b;
        int32_t wv = kNone, zv = 0;
        if (in_lattice(q.rows, q.cols, q.wrap, gi, gj)) {
            const int64_t n = gi * q.cols + gj;
            wv = __hip_atomic_load(&q.w[n], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            zv = clamp_z(q.z[n]);
        }
        sW[(a + 1) * P + (b + 1)] = wv;
        sz[(a + 1) * P + (b + 1)] = zv;
    }
    __syncthreads();

    // sweeps: lanes 0-31 run down (from row a - 1) then right (from column b - 1), lanes 32-63 at the same time up then left;
    // with connectivity 8 each also takes the two diagonal neighbours of that row or column.  A lowered W is an LDS atomic
    // min, so the two halves never lose each other's update where they meet.
    const int half = lane >> 5, x = lane & 31;
    const bool c8 = q.conn8 != 0;
    for (;;) {
        int ch = 0;
        for (int s = 0; s < th; s++) {
            if (x < tw) {
                const int a = half ? th - 1 - s : s, da = half ? 1 : -1;
                int32_t* v = &sW[(a + 1) * P + (x + 1)];
                const int32_t* u = &sW[(a + 1 + da) * P + (x + 1)];
                int32_t m = u[0];
                if (c8) m = min(m, min(u[-1], u[1]));
                const int32_t c = max(sz[(a + 1) * P + (x + 1)], m);
                if (c < *v) {
                    atomicMin(v, c);
                    ch = 1;
                }
            }
            __syncthreads();
        }
        for (int s = 0; s < tw; s++) {
            if (x < th) {
                const int b = half ? tw - 1 - s : s, db = half ? 1 : -1;
                int32_t* v = &sW[(x + 1) * P + (b + 1)];
                const int32_t* u = v + db;
                int32_t m = u[0];
                if (c8) m = min(m, min(u[-P], u[P]));
                const int32_t c = max(sz[(x + 1) * P + (b + 1)], m);
                if (c < *v) {
                    atomicMin(v, c);
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
        const int32_t nv = sW[(a + 1) * P + (b + 1)];
        if (nv < q.w[n]) {                   // only this workgroup writes its own nodes
            __hip_atomic_store(&q.w[n], nv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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

// one Jacobi step, one lane per node: w[v] = min(w_in[v], max(z[v], min_u w_in[u])).  w_in is not written in this launch.
__global__ void __launch_bounds__(256) fill_sweep_kernel(const FillC q) {
    const int64_t N = (int64_t)q.rows * q.cols;
    const int step = q.conn8 ? 1 : 2;
    uint32_t updates = 0;
    for (int64_t n = blockIdx.x * (int64_t)256 + threadIdx.x; n < N; n += (int64_t)gridDim.x * 256) {
        const int64_t i = n / q.cols, j = n % q.cols;
        const int32_t wv = q.w_in[n];
        int32_t m = kNone;
        for (int k = 0; k < 8; k += step) {
            int64_t uj = j + kDj[k];
            if (in_lattice(q.rows, q.cols, q.wrap, i + kDi[k], uj)) m = min(m, q.w_in[(i + kDi[k]) * q.cols + uj]);
        }
        const int32_t c = max(clamp_z(q.z[n]), m);
        q.w[n] = c < wv ? c : wv;
        updates += c < wv;
    }
    if (updates) {
        atomicAdd(&q.visits[0], (u64)updates);
        atomicAdd(&q.changed[q.slot], 1u);
    }
}

// ---- the catalogue
__global__ void __launch_bounds__(256) basins_init_kernel(const BasinC q) {
    for (uint32_t r = blockIdx.x * 256u + threadIdx.x; r < q.n_regions; r += gridDim.x * 256u) {
        BasinRec e;
        e.weight = 0; e.volume = 0; e.count = 0; e.level_min = 0x7FFFFFFF; e.level_max = (int32_t)0x80000000; e.depth_max = 0;
        e.deepest_at = -1; e.pour_at = -1; e.pour_level = 0x7FFFFFFF; e.reserved = 0;
        q.out[r] = e;
        q.keys[2 * (size_t)r] = ~0ull;
        q.keys[2 * (size_t)r + 1] = 0ull;
    }
}

// what the nodes of one region add to its record
struct BasinSum {
    u64 weight, volume, deep;
    uint32_t count;
    int32_t fmin, fmax;
    static __device__ __forceinline__ BasinSum none() {
        BasinSum v;
        v.weight = 0; v.volume = 0; v.deep = 0; v.count = 0; v.fmin = 0x7FFFFFFF; v.fmax = (int32_t)0x80000000;
        return v;
    }
};

// the sum over the wave's 64 lanes, in every lane (a lane that takes no part passes none())
__device__ __forceinline__ BasinSum wave_sum(BasinSum v) {
    for (int m = 1; m < 64; m <<= 1) {
        const u64 deep = xor64(v.deep, m);
        const int32_t fmin = __shfl_xor(v.fmin, m), fmax = __shfl_xor(v.fmax, m);
        v.weight += xor64(v.weight, m);
        v.volume += xor64(v.volume, m);
        v.count += __shfl_xor(v.count, m);
        v.deep = deep > v.deep ? deep : v.deep;
        v.fmin = fmin < v.fmin ? fmin : v.fmin;
        v.fmax = fmax > v.fmax ? fmax : v.fmax;
    }
    return v;
}

__device__ __forceinline__ void basin_add(const BasinC& q, int32_t l, const BasinSum& v) {
    BasinRec* e = &q.out[l];
    atomicAdd(&e->weight, v.weight);
    atomicAdd(&e->volume, v.volume);
    atomicAdd(&e->count, v.count);
    atomicMin(&e->level_min, v.fmin);
    atomicMax(&e->level_max, v.fmax);
    atomicMax(&q.keys[2 * (size_t)l + 1], v.deep);
}

// distinct labels a wave sums in its lanes before the lanes that are left add on their own
constexpr int kPeel = 4;

// A wave takes 64 consecutive nodes at a time, one lane per node v: its own region's sums and extremes, and its bid (fill[v], v)
// for the pour point of every other region that a neighbour of v carries.  The lanes that carry the label of the first open lane
// are summed in the wave and that lane alone issues the atomics, kPeel times over; every sum is an integer sum or an extreme,
// so the records do not depend on which lanes were summed together.
__global__ void __launch_bounds__(256) basins_sum_kernel(const BasinC q) {
    const int64_t N = (int64_t)q.rows * q.cols;
    const int step = q.conn8 ? 1 : 2;
    const int lane = threadIdx.x & 63;
    uint32_t bad_l = 0, bad_z = 0;
    // wave-uniform trip count: the lanes past the last node take part in the wave's sums with nothing
    for (int64_t base = blockIdx.x * (int64_t)256 + (threadIdx.x & ~63); base < N; base += (int64_t)gridDim.x * 256) {
        const int64_t n = base + lane;
        const bool in = n < N;
        const int64_t i = in ? n / q.cols : 0, j = in ? n % q.cols : 0;
        const int32_t l = in ? q.labels[n] : -1, zr = in ? q.z[n] : 0, f = in ? q.fill[n] : 0;
        bad_l += l < -1 || (l >= 0 && (uint32_t)l >= q.n_regions);
        bad_z += zr < -MRTX_FILL_ZMAX || zr > MRTX_FILL_ZMAX;
        bool open = in && label_ok(q.n_regions, l);
        BasinSum v = BasinSum::none();
        if (open) {
            // the depth of any fill table: (int64)fill - z held in 0 .. INT32_MAX
            long long d = (long long)f - (long long)clamp_z(zr);
            d = d < 0 ? 0 : d > 0x7FFFFFFFll ? 0x7FFFFFFFll : d;
            v.weight = q.row_weight ? (u64)q.row_weight[i] : 1ull;
            v.volume = v.weight * (u64)d;
            v.deep = ((u64)d << 32) | (u64)(uint32_t)~(uint32_t)n;
            v.count = 1u;
            v.fmin = v.fmax = f;
        }
        u64 pending = __ballot(open);
        for (int r = 0; r < kPeel && pending; r++) {
            const int lead = __ffsll((long long)pending) - 1;
            const int32_t ll = __shfl(l, lead);
            const bool mine = open && l == ll;
            const BasinSum s = wave_sum(mine ? v : BasinSum::none());
            if (lane == lead) basin_add(q, ll, s);
            if (mine) open = false;
            pending = __ballot(open);
        }
        if (open) basin_add(q, l, v);
        if (!in) continue;
        const u64 bid = ((u64)((uint32_t)f ^ 0x80000000u) << 32) | (u64)(uint32_t)n;
        int32_t seen = l;
        for (int k = 0; k < 8; k += step) {
            int64_t uj = j + kDj[k];
            if (!in_lattice(q.rows, q.cols, q.wrap, i + kDi[k], uj)) continue;
            const int32_t lu = q.labels[(i + kDi[k]) * q.cols + uj];
            if (lu == l || lu == seen || !label_ok(q.n_regions, lu)) continue;
            seen = lu;
            u64* key = &q.keys[2 * (size_t)lu];
            if (bid < __hip_atomic_load(key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(key, bid);
        }
    }
    if (bad_l) atomicAdd(&q.bad[0], bad_l);
    if (bad_z) atomicAdd(&q.bad[1], bad_z);
}

__global__ void __launch_bounds__(256) basins_finish_kernel(const BasinC q) {
    for (uint32_t r = blockIdx.x * 256u + threadIdx.x; r < q.n_regions; r += gridDim.x * 256u) {
        const u64 pour = q.keys[2 * (size_t)r], deep = q.keys[2 * (size_t)r + 1];
        BasinRec* e = &q.out[r];
        if (pour != ~0ull) {
            e->pour_at = (int32_t)(uint32_t)pour;
            e->pour_level = (int32_t)((uint32_t)(pour >> 32) ^ 0x80000000u);
        }
        if (deep != 0ull) {
            e->depth_max = (int32_t)(uint32_t)(deep >> 32);
            e->deepest_at = (int32_t)~(uint32_t)deep;
        }
    }
}

}  // namespace mrtx_fl

static unsigned fill_grid(int64_t n, int per_block) {
    const int64_t b = (n + per_block - 1) / per_block;
    return (unsigned)(b < 1 ? 1 : b > 65536 ? 65536 : b);
}

static bool fill_block_ok(const FillC& q) {
    return q.rows >= 1 && q.cols >= 1 && (int64_t)q.rows * q.cols <= ((int64_t)1 << 31) && q.z && q.w && q.visits && q.bad && q.changed;
}

hipError_t mrtx_launch_fill_init(const FillC& q, bool tiles, hipStream_t st) {
    if (!fill_block_ok(q) || (tiles && (!q.flag_in || q.tiles_x != (q.cols + MRTX_FILL_TS - 1) / MRTX_FILL_TS ||
                                        q.tiles_y != (q.rows + MRTX_FILL_TS - 1) / MRTX_FILL_TS)))
        return hipErrorInvalidValue;
    const dim3 grid(fill_grid((int64_t)q.rows * q.cols, 256)), block(256);
    if (tiles) hipLaunchKernelGGL(mrtx_fl::fill_init_kernel<true>, grid, block, 0, st, q);
    else hipLaunchKernelGGL(mrtx_fl::fill_init_kernel<false>, grid, block, 0, st, q);
    return hipGetLastError();
}

// one relaxation launch over every tile (the inactive ones return at once)
hipError_t mrtx_launch_fill_relax(const FillC& q, hipStream_t st) {
    const int64_t tiles = (int64_t)q.tiles_x * q.tiles_y;
    if (!fill_block_ok(q) || !q.flag_in || !q.flag_out || q.slot < 0 || q.slot >= MRTX_FILL_BATCH ||
        q.tiles_x != (q.cols + MRTX_FILL_TS - 1) / MRTX_FILL_TS || q.tiles_y != (q.rows + MRTX_FILL_TS - 1) / MRTX_FILL_TS ||
        tiles > 0x7FFFFFFFll)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(mrtx_fl::fill_relax_kernel<MRTX_FILL_TS>, dim3((unsigned)tiles), dim3(64), 0, st, q);
    return hipGetLastError();
}

hipError_t mrtx_launch_fill_sweep(const FillC& q, hipStream_t st) {
    if (!fill_block_ok(q) || !q.w_in || q.w_in == q.w || q.slot < 0 || q.slot >= MRTX_FILL_BATCH) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mrtx_fl::fill_sweep_kernel, dim3(fill_grid((int64_t)q.rows * q.cols, 256)), dim3(256), 0, st, q);
    return hipGetLastError();
}

hipError_t mrtx_launch_fill_basins(const BasinC& q, hipStream_t st, uint32_t* launches) {
    if (q.rows < 1 || q.cols < 1 || (int64_t)q.rows * q.cols > ((int64_t)1 << 31) || !q.labels || !q.z || !q.fill || !q.bad ||
        (q.n_regions && (!q.out || !q.keys)))
        return hipErrorInvalidValue;
    const dim3 block(256);
    if (q.n_regions) hipLaunchKernelGGL(mrtx_fl::basins_init_kernel, dim3(fill_grid(q.n_regions, 256)), block, 0, st, q);
    hipLaunchKernelGGL(mrtx_fl::basins_sum_kernel, dim3(fill_grid((int64_t)q.rows * q.cols, 256)), block, 0, st, q);
    if (q.n_regions) hipLaunchKernelGGL(mrtx_fl::basins_finish_kernel, dim3(fill_grid(q.n_regions, 256)), block, 0, st, q);
    if (launches) *launches = q.n_regions ? 3u : 1u;
    return hipGetLastError();
}
