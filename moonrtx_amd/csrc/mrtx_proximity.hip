// mrtx_proximity.hip -- gfx950 kernels of the proximity maps and the reach of labelled regions (mrtx_proximity,
// mrtx_regions_reach; DESIGN.md sections 3.22, 4.28).
//
// Every node's nearest feature by the exact squared distance of int32 positions, ties to the least node index.  The lattice is
// cut into tiles of 8 x 8 nodes, one wave (one workgroup) per tile, one node per lane:
//   prox_tiles_kernel       per tile: the features compacted into the tile's list in the order of their lanes, the bounding box
//                           of their positions and their number; every coordinate checked against +-2^29 and clamped to it, so
//                           that no difference leaves 31 bits whatever the caller's table holds
//   prox_scan_kernel<PRUNE> per tile of query nodes: the pair loop.  A feature tile's list is copied into LDS and every lane
//                           walks it: three 32 x 32 -> 64-bit multiply-adds and a two-word compare on (d2, index) per pair.
//                           Without PRUNE every tile that has features is walked (MOONRT_PROXIMITY=brute).  With PRUNE the
//                           wave first finds U, the least over the feature tiles of the greatest box-to-box distance, walks the
//                           tile that attains it, and then walks in ascending order the tiles whose least box-to-box distance
//                           is <= U; after every walked tile U falls to the greatest d2 any of the wave's nodes holds.  A tile
//                           is skipped only when its lower bound is strictly greater than U, so a feature at an equal distance
//                           and a lower index is never lost.
//   reach_*_kernel          per region the greatest and least dist2 (64-bit atomics, waves of one label reduced first), then
//                           the least node index attaining each, then nearest[min_at]
// All bounds are integers and no result depends on the order of evaluation.  No kernel waits on another workgroup.  Own
// translation unit: the existing kernels are compiled exactly as before.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mrtx_proximity.h"
#include "mrtx_lattice_dev.h"

namespace mrtx_px {

typedef unsigned long long u64;
using namespace mrtx_lat;       // label_ok, value_now, check_labels

constexpr int TW = MRTX_PX_TW;
constexpr int TILE = MRTX_PX_TILE;
constexpr int32_t CMAX = MRTX_PX_CMAX;
static_assert(TW * TW == TILE && TILE == 64, "one node per lane of a wave");

__device__ __forceinline__ int32_t clampc(int32_t c) { return c < -CMAX ? -CMAX : c > CMAX ? CMAX : c; }

__device__ __forceinline__ int32_t wave_min(int32_t v) {
    for (int d = 32; d >= 1; d >>= 1) { const int32_t o = __shfl_xor(v, d); v = o < v ? o : v; }
    return v;
}
__device__ __forceinline__ int32_t wave_max(int32_t v) {
    for (int d = 32; d >= 1; d >>= 1) { const int32_t o = __shfl_xor(v, d); v = o > v ? o : v; }
    return v;
}
__device__ __forceinline__ u64 wave_max(u64 v) {
    for (int d = 32; d >= 1; d >>= 1) { const u64 o = __shfl_xor(v, d); v = o > v ? o : v; }
    return v;
}
__device__ __forceinline__ u64 wave_min(u64 v) {
    for (int d = 32; d >= 1; d >>= 1) { const u64 o = __shfl_xor(v, d); v = o < v ? o : v; }
    return v;
}
// a value every lane holds alike, in scalar registers
__device__ __forceinline__ u64 uniform(u64 v) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return (u64)hi << 32 | lo;
}

__device__ __forceinline__ u64 sq(int64_t d) { return (u64)(d * d); }      // |d| <= 2^30

// the greatest and the least squared distance between a point of the box [qlo, qhi] and one of the box b, both non-empty
__device__ __forceinline__ u64 box_far(const int32_t* qlo, const int32_t* qhi, const ProxBox& b) {
    u64 s = 0;
    for (int k = 0; k < 3; k++) {
        const int64_t a = (int64_t)b.hi[k] - qlo[k], c = (int64_t)qhi[k] - b.lo[k];
        s += sq(a > c ? a : c);
    }
    return s;
}
__device__ __forceinline__ u64 box_near(const int32_t* qlo, const int32_t* qhi, const ProxBox& b) {
    u64 s = 0;
    for (int k = 0; k < 3; k++) {
        const int64_t a = (int64_t)b.lo[k] - qhi[k], c = (int64_t)qlo[k] - b.hi[k];
        const int64_t g = a > c ? a : c;
        s += sq(g > 0 ? g : 0);
    }
    return s;
}

// the node of lane `lane` of tile t, or false past the lattice's edge
__device__ __forceinline__ bool tile_node(const ProxC& q, int64_t t, int lane, int64_t* v) {
    const int32_t i = (int32_t)(t / q.tiles_x) * TW + (lane >> 3), j = (int32_t)(t % q.tiles_x) * TW + (lane & (TW - 1));
    *v = (int64_t)i * q.cols + j;
    return i < q.rows && j < q.cols;
}

__global__ void __launch_bounds__(64) prox_tiles_kernel(const ProxC q) {
    const int lane = threadIdx.x;
    const int64_t t = blockIdx.x;
    int64_t v;
    const bool valid = tile_node(q, t, lane, &v);
    int32_t p[3] = {0, 0, 0};
    bool isf = false;
    uint32_t nbad = 0;
    if (valid) {
        for (int k = 0; k < 3; k++) {
            const int32_t c = q.pos[3 * v + k];
            p[k] = clampc(c);
            nbad += p[k] != c;
        }
        const int32_t l = q.labels[v];
        isf = q.outside ? l < 0 : l >= 0;
    }
    if (nbad) atomicAdd(q.bad, nbad);
    const u64 m = __ballot(isf);
    if (isf) {
        ProxFeat f;
        f.x = p[0]; f.y = p[1]; f.z = p[2]; f.v = (int32_t)v;
        q.feat[t * TILE + __popcll(m & ((1ull << lane) - 1ull))] = f;
    }
    ProxBox b;
    for (int k = 0; k < 3; k++) {
        b.lo[k] = wave_min(isf ? p[k] : INT32_MAX);
        b.hi[k] = wave_max(isf ? p[k] : INT32_MIN);
    }
    b.n = __popcll(m);
    b.pad = 0;
    if (lane == 0) q.box[t] = b;
}

template <bool PRUNE>
__global__ void __launch_bounds__(64) prox_scan_kernel(const ProxC q) {
    __shared__ ProxFeat sf[TILE];
    const int lane = threadIdx.x;
    const int64_t t = blockIdx.x, T = (int64_t)q.tiles_x * q.tiles_y;
    int64_t v;
    const bool valid = tile_node(q, t, lane, &v);
    int32_t px = 0, py = 0, pz = 0;
    if (valid) { px = clampc(q.pos[3 * v]); py = clampc(q.pos[3 * v + 1]); pz = clampc(q.pos[3 * v + 2]); }
    const u64 nq = (u64)__popcll(__ballot(valid));          // lane 0 is always a node
    u64 best = ~0ull, npairs = 0;
    int32_t at = -1;

    // the pair loop over the list of feature tile ft: the same trip count in every lane
    auto walk = [&](int64_t ft) {
        const int n = q.box[ft].n;
        __syncthreads();                                    // the last walk has read sf
        if (lane < n) sf[lane] = q.feat[ft * TILE + lane];
        __syncthreads();
        for (int k = 0; k < n; k++) {
            const ProxFeat f = sf[k];
            const int32_t dx = px - f.x, dy = py - f.y, dz = pz - f.z;
            const u64 d2 = (u64)((int64_t)dx * dx + (int64_t)dy * dy + (int64_t)dz * dz);
            if (d2 < best || (d2 == best && f.v < at)) { best = d2; at = f.v; }
        }
        npairs += (u64)n * nq;
    };

    int32_t qlo[3], qhi[3];
    u64 U = ~0ull;          // every node of the tile has a feature at d2 <= U
    int64_t first = -1;
    if (PRUNE) {
        const int32_t pp[3] = {px, py, pz};
        for (int k = 0; k < 3; k++) {
            qlo[k] = wave_min(valid ? pp[k] : INT32_MAX);
            qhi[k] = wave_max(valid ? pp[k] : INT32_MIN);
        }
        u64 u = ~0ull;
        int64_t ut = T;
        for (int64_t f0 = 0; f0 < T; f0 += 64) {
            const int64_t f = f0 + lane;
            if (f < T) {
                const ProxBox b = q.box[f];
                if (b.n > 0) {
                    const u64 d = box_far(qlo, qhi, b);
                    if (d < u) { u = d; ut = f; }           // a lane's tiles ascend: the first of equals stays
                }
            }
        }
        for (int d = 32; d >= 1; d >>= 1) {
            const u64 ou = __shfl_xor(u, d);
            const int64_t ot = __shfl_xor(ut, d);
            if (ou < u || (ou == u && ot < ut)) { u = ou; ut = ot; }
        }
        U = uniform(u);
        if (U != ~0ull) {
            first = (int64_t)uniform((u64)ut);
            walk(first);
            const u64 w = uniform(wave_max(valid ? best : 0ull));
            U = w < U ? w : U;
        }
    }
    if (!PRUNE || first >= 0) {
        for (int64_t f0 = 0; f0 < T; f0 += 64) {
            const int64_t f = f0 + lane;
            bool take = false;
            u64 near = 0;
            if (f < T) {
                const ProxBox b = q.box[f];
                take = b.n > 0;
                if (PRUNE && take) {
                    near = box_near(qlo, qhi, b);
                    take = f != first && near <= U;
                }
            }
            for (u64 m = __ballot(take); m; m &= m - 1ull) {
                const int k = __ffsll((long long)m) - 1;
                if (PRUNE) {
                    if (uniform(__shfl(near, k)) > U) continue;     // U has fallen since the ballot
                    walk(f0 + k);
                    const u64 w = uniform(wave_max(valid ? best : 0ull));
                    U = w < U ? w : U;
                } else {
                    walk(f0 + k);
                }
            }
        }
    }
    if (valid) {
        q.nearest[v] = at;
        q.dist2[v] = best;
    }
    if (lane == 0 && npairs) atomicAdd(q.pairs, npairs);
}

// ---- the reach of labelled regions
__global__ void __launch_bounds__(256) check_kernel(const int32_t* labels, int64_t N, uint32_t n_regions, uint32_t* out) {
    check_labels(labels, N, n_regions, out);
}

__global__ void __launch_bounds__(256) reach_init_kernel(const ReachC q) {
    for (uint32_t r = blockIdx.x * 256u + threadIdx.x; r < q.n_regions; r += gridDim.x * 256u) {
        ReachRec z;
        z.d2_max = 0; z.d2_min = ~0ull; z.max_at = INT32_MAX; z.min_at = INT32_MAX; z.min_nearest = -1; z.count = 0;
        q.out[r] = z;
    }
}

// A maximum only ever rises and a minimum only ever falls, so a read of either, however old, is no further out than the entry:
// an atomic that would not move what was read cannot move the entry either and is left out.
__device__ __forceinline__ void reach_add(ReachRec* o, u64 hi, u64 lo, uint32_t count) {
    atomicAdd(&o->count, count);
    if (hi > value_now(&o->d2_max)) atomicMax(&o->d2_max, hi);
    if (lo < value_now(&o->d2_min)) atomicMin(&o->d2_min, lo);
}

// every wave takes 64 consecutive nodes at a time; when they all carry one label they are reduced in the wave first
__global__ void __launch_bounds__(256) reach_extent_kernel(const ReachC q) {
    const int64_t N = (int64_t)q.rows * q.cols;
    const int lane = threadIdx.x & 63;
    for (int64_t n0 = blockIdx.x * (int64_t)256 + (threadIdx.x & ~63); n0 < N; n0 += (int64_t)gridDim.x * 256) {
        const int64_t n = n0 + lane;
        int32_t l = n < N ? q.labels[n] : -1;
        if (!label_ok(q.n_regions, l)) l = -1;
        const u64 d = l >= 0 ? q.dist2[n] : 0ull;
        if (__all(l == __shfl(l, 0))) {                     // the trip count is the wave's: every lane is here
            if (l < 0) continue;
            const u64 hi = wave_max(d), lo = wave_min(d);
            if (lane == 0) reach_add(q.out + l, hi, lo, 64u);
        } else if (l >= 0) {
            reach_add(q.out + l, d, d, 1u);
        }
    }
}

// the least node index that attains each extreme, which the launch before has settled
__global__ void __launch_bounds__(256) reach_place_kernel(const ReachC q) {
    const int64_t N = (int64_t)q.rows * q.cols;
    for (int64_t n = blockIdx.x * (int64_t)256 + threadIdx.x; n < N; n += (int64_t)gridDim.x * 256) {
        const int32_t l = q.labels[n];
        if (!label_ok(q.n_regions, l)) continue;
        ReachRec* o = q.out + l;
        const u64 d = q.dist2[n];
        if (d == o->d2_max && (int32_t)n < value_now(&o->max_at)) atomicMin(&o->max_at, (int32_t)n);
        if (d == o->d2_min && (int32_t)n < value_now(&o->min_at)) atomicMin(&o->min_at, (int32_t)n);
    }
}

__global__ void __launch_bounds__(256) reach_finish_kernel(const ReachC q) {
    for (uint32_t r = blockIdx.x * 256u + threadIdx.x; r < q.n_regions; r += gridDim.x * 256u) {
        ReachRec* o = q.out + r;
        if (o->count) {
            o->min_nearest = q.nearest[o->min_at];
        } else {
            o->max_at = -1; o->min_at = -1; o->min_nearest = -1;
        }
    }
}

}  // namespace mrtx_px

static unsigned reach_grid(int64_t n) {
    const int64_t b = (n + 255) / 256;
    return (unsigned)(b < 1 ? 1 : b > 65536 ? 65536 : b);
}

// prune: skip the feature tiles whose integer lower bound exceeds the tile's proven upper bound.  Two launches whatever the
// data; one workgroup per tile, so at most 2^31 / 64 of them.
hipError_t mrtx_launch_proximity(const ProxC& q, bool prune, hipStream_t st, uint32_t* launches) {
    if (q.rows < 1 || q.cols < 1 || !q.pos || !q.labels || !q.nearest || !q.dist2 || !q.box || !q.feat || !q.pairs || !q.bad)
        return hipErrorInvalidValue;
    const ProxLayout at = prox_layout(q.rows, q.cols, false, false);
    if (q.tiles_x != at.tiles_x || q.tiles_y != at.tiles_y) return hipErrorInvalidValue;
    const int64_t T = (int64_t)q.tiles_x * q.tiles_y;
    if (T > 0x7FFFFFFFll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mrtx_px::prox_tiles_kernel, dim3((unsigned)T), dim3(64), 0, st, q);
    if (prune) hipLaunchKernelGGL(mrtx_px::prox_scan_kernel<true>, dim3((unsigned)T), dim3(64), 0, st, q);
    else hipLaunchKernelGGL(mrtx_px::prox_scan_kernel<false>, dim3((unsigned)T), dim3(64), 0, st, q);
    if (launches) *launches = 2;
    return hipGetLastError();
}

// Without regions only the check of the table runs.
hipError_t mrtx_launch_regions_reach(const ReachC& q, hipStream_t st, uint32_t* launches) {
    if (q.rows < 1 || q.cols < 1 || !q.labels || !q.bad || (q.n_regions && (!q.out || !q.dist2 || !q.nearest)))
        return hipErrorInvalidValue;
    const int64_t N = (int64_t)q.rows * q.cols;
    const unsigned gn = reach_grid(N), gr = reach_grid(q.n_regions);
    hipLaunchKernelGGL(mrtx_px::check_kernel, dim3(gn), dim3(256), 0, st, q.labels, N, q.n_regions, q.bad);
    if (q.n_regions) {
        hipLaunchKernelGGL(mrtx_px::reach_init_kernel, dim3(gr), dim3(256), 0, st, q);
        hipLaunchKernelGGL(mrtx_px::reach_extent_kernel, dim3(gn), dim3(256), 0, st, q);
        hipLaunchKernelGGL(mrtx_px::reach_place_kernel, dim3(gn), dim3(256), 0, st, q);
        hipLaunchKernelGGL(mrtx_px::reach_finish_kernel, dim3(gr), dim3(256), 0, st, q);
    }
    if (launches) *launches = q.n_regions ? 5 : 1;
    return hipGetLastError();
}
