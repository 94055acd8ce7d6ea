// mrtx_bowls.hip -- gfx950 kernels of the depression hierarchy: mrtx_bowls (DESIGN.md sections 3.25, 4.31).
//
// The hierarchy is the sublevel-set merge tree of the lattice under the keys (z, v).  The device does everything that is
// proportional to the number of nodes; the host sorts and walks only the minima and the edges of a spanning forest over them.
//   bowls_init_kernel      one lane per node: the steepest-descent pointer by key (an outlet points at the outside, N), the
//                          minima counted, the heights beyond the bound counted
//   bowls_jump_kernel      pointer jumping in place, a few hops per launch, until a launch moves nothing: ptr = the catchment
//   bowls_list_kernel      the packed keys of the minima, appended wave by wave
//   bowls_reset_kernel, bowls_bid_kernel, bowls_tie_kernel, bowls_hook_kernel, bowls_link_kernel, bowls_flatten_kernel
//                          one Boruvka round over the catchments and the outside: every lattice edge (u, v), key(u) < key(v),
//                          whose ends lie in different components bids key(v) for both (a plain load first, a 64-bit atomicMin
//                          only where it can win); among the edges with the winning key the least u wins, so the order of the
//                          edges is strict and the hooks form no cycle but the mutual pair, of which the lesser id stays a root;
//                          each hook appends its edge with the catchments of its two ends; then the parents are flattened
//   bowls_leaf_kernel, bowls_label_kernel
//                          the label of a node: up the parent chain from the leaf of its catchment to the first bowl that
//                          spills above the node's key; the nodes, weights and sums of w z of a label are summed over the lanes
//                          of a wave that carry it before the atomics
// Memory rule as in mrtx_fill.hip: no result depends on seeing, within a launch, what another workgroup of that launch wrote.
// The jumps and the flattening read and write one table in place with relaxed agent-scope atomics: every value a lane can see is
// an ancestor of its node, and only a launch that moved nothing ends the jumps.  Everything is integer; no compare-and-swap loop.
// A height beyond +-MRTX_BOWLS_ZMAX is clamped wherever it is read.
// Own translation unit: the existing kernels are compiled exactly as before.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mrtx_bowls.h"
#include "mrtx_lattice_dev.h"

namespace mrtx_bw {

typedef unsigned long long u64;
using namespace mrtx_lat;       // xor64

constexpr u64 kNoKey = ~0ull;

__device__ constexpr int kDi[8] = {-1, -1, 0, 1, 1, 1, 0, -1};   // N, NE, E, SE, S, SW, W, NW
__device__ constexpr int kDj[8] = {0, 1, 1, 1, 0, -1, -1, -1};

__device__ __forceinline__ int32_t clamp_z(int32_t z) { return z < -MRTX_BOWLS_ZMAX ? -MRTX_BOWLS_ZMAX : z > MRTX_BOWLS_ZMAX ? MRTX_BOWLS_ZMAX : z; }

// the height the sweep sees: clamped, negated with invert
__device__ __forceinline__ int32_t swept_z(const BowlC& q, int64_t n) {
    const int32_t z = clamp_z(q.z[n]);
    return q.invert ? -z : z;
}

__device__ __forceinline__ u64 key_of(const BowlC& q, int64_t n) {
    return ((u64)((uint32_t)swept_z(q, n) + 0x40000000u) << 32) | (u64)(uint32_t)n;
}

// neighbour k of node (i, j), or -1: no edge crosses the first or the last row, wrap joins the last column to the first
__device__ __forceinline__ int64_t neighbour(const BowlC& q, int64_t i, int64_t j, int k) {
    const int64_t a = i + kDi[k];
    int64_t b = j + kDj[k];
    if (a < 0 || a >= q.rows) return -1;
    if (b < 0 || b >= q.cols) {
        if (!q.wrap) return -1;
        b = b < 0 ? b + q.cols : b - q.cols;
    }
    return a * q.cols + b;
}

__device__ __forceinline__ bool is_outlet(const BowlC& q, int64_t i, int64_t j, int64_t n) {
    if (q.edge_outlets && (i == 0 || i == q.rows - 1 || (!q.wrap && (j == 0 || j == q.cols - 1)))) return true;
    return q.outlet && q.outlet[n] != 0;
}

__device__ __forceinline__ uint32_t ld32(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st32(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// one lane per entry of 0 .. N: the descent pointer of a node, ptr[N] = N for the outside, every catchment its own component.
// A wave takes 64 consecutive entries, so its minima are counted by one ballot.
__global__ void __launch_bounds__(256) bowls_init_kernel(const BowlC q) {
    const int64_t N = (int64_t)q.rows * q.cols;
    const int step = q.conn8 ? 1 : 2;
    const int lane = threadIdx.x & 63;
    uint32_t bad = 0, minima = 0;
    for (int64_t base = blockIdx.x * (int64_t)256 + (threadIdx.x & ~63); base <= N; base += (int64_t)gridDim.x * 256) {
        const int64_t n = base + lane;
        bool is_min = false;
        if (n == N) {
            q.ptr[N] = (uint32_t)N;
            q.cpar[N] = (uint32_t)N;
        } else if (n < N) {
            const int64_t i = n / q.cols, j = n % q.cols;
            const int32_t zr = q.z[n];
            bad += zr < -MRTX_BOWLS_ZMAX || zr > MRTX_BOWLS_ZMAX;
            int64_t to = N;
            if (!is_outlet(q, i, j, n)) {
                u64 least = key_of(q, n);
                to = n;
                for (int k = 0; k < 8; k += step) {
                    const int64_t u = neighbour(q, i, j, k);
                    if (u < 0) continue;
                    const u64 ku = key_of(q, u);
                    if (ku < least) {
                        least = ku;
                        to = u;
                    }
                }
                is_min = to == n;
            }
            q.ptr[n] = (uint32_t)to;
            q.cpar[n] = (uint32_t)n;
        }
        minima += (uint32_t)__popcll(__ballot(is_min));
    }
    if (bad) atomicAdd(&q.counters[0], bad);
    if (lane == 0 && minima) atomicAdd(&q.counters[1], minima);
}

// ptr[n] = the pointer a few hops further on, in place.  ptr[r] == r only for a minimum and for N, and every value ever stored
// in ptr[n] lies on n's descent path, so a stale read only costs a hop.
__global__ void __launch_bounds__(256) bowls_jump_kernel(const BowlC q) {
    const int64_t N = (int64_t)q.rows * q.cols;
    bool any = false;
    for (int64_t n = blockIdx.x * (int64_t)256 + threadIdx.x; n < N; n += (int64_t)gridDim.x * 256) {
        uint32_t p = ld32(&q.ptr[n]);
        bool moved = false;
        for (int h = 0; h < 4; h++) {
            const uint32_t r = ld32(&q.ptr[p]);
            if (r == p) break;
            p = r;
            moved = true;
        }
        if (moved) {
            st32(&q.ptr[n], p);
            any = true;
        }
    }
    if (any) st32(&q.counters[8 + q.slot], 1u);
}

// the minima's packed keys: one cursor step per wave
__global__ void __launch_bounds__(256) bowls_list_kernel(const BowlC q) {
    const int64_t N = (int64_t)q.rows * q.cols;
    const int lane = threadIdx.x & 63;
    for (int64_t base = blockIdx.x * (int64_t)256 + (threadIdx.x & ~63); base < N; base += (int64_t)gridDim.x * 256) {
        const int64_t n = base + lane;
        const bool is_min = n < N && q.ptr[n] == (uint32_t)n;
        const u64 mask = __ballot(is_min);
        if (!mask) continue;
        uint32_t at = 0;
        if (lane == 0) at = atomicAdd(&q.counters[3], (uint32_t)__popcll(mask));
        at = __shfl(at, 0);
        const uint32_t mine = at + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        if (is_min && mine < q.n_min) q.list[mine] = key_of(q, n);
    }
}

// entry i of the component list: a minimum, or the outside for i == n_min
__device__ __forceinline__ uint32_t listed(const BowlC& q, uint32_t i) {
    return i == q.n_min ? (uint32_t)((int64_t)q.rows * q.cols) : (uint32_t)q.list[i];
}

__global__ void __launch_bounds__(256) bowls_reset_kernel(const BowlC q) {
    for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i <= (int64_t)q.n_min; i += (int64_t)gridDim.x * 256) {
        const uint32_t c = listed(q, (uint32_t)i);
        q.best[c] = kNoKey;
        q.best2[c] = 0xFFFFFFFFu;
    }
}

__device__ __forceinline__ void bid(u64* slot, u64 key) {
    if (key < __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(slot, key);
}

// one lane per node v, the upper end of its edges to the neighbours of lesser key
template <bool TIE>
__global__ void __launch_bounds__(256) bowls_bid_kernel(const BowlC q) {
    const int64_t N = (int64_t)q.rows * q.cols;
    const int step = q.conn8 ? 1 : 2;
    for (int64_t v = blockIdx.x * (int64_t)256 + threadIdx.x; v < N; v += (int64_t)gridDim.x * 256) {
        const int64_t i = v / q.cols, j = v % q.cols;
        const uint32_t cv = q.cpar[q.ptr[v]];
        const u64 kv = key_of(q, v);
        const bool v_wins = TIE && q.best[cv] == kv;
        bool cross = false;
        uint32_t seen = cv;
        for (int k = 0; k < 8; k += step) {
            const int64_t u = neighbour(q, i, j, k);
            if (u < 0 || key_of(q, u) >= kv) continue;
            const uint32_t cu = q.cpar[q.ptr[u]];
            if (cu == cv) continue;
            cross = true;
            if (TIE) {
                if (v_wins && (uint32_t)u < ld32(&q.best2[cv])) atomicMin(&q.best2[cv], (uint32_t)u);
                if (q.best[cu] == kv && (uint32_t)u < ld32(&q.best2[cu])) atomicMin(&q.best2[cu], (uint32_t)u);
            } else if (cu != seen) {
                seen = cu;
                bid(&q.best[cu], kv);
            }
        }
        if (!TIE && cross) bid(&q.best[cv], kv);
    }
}

// one lane per listed component that is still a root and has a cross edge: where it hooks, and the edge it hooks by
__global__ void __launch_bounds__(256) bowls_hook_kernel(const BowlC q) {
    for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i <= (int64_t)q.n_min; i += (int64_t)gridDim.x * 256) {
        const uint32_t c = listed(q, (uint32_t)i);
        uint32_t to = MRTX_BOWLS_NOHOOK;
        const u64 kc = q.best[c];
        if (q.cpar[c] == c && kc != kNoKey) {
            const uint32_t v = (uint32_t)kc, u = q.best2[c];
            const uint32_t N = (uint32_t)((int64_t)q.rows * q.cols);
            if (v < N && u < N) {                    // (the tie pass gave every winning key a low end)
                const uint32_t rv = q.ptr[v], ru = q.ptr[u];
                const uint32_t cv = q.cpar[rv], cu = q.cpar[ru];
                const uint32_t d = cv == c ? cu : cv;
                const bool mutual = q.best[d] == kc && q.best2[d] == u;
                if (d != c && !(mutual && c < d)) {
                    to = d;
                    const uint32_t e = atomicAdd(&q.counters[2], 1u);
                    if (e < q.n_min) {
                        BowlEdge edge;
                        edge.pass = kc; edge.a = rv; edge.b = ru;
                        q.edges[e] = edge;
                    } else {
                        atomicAdd(&q.counters[4], 1u);
                    }
                }
            }
        }
        q.hook[i] = to;
    }
}

__global__ void __launch_bounds__(256) bowls_link_kernel(const BowlC q) {
    for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i <= (int64_t)q.n_min; i += (int64_t)gridDim.x * 256) {
        const uint32_t to = q.hook[i];
        if (to != MRTX_BOWLS_NOHOOK) q.cpar[listed(q, (uint32_t)i)] = to;
    }
}

// cpar[c] = the root of c's tree of hooks.  Another lane's store only replaces a parent by an ancestor further up, so the walk
// ends at the same root whatever it sees; the hooks form a forest, and the hop count is bounded all the same.
__global__ void __launch_bounds__(256) bowls_flatten_kernel(const BowlC q) {
    for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i <= (int64_t)q.n_min; i += (int64_t)gridDim.x * 256) {
        const uint32_t c = listed(q, (uint32_t)i);
        uint32_t r = ld32(&q.cpar[c]);
        if (r == c) continue;
        for (uint32_t h = 0; h <= q.n_min; h++) {
            const uint32_t p = ld32(&q.cpar[r]);
            if (p == r) break;
            r = p;
        }
        st32(&q.cpar[c], r);
    }
}

// ---- the labels
// the leaf bowl of every minimum, into the table that held the components
__global__ void __launch_bounds__(256) bowls_leaf_kernel(const BowlC q) {
    const int64_t N = (int64_t)q.rows * q.cols;
    for (int64_t b = blockIdx.x * (int64_t)256 + threadIdx.x; b < (int64_t)q.n_bowls; b += (int64_t)gridDim.x * 256) {
        const int32_t at = q.walk[b].leaf_at;
        if (at >= 0 && at < N) q.cpar[at] = (uint32_t)b;
    }
}

struct OwnSum {
    u64 weight, wz;
    uint32_t count;
};

__device__ __forceinline__ OwnSum wave_sum(OwnSum v) {
    for (int m = 1; m < 64; m <<= 1) {
        v.weight += xor64(v.weight, m);
        v.wz += xor64(v.wz, m);
        v.count += __shfl_xor(v.count, m);
    }
    return v;
}

__device__ __forceinline__ void own_add(const BowlC& q, int32_t b, const OwnSum& v) {
    u64* e = &q.own[3 * (size_t)b];
    atomicAdd(&e[0], (u64)v.count);
    atomicAdd(&e[1], v.weight);
    atomicAdd(&e[2], v.wz);
}

constexpr int kPeel = 4;        // distinct labels a wave sums in its lanes before the lanes that are left add on their own

// A wave takes 64 consecutive nodes.  label[v]: from the leaf of v's catchment up the parents to the first bowl whose spill key
// lies above key(v); -1 where the catchment is the outside or the chain ends.  parent > child, so the walk ends.
__global__ void __launch_bounds__(256) bowls_label_kernel(const BowlC q) {
    const int64_t N = (int64_t)q.rows * q.cols;
    const int lane = threadIdx.x & 63;
    for (int64_t base = blockIdx.x * (int64_t)256 + (threadIdx.x & ~63); base < N; base += (int64_t)gridDim.x * 256) {
        const int64_t n = base + lane;
        const bool in = n < N;
        int32_t b = -1;
        OwnSum v;
        v.weight = 0; v.wz = 0; v.count = 0;
        if (in) {
            const uint32_t m = q.ptr[n];
            if (m < (uint32_t)N) {
                const u64 kn = key_of(q, n);
                b = (int32_t)q.cpar[m];
                while (b >= 0 && (uint32_t)b < q.n_bowls) {
                    const BowlWalk w = q.walk[b];
                    if (kn < w.spill) break;
                    b = w.parent > b ? w.parent : -1;
                }
                if (b >= 0 && (uint32_t)b >= q.n_bowls) b = -1;
            }
            if (q.label) q.label[n] = b;
            if (b >= 0) {
                v.weight = q.row_weight ? (u64)q.row_weight[n / q.cols] : 1ull;
                v.wz = v.weight * (u64)(long long)swept_z(q, n);
                v.count = 1u;
            }
        }
        bool open = b >= 0;
        u64 pending = __ballot(open);
        for (int r = 0; r < kPeel && pending; r++) {
            const int lead = __ffsll((long long)pending) - 1;
            const int32_t bl = __shfl(b, lead);
            const bool mine = open && b == bl;
            OwnSum none;
            none.weight = 0; none.wz = 0; none.count = 0;
            const OwnSum s = wave_sum(mine ? v : none);
            if (lane == lead) own_add(q, bl, s);
            if (mine) open = false;
            pending = __ballot(open);
        }
        if (open) own_add(q, b, v);
    }
}

}  // namespace mrtx_bw

static unsigned bowls_grid(int64_t n, int per_block) {
    const int64_t b = (n + per_block - 1) / per_block;
    return (unsigned)(b < 1 ? 1 : b > 65536 ? 65536 : b);
}

static bool bowls_block_ok(const BowlC& q) {
    return q.rows >= 1 && q.cols >= 1 && (int64_t)q.rows * q.cols <= ((int64_t)1 << 31) && q.z && q.ptr && q.cpar && q.counters;
}

hipError_t mrtx_launch_bowls_init(const BowlC& q, hipStream_t st) {
    if (!bowls_block_ok(q)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mrtx_bw::bowls_init_kernel, dim3(bowls_grid((int64_t)q.rows * q.cols + 1, 256)), dim3(256), 0, st, q);
    return hipGetLastError();
}

hipError_t mrtx_launch_bowls_jump(const BowlC& q, hipStream_t st) {
    if (!bowls_block_ok(q) || q.slot < 0 || q.slot >= MRTX_BOWLS_BATCH) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mrtx_bw::bowls_jump_kernel, dim3(bowls_grid((int64_t)q.rows * q.cols, 256)), dim3(256), 0, st, q);
    return hipGetLastError();
}

hipError_t mrtx_launch_bowls_list(const BowlC& q, hipStream_t st) {
    if (!bowls_block_ok(q) || !q.list || q.n_min < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mrtx_bw::bowls_list_kernel, dim3(bowls_grid((int64_t)q.rows * q.cols, 256)), dim3(256), 0, st, q);
    return hipGetLastError();
}

// one round over the components: reset, bid, tie, hook, link, flatten
hipError_t mrtx_launch_bowls_round(const BowlC& q, hipStream_t st, uint32_t* launches) {
    if (!bowls_block_ok(q) || !q.list || !q.best || !q.best2 || !q.hook || !q.edges || q.n_min < 1) return hipErrorInvalidValue;
    const dim3 block(256), nodes(bowls_grid((int64_t)q.rows * q.cols, 256)), comps(bowls_grid((int64_t)q.n_min + 1, 256));
    hipLaunchKernelGGL(mrtx_bw::bowls_reset_kernel, comps, block, 0, st, q);
    hipLaunchKernelGGL(mrtx_bw::bowls_bid_kernel<false>, nodes, block, 0, st, q);
    hipLaunchKernelGGL(mrtx_bw::bowls_bid_kernel<true>, nodes, block, 0, st, q);
    hipLaunchKernelGGL(mrtx_bw::bowls_hook_kernel, comps, block, 0, st, q);
    hipLaunchKernelGGL(mrtx_bw::bowls_link_kernel, comps, block, 0, st, q);
    hipLaunchKernelGGL(mrtx_bw::bowls_flatten_kernel, comps, block, 0, st, q);
    if (launches) *launches += 6u;
    return hipGetLastError();
}

hipError_t mrtx_launch_bowls_label(const BowlC& q, hipStream_t st, uint32_t* launches) {
    if (!bowls_block_ok(q) || (q.n_bowls && (!q.walk || !q.own))) return hipErrorInvalidValue;
    const dim3 block(256);
    if (q.n_bowls) hipLaunchKernelGGL(mrtx_bw::bowls_leaf_kernel, dim3(bowls_grid(q.n_bowls, 256)), block, 0, st, q);
    hipLaunchKernelGGL(mrtx_bw::bowls_label_kernel, dim3(bowls_grid((int64_t)q.rows * q.cols, 256)), block, 0, st, q);
    if (launches) *launches += q.n_bowls ? 2u : 1u;
    return hipGetLastError();
}
