// mrtx_regions.hip -- gfx950 kernels of the regions stage (mrtx_regions_label, mrtx_regions_stats; DESIGN.md sections 3.20, 4.26).
//
// Connected components of a set of lattice nodes, exact integer work.  The labelling is a union-find in a table of node indices
// with the invariant parent[v] <= v (-1 outside the set), so every walk towards a root strictly descends and ends, and a
// component's root is its least node index.  The number of launches depends on nothing but the window:
//   label_tile_kernel      one 256-lane workgroup per tile of 16 x 64 nodes: the predicate, then the tile's own components in
//                          LDS to convergence (the loop stays inside the workgroup); parent[v] = the tile-local root
//   label_seam_kernel      one lane per node: the edges the tile pass did not see (across a tile border, across the wrapped
//                          column) union the two trees; parent is written with atomicMin only
//   label_flatten_kernel   parent[v] = find(v), and the roots of every chunk of 4096 nodes counted
//   label_scan_kernel      one workgroup: the exclusive prefix of the chunks' counts, and K
//   label_rank_kernel      every root's rank among the roots into labels
//   label_apply_kernel     labels[v] = labels[parent[v]] for the rest, -1 outside the set
// and the catalogue over a label table that may be the caller's own (every entry bound-checked, nothing written for a bad one):
//   stats_init_kernel      the records' identities
//   stats_root_kernel      the least node index of every label, and the count of bad entries
//   stats_sum_kernel<RUNS> count, weight, sum_i, sum_dj and the extents: with RUNS the lanes of a wave that follow each other
//                          with one label are reduced in the wave first, a run that reaches the wave's end is carried into
//                          the wave's next 64 nodes, and only run heads issue atomics; without, one set of atomics per node
//                          (the yardstick, MOONRT_REGIONS_CATALOGUE=plain)
//   stats_finish_kernel    the root's index split into (root_i, root_j)
// No kernel waits on another workgroup.  Own translation unit: the existing kernels are compiled exactly as before.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mrtx_regions.h"
#include "mrtx_lattice_dev.h"

namespace mrtx_rg {
using namespace mrtx_lat;       // value_now

constexpr int TH = MRTX_RG_TH, TW = MRTX_RG_TW, TN = TH * TW;
constexpr int CHUNK = MRTX_RG_CHUNK;

// is node n (row-major, 64-bit) in the set?  NaN fails both comparisons
__device__ __forceinline__ bool in_set(const RegionsC& q, int64_t n) {
    if (q.mask) return q.mask[n] != 0;
    const float x = q.field[n * q.n_ch + q.ch];
    return x >= q.lo && x <= q.hi;
}

__global__ void __launch_bounds__(256) label_tile_kernel(const RegionsC q) {
    __shared__ int lab[TN];
    __shared__ int changed;
    const int t = threadIdx.x;
    const int64_t ty = blockIdx.x / (unsigned)q.tiles_x, tx = blockIdx.x % (unsigned)q.tiles_x;
    const int64_t i0 = ty * TH, j0 = tx * TW;
    for (int k = 0; k < TN / 256; k++) {
        const int p = t + 256 * k, a = p / TW, b = p % TW;
        const int64_t i = i0 + a, j = j0 + b;
        lab[p] = (i < q.rows && j < q.cols && in_set(q, i * q.cols + j)) ? p : -1;
    }
    for (;;) {
        __syncthreads();
        if (t == 0) changed = 0;
        __syncthreads();
        // every node hangs its label's tree under the least label among its neighbours
        for (int k = 0; k < TN / 256; k++) {
            const int p = t + 256 * k, a = p / TW, b = p % TW;
            const int l = lab[p];
            if (l < 0) continue;
            int m = l;
            for (int da = -1; da <= 1; da++)
                for (int db = -1; db <= 1; db++) {
                    if ((da == 0 && db == 0) || (!q.conn8 && da != 0 && db != 0)) continue;
                    const int na = a + da, nb = b + db;
                    if (na < 0 || na >= TH || nb < 0 || nb >= TW) continue;
                    const int lq = lab[na * TW + nb];
                    if (lq >= 0 && lq < m) m = lq;
                }
            if (m < l) { atomicMin(&lab[l], m); changed = 1; }
        }
        __syncthreads();
        // flatten: roots (lab[r] == r) do not change here, so a walk through a node that is being rewritten ends the same
        for (int k = 0; k < TN / 256; k++) {
            const int p = t + 256 * k;
            int r = lab[p];
            if (r < 0) continue;
            for (int x; (x = lab[r]) != r;) r = x;
            lab[p] = r;
        }
        __syncthreads();
        if (!changed) break;
    }
    for (int k = 0; k < TN / 256; k++) {
        const int p = t + 256 * k, a = p / TW, b = p % TW;
        const int64_t i = i0 + a, j = j0 + b;
        if (i >= q.rows || j >= q.cols) continue;
        const int r = lab[p];
        q.parent[i * q.cols + j] = r < 0 ? -1 : (int32_t)((i0 + r / TW) * q.cols + j0 + r % TW);
    }
}

// a parent entry as every workgroup of the device sees it
__device__ __forceinline__ int32_t parent_now(const int32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int32_t find_now(const int32_t* parent, int32_t x) {
    for (int32_t p; (p = parent_now(parent + x)) != x;) x = p;
    return x;
}

// Union of the trees of a and b.  Only roots are written, only downwards and only by atomicMin, so parent[v] <= v holds.  When
// the atomicMin meets a value `old` other than the root itself, another union got there first: the root now hangs under
// min(old, b), and what is left to join is old and b.  Every retry starts strictly below the last one.
__device__ void unite(int32_t* parent, int32_t a, int32_t b) {
    for (;;) {
        a = find_now(parent, a);
        b = find_now(parent, b);
        if (a == b) return;
        if (a < b) { const int32_t s = a; a = b; b = s; }
        const int32_t old = atomicMin(parent + a, b);
        if (old == a) return;
        a = old;
    }
}

__global__ void __launch_bounds__(256) label_seam_kernel(const RegionsC q) {
    const int64_t N = (int64_t)q.rows * q.cols;
    for (int64_t n = blockIdx.x * (int64_t)256 + threadIdx.x; n < N; n += (int64_t)gridDim.x * 256) {
        const int64_t i = n / q.cols, j = n % q.cols;
        // only nodes on a tile's first row, its first or last column, or the window's last column have such an edge
        if (i % TH != 0 && j % TW != 0 && (j + 1) % TW != 0 && j != q.cols - 1) continue;
        if (q.parent[n] < 0) continue;
        // the four neighbours behind the node: W, N, NW, NE; each edge of the lattice is some node's
        const int di[4] = {0, -1, -1, -1}, dj[4] = {-1, 0, -1, 1};
        for (int k = 0; k < 4; k++) {
            if (k >= 2 && !q.conn8) break;
            const int64_t ni = i + di[k];
            int64_t nj = j + dj[k];
            bool seam = false;
            if (ni < 0) continue;
            if (nj < 0 || nj >= q.cols) {
                if (!q.wrap) continue;
                nj = nj < 0 ? q.cols - 1 : 0;
                seam = true;
            }
            if (!seam && ni / TH == i / TH && nj / TW == j / TW) continue;     // the tile pass joined these
            const int64_t m = ni * q.cols + nj;
            if (q.parent[m] < 0) continue;
            unite(q.parent, (int32_t)n, (int32_t)m);
        }
    }
}

// the sum of v over the workgroup's 256 lanes, in every lane
__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t* s4) {
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
    __syncthreads();
    return s4[0] + s4[1] + s4[2] + s4[3];
}

// The seam pass is over: roots stay roots.  Other lanes shorten paths at the same time; an entry read is the old parent or
// the root, and both lead to the same root.
__global__ void __launch_bounds__(256) label_flatten_kernel(const RegionsC q) {
    __shared__ uint32_t s4[4];
    const int64_t N = (int64_t)q.rows * q.cols;
    for (uint32_t c = blockIdx.x; c < q.n_chunks; c += gridDim.x) {
        uint32_t roots = 0;
        for (int k = 0; k < CHUNK / 256; k++) {
            const int64_t n = (int64_t)c * CHUNK + k * 256 + threadIdx.x;
            if (n >= N) break;
            int32_t r = q.parent[n];
            if (r < 0) continue;
            for (int32_t x; (x = q.parent[r]) != r;) r = x;
            q.parent[n] = r;
            roots += r == (int32_t)n;
        }
        const uint32_t all = block_sum(roots, s4);
        if (threadIdx.x == 0) q.sums[c] = all;
    }
}

// one workgroup: lane t folds its own stretch of the counts, the 256 stretch sums are scanned in LDS, then the stretch again
__global__ void __launch_bounds__(256) label_scan_kernel(const RegionsC q) {
    __shared__ uint32_t s[256];
    const int t = threadIdx.x;
    const uint32_t per = (q.n_chunks + 255) / 256;
    const uint32_t a = min((uint32_t)t * per, q.n_chunks), b = min(a + per, q.n_chunks);
    uint32_t sum = 0;
    for (uint32_t c = a; c < b; c++) sum += q.sums[c];
    s[t] = sum;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const uint32_t u = t >= d ? s[t - d] : 0u;
        __syncthreads();
        s[t] += u;
        __syncthreads();
    }
    uint32_t run = s[t] - sum;
    for (uint32_t c = a; c < b; c++) {
        const uint32_t v = q.sums[c];
        q.sums[c] = run;
        run += v;
    }
    if (t == 255) *q.total = s[255];
}

// a root's rank: the roots of the chunks before its own, of the earlier 256-node rows of its chunk, of the earlier waves of its
// row, and of the lower lanes of its wave
__global__ void __launch_bounds__(256) label_rank_kernel(const RegionsC q) {
    __shared__ uint32_t w4[4];
    const int64_t N = (int64_t)q.rows * q.cols;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t c = blockIdx.x; c < q.n_chunks; c += gridDim.x) {
        uint32_t base = q.sums[c];
        for (int k = 0; k < CHUNK / 256; k++) {
            const int64_t n = (int64_t)c * CHUNK + k * 256 + threadIdx.x;
            const bool root = n < N && q.parent[n] == (int32_t)n;
            const unsigned long long m = __ballot(root);
            __syncthreads();
            if (lane == 0) w4[wave] = (uint32_t)__popcll(m);
            __syncthreads();
            uint32_t before = 0;
            for (int w = 0; w < wave; w++) before += w4[w];
            if (root) q.labels[n] = (int32_t)(base + before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull)));
            base += w4[0] + w4[1] + w4[2] + w4[3];
        }
    }
}

__global__ void __launch_bounds__(256) label_apply_kernel(const RegionsC q) {
    const int64_t N = (int64_t)q.rows * q.cols;
    for (int64_t n = blockIdx.x * (int64_t)256 + threadIdx.x; n < N; n += (int64_t)gridDim.x * 256) {
        const int32_t p = q.parent[n];
        if (p < 0) q.labels[n] = -1;
        else if (p != (int32_t)n) q.labels[n] = q.labels[p];      // a root's entry, written by the launch before this one
    }
}

// ---- the catalogue
__global__ void __launch_bounds__(256) stats_init_kernel(const RegionStatsC q) {
    for (uint32_t r = blockIdx.x * 256u + threadIdx.x; r < q.n_regions; r += gridDim.x * 256u) {
        RegionRec z;
        z.weight = 0; z.sum_i = 0; z.sum_dj = 0; z.count = 0;
        z.root_i = 0x7FFFFFFF; z.root_j = 0;
        z.i_min = 0x7FFFFFFF; z.i_max = -0x7FFFFFFF - 1; z.dj_min = 0x7FFFFFFF; z.dj_max = -0x7FFFFFFF - 1;
        z.reserved = 0;
        q.out[r] = z;
    }
}

// a table entry is a region's iff 0 <= l < n_regions; -1 is outside every region; anything else is counted as bad
__device__ __forceinline__ bool label_ok(const RegionStatsC& q, int32_t l) { return l >= 0 && (uint32_t)l < q.n_regions; }

__global__ void __launch_bounds__(256) stats_root_kernel(const RegionStatsC q) {
    const int64_t N = (int64_t)q.rows * q.cols;
    const int lane = threadIdx.x & 63;
    uint32_t bad = 0;
    // the trip count is the wave's, so that every lane takes part in the shuffle
    for (int64_t n0 = (blockIdx.x * (int64_t)256 + threadIdx.x) - lane; n0 < N; n0 += (int64_t)gridDim.x * 256) {
        const int64_t n = n0 + lane;
        const int32_t l = n < N ? q.labels[n] : -1;
        const int32_t before = __shfl_up(l, 1);
        bad += l < -1 || (l >= 0 && (uint32_t)l >= q.n_regions);
        // nodes ascend along the wave: of lanes that follow each other with one label, the first holds the least index; and
        // the entry only ever falls, so a node that is not below what is read now cannot lower it
        if (label_ok(q, l) && (lane == 0 || before != l) && (int32_t)n < value_now(&q.out[l].root_i))
            atomicMin(&q.out[l].root_i, (int32_t)n);
    }
    if (bad) atomicAdd(q.bad, bad);
}

struct RunSum {
    unsigned long long weight, sum_i, sum_dj;
    uint32_t count;
    int32_t i_min, i_max, dj_min, dj_max;
};

__device__ __forceinline__ RunSum run_none() {
    RunSum v;
    v.weight = 0; v.sum_i = 0; v.sum_dj = 0; v.count = 0;
    v.i_min = 0x7FFFFFFF; v.i_max = -0x7FFFFFFF - 1; v.dj_min = 0x7FFFFFFF; v.dj_max = -0x7FFFFFFF - 1;
    return v;
}

__device__ __forceinline__ void run_join(RunSum& v, const RunSum& u) {
    v.weight += u.weight; v.sum_i += u.sum_i; v.sum_dj += u.sum_dj; v.count += u.count;
    v.i_min = min(v.i_min, u.i_min); v.i_max = max(v.i_max, u.i_max);
    v.dj_min = min(v.dj_min, u.dj_min); v.dj_max = max(v.dj_max, u.dj_max);
}

// the yardstick: every field, unconditionally
__device__ __forceinline__ void add_record_plain(RegionRec* r, const RunSum& v) {
    atomicAdd(&r->weight, v.weight);
    atomicAdd(&r->sum_i, v.sum_i);
    atomicAdd(&r->sum_dj, v.sum_dj);
    atomicAdd(&r->count, v.count);
    atomicMin(&r->i_min, v.i_min);
    atomicMax(&r->i_max, v.i_max);
    atomicMin(&r->dj_min, v.dj_min);
    atomicMax(&r->dj_max, v.dj_max);
}

// A run's sums into its record.  Without row weights the weight is the count and stats_finish_kernel copies it.  An extent
// only ever moves outwards, so a read of it, however old, is no further out than the record's: an atomic that would not
// move what was read cannot move the record either and is left out.
__device__ __forceinline__ void add_record(RegionRec* r, const RunSum& v, bool weighted) {
    if (weighted) atomicAdd(&r->weight, v.weight);
    atomicAdd(&r->sum_i, v.sum_i);
    atomicAdd(&r->sum_dj, v.sum_dj);
    atomicAdd(&r->count, v.count);
    if (v.i_min < value_now(&r->i_min)) atomicMin(&r->i_min, v.i_min);
    if (v.i_max > value_now(&r->i_max)) atomicMax(&r->i_max, v.i_max);
    if (v.dj_min < value_now(&r->dj_min)) atomicMin(&r->dj_min, v.dj_min);
    if (v.dj_max > value_now(&r->dj_max)) atomicMax(&r->dj_max, v.dj_max);
}

__device__ __forceinline__ RunSum run_from_lane(const RunSum& v, int src) {
    RunSum u;
    u.weight = __shfl(v.weight, src);
    u.sum_i = __shfl(v.sum_i, src);
    u.sum_dj = __shfl(v.sum_dj, src);
    u.count = __shfl(v.count, src);
    u.i_min = __shfl(v.i_min, src);
    u.i_max = __shfl(v.i_max, src);
    u.dj_min = __shfl(v.dj_min, src);
    u.dj_max = __shfl(v.dj_max, src);
    return u;
}

// A wave takes a stretch of STRETCH x 64 consecutive nodes, 64 at a time.  With RUNS the run that reaches the wave's last
// lane is not added to its record but carried into the next 64 nodes, where it goes on if lane 0 has its label: a region
// that fills rows adds to its record once per stretch, holes or not.
constexpr int STRETCH = 16;

template <bool RUNS>
__global__ void __launch_bounds__(256) stats_sum_kernel(const RegionStatsC q) {
    const int64_t N = (int64_t)q.rows * q.cols;
    const int lane = threadIdx.x & 63;
    const int32_t half = q.cols / 2;
    const bool weighted = q.row_weight != nullptr;
    const int64_t per_wave = 64 * STRETCH;
    for (int64_t s0 = (blockIdx.x * (int64_t)4 + (threadIdx.x >> 6)) * per_wave; s0 < N; s0 += (int64_t)gridDim.x * 4 * per_wave) {
        RunSum carry = run_none();
        int32_t carry_l = -1;
        for (int it = 0; it < STRETCH && s0 + it * 64 < N; it++) {     // the trip count is the wave's
            const int64_t n = s0 + it * 64 + lane;
            int32_t l = n < N ? q.labels[n] : -1;
            if (!label_ok(q, l)) l = -1;
            RunSum v = run_none();
            if (l >= 0) {
                const int32_t i = (int32_t)(n / q.cols), j = (int32_t)(n % q.cols);
                const int32_t rj = q.out[l].root_i % q.cols;        // the root's node index, final since the launch before
                int32_t dj = j - rj;
                if (q.wrap) {
                    int32_t m = (dj + half) % q.cols;
                    if (m < 0) m += q.cols;
                    dj = m - half;
                }
                v.weight = weighted ? q.row_weight[i] : 1u;
                v.sum_i = (unsigned long long)(long long)i;
                v.sum_dj = (unsigned long long)(long long)dj;
                v.count = 1;
                v.i_min = v.i_max = i;
                v.dj_min = v.dj_max = dj;
            }
            if (!RUNS) {
                if (l >= 0) add_record_plain(q.out + l, v);
                continue;
            }
            // a lane outside every region takes the label of the last lane before it that is inside one (of the carried run
            // when there is none) and adds nothing: holes do not cut a region's run
            const unsigned long long inside = __ballot(l >= 0);
            const unsigned long long below = inside & ((1ull << lane) - 1ull);
            const int32_t seen = __shfl(l, below ? 63 - __clzll((long long)below) : 0);
            if (l < 0) l = below ? seen : carry_l;
            // run heads: a lane whose label differs from the lane before it; a run ends before the next head
            const int32_t before = __shfl_up(l, 1);
            const unsigned long long heads = __ballot(lane == 0 || before != l);
            const unsigned long long above = lane == 63 ? 0ull : heads & ~((2ull << lane) - 1ull);
            const int end = above ? __ffsll((long long)above) - 1 : 64;
            // after the step of width d a lane holds the sum of its run's lanes [lane, lane + 2 d)
            for (int d = 1; d < 64; d <<= 1) {
                RunSum u;
                u.weight = __shfl_down(v.weight, d);
                u.sum_i = __shfl_down(v.sum_i, d);
                u.sum_dj = __shfl_down(v.sum_dj, d);
                u.count = __shfl_down(v.count, d);
                u.i_min = __shfl_down(v.i_min, d);
                u.i_max = __shfl_down(v.i_max, d);
                u.dj_min = __shfl_down(v.dj_min, d);
                u.dj_max = __shfl_down(v.dj_max, d);
                if (lane + d < end) run_join(v, u);
            }
            // The carried run takes every run of its label among these 64 nodes, wherever it starts: a region with islands
            // of other regions inside it still adds to its record once per stretch.  When none has its label the carried
            // run is over, and the run that reaches lane 63 is carried instead.
            const bool head = ((heads >> lane) & 1ull) != 0 && l >= 0 && v.count != 0;
            const bool mine = head && l == carry_l;
            const unsigned long long match = __ballot(mine);
            if (match) {
                RunSum m = mine ? v : run_none();
                if (__popcll(match) == 1) {
                    m = run_from_lane(v, __ffsll((long long)match) - 1);
                } else {
                    for (int d = 32; d >= 1; d >>= 1) {
                        RunSum u;
                        u.weight = __shfl_xor(m.weight, d);
                        u.sum_i = __shfl_xor(m.sum_i, d);
                        u.sum_dj = __shfl_xor(m.sum_dj, d);
                        u.count = __shfl_xor(m.count, d);
                        u.i_min = __shfl_xor(m.i_min, d);
                        u.i_max = __shfl_xor(m.i_max, d);
                        u.dj_min = __shfl_xor(m.dj_min, d);
                        u.dj_max = __shfl_xor(m.dj_max, d);
                        run_join(m, u);
                    }
                }
                run_join(carry, m);
                if (head && !mine) add_record(q.out + l, v, weighted);
            } else {
                if (carry_l >= 0 && carry.count && lane == 0) add_record(q.out + carry_l, carry, weighted);
                const int last = 63 - __clzll((long long)heads);    // the head of the run that reaches lane 63 (lane 0 is a head)
                carry_l = __shfl(l, last);
                carry = run_from_lane(v, last);
                if (head && lane != last) add_record(q.out + l, v, weighted);
            }
        }
        if (RUNS && carry_l >= 0 && carry.count && lane == 0) add_record(q.out + carry_l, carry, weighted);
    }
}

// a label no node carries keeps count 0: its root is (-1, -1) and its extents are 0
__global__ void __launch_bounds__(256) stats_finish_kernel(const RegionStatsC q) {
    for (uint32_t r = blockIdx.x * 256u + threadIdx.x; r < q.n_regions; r += gridDim.x * 256u) {
        RegionRec* o = q.out + r;
        if (!q.row_weight) o->weight = o->count;
        if (o->count == 0) {
            o->root_i = -1; o->root_j = -1; o->i_min = 0; o->i_max = 0; o->dj_min = 0; o->dj_max = 0;
        } else {
            const int32_t n = o->root_i;
            o->root_i = n / q.cols;
            o->root_j = n % q.cols;
        }
    }
}

}  // namespace mrtx_rg

static unsigned regions_grid(int64_t n, int per_block) {
    const int64_t b = (n + per_block - 1) / per_block;
    return (unsigned)(b < 1 ? 1 : b > 65536 ? 65536 : b);
}

// six launches whatever the set is
hipError_t mrtx_launch_regions_label(const RegionsC& q, hipStream_t st, uint32_t* launches) {
    if (q.rows < 1 || q.cols < 1 || (!q.field) == (!q.mask) || !q.parent || !q.labels || !q.sums || !q.total)
        return hipErrorInvalidValue;
    const int64_t N = (int64_t)q.rows * q.cols;
    const int64_t tiles_x = ((int64_t)q.cols + MRTX_RG_TW - 1) / MRTX_RG_TW, tiles_y = ((int64_t)q.rows + MRTX_RG_TH - 1) / MRTX_RG_TH;
    if (tiles_x * tiles_y > 0x7FFFFFFFll || q.tiles_x != (int32_t)tiles_x ||
        (int64_t)q.n_chunks != (N + MRTX_RG_CHUNK - 1) / MRTX_RG_CHUNK)
        return hipErrorInvalidValue;
    const unsigned gn = regions_grid(N, 256), gc = regions_grid(q.n_chunks, 1);
    hipLaunchKernelGGL(mrtx_rg::label_tile_kernel, dim3((unsigned)(tiles_x * tiles_y)), dim3(256), 0, st, q);
    hipLaunchKernelGGL(mrtx_rg::label_seam_kernel, dim3(gn), dim3(256), 0, st, q);
    hipLaunchKernelGGL(mrtx_rg::label_flatten_kernel, dim3(gc), dim3(256), 0, st, q);
    hipLaunchKernelGGL(mrtx_rg::label_scan_kernel, dim3(1), dim3(256), 0, st, q);
    hipLaunchKernelGGL(mrtx_rg::label_rank_kernel, dim3(gc), dim3(256), 0, st, q);
    hipLaunchKernelGGL(mrtx_rg::label_apply_kernel, dim3(gn), dim3(256), 0, st, q);
    if (launches) *launches = 6;
    return hipGetLastError();
}

// runs: reduce runs of equal labels inside the wave before the atomics.  Without regions only the check of the table runs.
hipError_t mrtx_launch_regions_stats(const RegionStatsC& q, bool runs, hipStream_t st, uint32_t* launches) {
    if (q.rows < 1 || q.cols < 1 || !q.labels || !q.bad || (q.n_regions && !q.out)) return hipErrorInvalidValue;
    const int64_t N = (int64_t)q.rows * q.cols;
    const unsigned gn = regions_grid(N, 256), gr = regions_grid(q.n_regions, 256);
    if (q.n_regions) hipLaunchKernelGGL(mrtx_rg::stats_init_kernel, dim3(gr), dim3(256), 0, st, q);
    hipLaunchKernelGGL(mrtx_rg::stats_root_kernel, dim3(gn), dim3(256), 0, st, q);
    if (q.n_regions) {
        const unsigned gs = regions_grid(N, 256 * mrtx_rg::STRETCH);
        if (runs) hipLaunchKernelGGL(mrtx_rg::stats_sum_kernel<true>, dim3(gs), dim3(256), 0, st, q);
        else hipLaunchKernelGGL(mrtx_rg::stats_sum_kernel<false>, dim3(gs), dim3(256), 0, st, q);
        hipLaunchKernelGGL(mrtx_rg::stats_finish_kernel, dim3(gr), dim3(256), 0, st, q);
    }
    if (launches) *launches = q.n_regions ? 4 : 1;
    return hipGetLastError();
}
