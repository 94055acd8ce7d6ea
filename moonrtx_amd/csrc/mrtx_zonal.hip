// mrtx_zonal.hip -- gfx950 kernels of the zonal statistics and outlines of labelled regions (mrtx_regions_zonal,
// mrtx_regions_shape; DESIGN.md sections 3.21, 4.27).
//
// Streaming passes over a label table that may be the caller's own (every entry bound-checked, nothing indexed by a bad one),
// with per-region integer atomics; no float is ever added, so no result depends on the order of a reduction:
//   check_kernel           the count of entries outside -1 .. n_regions - 1
//   zonal_init_kernel      the records' and the packed extremes' identities, the histogram zeroed
//   zonal_sum_kernel<RUNS> per channel: counts, fixed-point sums and the extremes as packed 64-bit keys.  With RUNS the lanes
//                          of a wave that follow each other with one label are reduced in the wave first, the run that reaches
//                          the wave's last lane is carried into the wave's next 64 nodes, and only run heads issue atomics;
//                          without, one set of atomics per node (the yardstick, MOONRT_REGIONS_ZONAL=plain)
//   zonal_hist_kernel<RUNS> the histogram of one channel: with RUNS a wave carries the columns of one region along its stretch
//                          (rows of at most 128 columns), and the lanes that hit one (region, column) are summed in the wave
//                          first (a peel loop over the first open lane's key)
//   zonal_finish_kernel    the keys unpacked into min, max and their places; wcount and wsum copied without weights
//   shape_init_kernel, shape_sum_kernel<RUNS>, shape_finish_kernel
//                          boundary sides and bit quads per node, the Euler number from 64-bit intermediates
// No kernel waits on another workgroup.  Own translation unit: the existing kernels are compiled exactly as before.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mrtx_zonal.h"
#include "mrtx_lattice_dev.h"

namespace mrtx_zn {

typedef unsigned long long u64;
using namespace mrtx_lat;       // label_ok, value_now, check_labels

// a wave takes a stretch of STRETCH x 64 consecutive nodes, 64 at a time, as the catalogue's stats_sum_kernel does
constexpr int STRETCH = 16;
// distinct (region, column) keys a wave peels before the lanes that are left add on their own
constexpr int PEEL = 8;

__global__ void __launch_bounds__(256) check_kernel(const int32_t* labels, int64_t N, uint32_t n_regions, uint32_t* out) {
    check_labels(labels, N, n_regions, out);
}

// ---- a value of any plain struct of 32-bit words from another lane
template <class V>
__device__ __forceinline__ V lane_from(const V& v, int src) {
    constexpr int W = sizeof(V) / 4;
    static_assert(sizeof(V) % 4 == 0, "whole words");
    uint32_t w[W];
    __builtin_memcpy(w, &v, sizeof(V));
#pragma unroll
    for (int k = 0; k < W; k++) w[k] = __shfl(w[k], src);
    V u;
    __builtin_memcpy(&u, w, sizeof(V));
    return u;
}

template <class V>
__device__ __forceinline__ V lane_down(const V& v, int d) {
    constexpr int W = sizeof(V) / 4;
    uint32_t w[W];
    __builtin_memcpy(w, &v, sizeof(V));
#pragma unroll
    for (int k = 0; k < W; k++) w[k] = __shfl_down(w[k], d);
    V u;
    __builtin_memcpy(&u, w, sizeof(V));
    return u;
}

// The runs of one label among a wave's 64 nodes, every lane of the wave taking part.  l: the lane's label or -1; v: its value
// (V::none() with l < 0).  A lane outside every region takes the label of the last lane before it that is inside one (the
// carried run's when there is none) and adds nothing, so holes do not cut a run.  Every run is summed into its head; the run
// of lane 0 goes on the carried one when it has its label, else lane 0 emits the carried run; the run that reaches lane 63 is
// carried on and every other one emitted.  The caller emits what is carried after the wave's last 64 nodes.
template <class V, class Emit>
__device__ __forceinline__ void wave_runs(int lane, int32_t l, V v, int32_t& carry_l, V& carry, Emit emit) {
    const u64 inside = __ballot(l >= 0);
    const u64 below = inside & ((1ull << lane) - 1ull);
    const int32_t seen = __shfl(l, below ? 63 - __clzll((long long)below) : 0);
    if (l < 0) l = below ? seen : carry_l;
    const int32_t before = __shfl_up(l, 1);
    const u64 heads = __ballot(lane == 0 || before != l);
    const u64 above = lane == 63 ? 0ull : heads & ~((2ull << lane) - 1ull);
    const int end = above ? __ffsll((long long)above) - 1 : 64;
    // after the step of width d a lane holds the sum of its run's lanes [lane, lane + 2 d)
    for (int d = 1; d < 64; d <<= 1) {
        const V u = lane_down(v, d);
        if (lane + d < end) v.join(u);
    }
    if (lane == 0) {
        if (l == carry_l) v.join(carry);
        else if (carry_l >= 0 && carry.nodes) emit(carry_l, carry);
    }
    const int last = 63 - __clzll((long long)heads);        // lane 0 is a head
    carry_l = __shfl(l, last);
    carry = lane_from(v, last);
    if (((heads >> lane) & 1ull) && lane != last && l >= 0 && v.nodes) emit(l, v);
}

// ---- zonal statistics
// the total order of the float32 bit patterns as an unsigned key: -0.0 precedes +0.0
__device__ __forceinline__ uint32_t order_key(float x) {
    const uint32_t b = __float_as_uint(x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float order_value(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

struct ZRun {
    u64 wcount, wsum, sum, kmin, kmax;
    uint32_t count, n_nan, n_clipped, nodes;
    static __device__ __forceinline__ ZRun none() {
        ZRun v;
        v.wcount = 0; v.wsum = 0; v.sum = 0; v.kmin = ~0ull; v.kmax = 0; v.count = 0; v.n_nan = 0; v.n_clipped = 0; v.nodes = 0;
        return v;
    }
    __device__ __forceinline__ void join(const ZRun& u) {
        wcount += u.wcount; wsum += u.wsum; sum += u.sum; count += u.count; n_nan += u.n_nan; n_clipped += u.n_clipped;
        nodes += u.nodes;
        kmin = u.kmin < kmin ? u.kmin : kmin;
        kmax = u.kmax > kmax ? u.kmax : kmax;
    }
};
static_assert(sizeof(ZRun) == 56, "14 words");

// one node's value x of weight w at node index n
__device__ __forceinline__ ZRun zonal_node(float x, double scale, uint32_t w, uint32_t n) {
    ZRun v = ZRun::none();
    v.nodes = 1;
    if (x != x) { v.n_nan = 1; return v; }
    const double p = __dmul_rn((double)x, scale);           // one float64 product
    long long q;
    if (fabs(p) >= 2147483648.0) {
        v.n_clipped = 1;
        q = p < 0.0 ? -2147483648ll : 2147483648ll;
    } else {
        q = __double2ll_rn(p);                              // half to even
    }
    v.count = 1;
    v.wcount = w;
    v.sum = (u64)q;
    v.wsum = (u64)((long long)w * q);                       // |.| <= 2^32 x 2^31
    const u64 k = (u64)order_key(x) << 32;
    v.kmin = k | n;
    v.kmax = k | (uint32_t)~n;
    return v;
}

__global__ void __launch_bounds__(256) zonal_init_kernel(const ZonalC q) {
    const size_t R = (size_t)q.n_regions * (size_t)q.n_ch;
    const size_t H = q.hist ? (size_t)q.n_regions * (size_t)(q.n_bins + 2) : 0;
    const size_t step = (size_t)gridDim.x * 256;
    for (size_t r = blockIdx.x * (size_t)256 + threadIdx.x; r < R; r += step) {
        ZonalRec z;
        z.wcount = 0; z.wsum = 0; z.sum = 0; z.count = 0; z.n_nan = 0; z.n_clipped = 0;
        z.min = __uint_as_float(0x7F800000u); z.max = __uint_as_float(0xFF800000u); z.min_at = -1; z.max_at = -1; z.reserved = 0;
        q.out[r] = z;
        q.keys[2 * r] = ~0ull;
        q.keys[2 * r + 1] = 0ull;
    }
    for (size_t h = blockIdx.x * (size_t)256 + threadIdx.x; h < H; h += step) q.hist[h] = 0ull;
}

// the yardstick: every field, unconditionally
__device__ __forceinline__ void zonal_add_plain(const ZonalC& q, size_t r, const ZRun& v) {
    ZonalRec* o = q.out + r;
    atomicAdd(&o->wcount, v.wcount);
    atomicAdd(&o->wsum, v.wsum);
    atomicAdd(&o->sum, v.sum);
    atomicAdd(&o->count, v.count);
    atomicAdd(&o->n_nan, v.n_nan);
    atomicAdd(&o->n_clipped, v.n_clipped);
    atomicMin(q.keys + 2 * r, v.kmin);
    atomicMax(q.keys + 2 * r + 1, v.kmax);
}

// A run's sums into its record.  Without row weights wcount = count and wsum = sum, which zonal_finish_kernel copies.  A key
// under min only ever falls and one under max only ever rises, so a read of it, however old, is no further out than the entry:
// an atomic that would not move what was read cannot move the entry either and is left out.
__device__ __forceinline__ void zonal_add(const ZonalC& q, size_t r, const ZRun& v, bool weighted) {
    ZonalRec* o = q.out + r;
    if (v.count) {
        if (weighted) {
            atomicAdd(&o->wcount, v.wcount);
            atomicAdd(&o->wsum, v.wsum);
        }
        atomicAdd(&o->sum, v.sum);
        atomicAdd(&o->count, v.count);
        if (v.kmin < value_now(q.keys + 2 * r)) atomicMin(q.keys + 2 * r, v.kmin);
        if (v.kmax > value_now(q.keys + 2 * r + 1)) atomicMax(q.keys + 2 * r + 1, v.kmax);
    }
    if (v.n_nan) atomicAdd(&o->n_nan, v.n_nan);
    if (v.n_clipped) atomicAdd(&o->n_clipped, v.n_clipped);
}

template <bool RUNS>
__global__ void __launch_bounds__(256) zonal_sum_kernel(const ZonalC q) {
    const int64_t N = (int64_t)q.rows * q.cols;
    const int lane = threadIdx.x & 63;
    const bool weighted = q.row_weight != nullptr;
    const int64_t per_wave = 64 * STRETCH;
    for (int64_t s0 = (blockIdx.x * (int64_t)4 + (threadIdx.x >> 6)) * per_wave; s0 < N; s0 += (int64_t)gridDim.x * 4 * per_wave) {
        // a channel at a time, so that one run is carried; the stretch's labels and values come from the cache after the first
        for (int ch = 0; ch < q.n_ch; ch++) {
            ZRun carry = ZRun::none();
            int32_t carry_l = -1;
            for (int it = 0; it < STRETCH && s0 + it * 64 < N; it++) {     // the trip count is the wave's
                const int64_t n = s0 + it * 64 + lane;
                int32_t l = n < N ? q.labels[n] : -1;
                if (!label_ok(q.n_regions, l)) l = -1;
                ZRun v = ZRun::none();
                if (l >= 0) {
                    const float x = q.field[n * q.n_ch + ch];
                    const uint32_t w = weighted ? q.row_weight[n / q.cols] : 1u;
                    v = zonal_node(x, q.scale, w, (uint32_t)n);
                }
                if (!RUNS) {
                    if (l >= 0) zonal_add_plain(q, (size_t)l * q.n_ch + ch, v);
                    continue;
                }
                wave_runs(lane, l, v, carry_l, carry,
                          [&](int32_t r, const ZRun& u) { zonal_add(q, (size_t)r * q.n_ch + ch, u, weighted); });
            }
            if (RUNS && lane == 0 && carry_l >= 0 && carry.nodes) zonal_add(q, (size_t)carry_l * q.n_ch + ch, carry, weighted);
        }
    }
}

// the columns of one region a wave carries along its stretch, two per lane
constexpr int HCOLS = 128;

// what a wave carried for region r into the histogram: lane k holds columns k and 64 + k, so the adds are contiguous
__device__ __forceinline__ void hist_flush(const ZonalC& q, int lane, int32_t r, u64 acc0, u64 acc1) {
    if (r < 0) return;
    u64* row = q.hist + (u64)r * (u64)(q.n_bins + 2);
    if (acc0) atomicAdd(row + lane, acc0);
    if (acc1) atomicAdd(row + 64 + lane, acc1);
}

// With RUNS a wave takes a stretch of STRETCH x 64 consecutive nodes.  When a region's row of the histogram has at most HCOLS
// columns the wave carries one region, that of the first counted lane: its lanes' weights are summed per column in the wave
// and kept in the lane that owns the column, and added to the histogram when the carried region changes and after the
// stretch.  What is left (other regions, or every lane with wider rows) is peeled: the lanes that hit the first open lane's
// (region, column) are summed in the wave and added once, PEEL times, and the lanes still open add on their own.
template <bool RUNS>
__global__ void __launch_bounds__(256) zonal_hist_kernel(const ZonalC q) {
    const int64_t N = (int64_t)q.rows * q.cols;
    const int lane = threadIdx.x & 63;
    const u64 width = (u64)(q.n_bins + 2);
    const bool carrying = RUNS && width <= (u64)HCOLS;
    const int64_t per_wave = 64 * STRETCH;
    for (int64_t s0 = (blockIdx.x * (int64_t)4 + (threadIdx.x >> 6)) * per_wave; s0 < N; s0 += (int64_t)gridDim.x * 4 * per_wave) {
        u64 acc0 = 0, acc1 = 0;
        int32_t carry_l = -1;
        for (int it = 0; it < STRETCH && s0 + it * 64 < N; it++) {         // the trip count is the wave's
            const int64_t n = s0 + it * 64 + lane;
            int32_t l = n < N ? q.labels[n] : -1;
            if (!label_ok(q.n_regions, l)) l = -1;
            bool open = false;
            uint32_t col = 0;
            u64 w = 0;
            if (l >= 0) {
                const float x = q.field[n * q.n_ch + q.hist_ch];
                if (x == x) {
                    // one float64 subtraction and one float64 product
                    const double t = __dmul_rn(__dsub_rn((double)x, q.hist_lo), q.hist_inv_w);
                    col = t < 0.0 ? 0u : t >= (double)q.n_bins ? (uint32_t)q.n_bins + 1u : 1u + (uint32_t)(int)floor(t);
                    w = q.row_weight ? q.row_weight[n / q.cols] : 1u;
                    open = true;
                }
            }
            if (!RUNS) {
                if (open) atomicAdd(q.hist + (u64)l * width + col, w);
                continue;
            }
            if (carrying) {
                const u64 any = __ballot(open);
                if (any) {
                    const int32_t first_l = __shfl(l, __ffsll((long long)any) - 1);
                    if (first_l != carry_l) {
                        hist_flush(q, lane, carry_l, acc0, acc1);
                        acc0 = 0; acc1 = 0; carry_l = first_l;
                    }
                    bool mine = open && l == carry_l;
                    for (u64 m = __ballot(mine); m; m = __ballot(mine)) {
                        const uint32_t c = __shfl(col, __ffsll((long long)m) - 1);
                        const bool same = mine && col == c;
                        u64 s = same ? w : 0ull;
                        for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
                        if (lane == (int)(c & 63u)) { if (c >> 6) acc1 += s; else acc0 += s; }
                        if (same) { mine = false; open = false; }
                    }
                }
            }
            u64 key = open ? (u64)l * width + col : ~0ull;
            for (int round = 0; round < PEEL; round++) {
                const u64 left = __ballot(key != ~0ull);
                if (!left) break;
                const int first = __ffsll((long long)left) - 1;
                const u64 k = __shfl(key, first);
                const bool mine = key == k;
                u64 s = mine ? w : 0ull;
                for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
                if (lane == first) atomicAdd(q.hist + k, s);
                if (mine) key = ~0ull;
            }
            if (key != ~0ull) atomicAdd(q.hist + key, w);
        }
        if (carrying) hist_flush(q, lane, carry_l, acc0, acc1);
    }
}

__global__ void __launch_bounds__(256) zonal_finish_kernel(const ZonalC q) {
    const size_t R = (size_t)q.n_regions * (size_t)q.n_ch;
    for (size_t r = blockIdx.x * (size_t)256 + threadIdx.x; r < R; r += (size_t)gridDim.x * 256) {
        ZonalRec* o = q.out + r;
        if (!q.row_weight) { o->wcount = o->count; o->wsum = o->sum; }
        if (o->count) {
            const u64 a = q.keys[2 * r], b = q.keys[2 * r + 1];
            o->min = order_value((uint32_t)(a >> 32));
            o->min_at = (int32_t)(uint32_t)a;
            o->max = order_value((uint32_t)(b >> 32));
            o->max_at = (int32_t)~(uint32_t)b;
        }
    }
}

// ---- outlines
struct SRun {
    u64 perimeter;
    uint32_t sides_ns, sides_ew, q1, q3, qd, nodes;
    static __device__ __forceinline__ SRun none() {
        SRun v;
        v.perimeter = 0; v.sides_ns = 0; v.sides_ew = 0; v.q1 = 0; v.q3 = 0; v.qd = 0; v.nodes = 0;
        return v;
    }
    __device__ __forceinline__ void join(const SRun& u) {
        perimeter += u.perimeter; sides_ns += u.sides_ns; sides_ew += u.sides_ew; q1 += u.q1; q3 += u.q3; qd += u.qd;
        nodes += u.nodes;
    }
};
static_assert(sizeof(SRun) == 32, "8 words");

__global__ void __launch_bounds__(256) shape_init_kernel(const ShapeC q) {
    for (uint32_t r = blockIdx.x * 256u + threadIdx.x; r < q.n_regions; r += gridDim.x * 256u) {
        ShapeRec z;
        z.perimeter = 0; z.sides_ns = 0; z.sides_ew = 0; z.q1 = 0; z.q3 = 0; z.qd = 0; z.euler = 0;
        q.out[r] = z;
    }
}

// the label of node (i, j): -1 outside the lattice (a column past either end is the other end's with wrap) and for a bad entry
__device__ __forceinline__ int32_t label_at(const ShapeC& q, int32_t i, int32_t j) {
    if (i < 0 || i >= q.rows) return -1;
    if (j < 0 || j >= q.cols) {
        if (!q.wrap) return -1;
        j = j < 0 ? q.cols - 1 : 0;
    }
    const int32_t l = q.labels[(int64_t)i * q.cols + j];
    return label_ok(q.n_regions, l) ? l : -1;
}

// What node (i, j) of label l >= 0 adds to its region: its boundary sides, and of the four 2 x 2 windows it lies in those in
// which no node before it (in the order NW, NE, SW, SE) carries l, so that every (window, label) pair is counted once.
__device__ __forceinline__ SRun shape_node(const ShapeC& q, int32_t i, int32_t j, int32_t l) {
    SRun v = SRun::none();
    v.nodes = 1;
    bool m[3][3];
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) m[a][b] = (a == 1 && b == 1) || label_at(q, i + a - 1, j + b - 1) == l;
    const uint32_t ew = q.side_ew ? q.side_ew[i] : 1u;
    if (!m[0][1]) { v.sides_ns++; v.perimeter += q.side_ns ? q.side_ns[i] : 1u; }
    if (!m[2][1]) { v.sides_ns++; v.perimeter += q.side_ns ? q.side_ns[i + 1] : 1u; }
    if (!m[1][0]) { v.sides_ew++; v.perimeter += ew; }
    if (!m[1][2]) { v.sides_ew++; v.perimeter += ew; }
    for (int a = 0; a < 2; a++)
        for (int b = 0; b < 2; b++) {
            // the window whose NW node is (i + a - 1, j + b - 1); this node is its number (1 - a) * 2 + (1 - b)
            const uint32_t bits = (uint32_t)m[a][b] | (uint32_t)m[a][b + 1] << 1 | (uint32_t)m[a + 1][b] << 2 | (uint32_t)m[a + 1][b + 1] << 3;
            const int pos = (1 - a) * 2 + (1 - b);
            if (bits & ((1u << pos) - 1u)) continue;
            const int cnt = __popc(bits);
            v.q1 += cnt == 1;
            v.q3 += cnt == 3;
            v.qd += bits == 9u || bits == 6u;
        }
    return v;
}

__device__ __forceinline__ void shape_add_plain(ShapeRec* o, const SRun& v) {
    atomicAdd(&o->perimeter, v.perimeter);
    atomicAdd(&o->sides_ns, v.sides_ns);
    atomicAdd(&o->sides_ew, v.sides_ew);
    atomicAdd(&o->q1, v.q1);
    atomicAdd(&o->q3, v.q3);
    atomicAdd(&o->qd, v.qd);
}

__device__ __forceinline__ void shape_add(ShapeRec* o, const SRun& v) {
    if (v.perimeter) atomicAdd(&o->perimeter, v.perimeter);
    if (v.sides_ns) atomicAdd(&o->sides_ns, v.sides_ns);
    if (v.sides_ew) atomicAdd(&o->sides_ew, v.sides_ew);
    if (v.q1) atomicAdd(&o->q1, v.q1);
    if (v.q3) atomicAdd(&o->q3, v.q3);
    if (v.qd) atomicAdd(&o->qd, v.qd);
}

template <bool RUNS>
__global__ void __launch_bounds__(256) shape_sum_kernel(const ShapeC q) {
    const int64_t N = (int64_t)q.rows * q.cols;
    const int lane = threadIdx.x & 63;
    const int64_t per_wave = 64 * STRETCH;
    for (int64_t s0 = (blockIdx.x * (int64_t)4 + (threadIdx.x >> 6)) * per_wave; s0 < N; s0 += (int64_t)gridDim.x * 4 * per_wave) {
        SRun carry = SRun::none();
        int32_t carry_l = -1;
        for (int it = 0; it < STRETCH && s0 + it * 64 < N; it++) {         // the trip count is the wave's
            const int64_t n = s0 + it * 64 + lane;
            int32_t l = n < N ? q.labels[n] : -1;
            if (!label_ok(q.n_regions, l)) l = -1;
            SRun v = SRun::none();
            if (l >= 0) v = shape_node(q, (int32_t)(n / q.cols), (int32_t)(n % q.cols), l);
            if (!RUNS) {
                if (l >= 0) shape_add_plain(q.out + l, v);
                continue;
            }
            wave_runs(lane, l, v, carry_l, carry, [&](int32_t r, const SRun& u) { shape_add(q.out + r, u); });
        }
        if (RUNS && lane == 0 && carry_l >= 0 && carry.nodes) shape_add(q.out + carry_l, carry);
    }
}

// euler = (q1 - q3 + 2 qd) / 4 for connectivity 4, (q1 - q3 - 2 qd) / 4 for 8: exact, from 64-bit intermediates
__global__ void __launch_bounds__(256) shape_finish_kernel(const ShapeC q) {
    for (uint32_t r = blockIdx.x * 256u + threadIdx.x; r < q.n_regions; r += gridDim.x * 256u) {
        ShapeRec* o = q.out + r;
        const long long d = 2ll * (long long)o->qd;
        o->euler = (int32_t)(((long long)o->q1 - (long long)o->q3 + (q.conn8 ? -d : d)) / 4);
    }
}

}  // namespace mrtx_zn

static unsigned zonal_grid(int64_t n, int per_block) {
    const int64_t b = (n + per_block - 1) / per_block;
    return (unsigned)(b < 1 ? 1 : b > 65536 ? 65536 : b);
}

// runs: reduce runs of equal labels (and equal histogram columns) inside the wave before the atomics.  Without regions only
// the check of the table runs.
hipError_t mrtx_launch_regions_zonal(const ZonalC& q, bool runs, hipStream_t st, uint32_t* launches) {
    if (q.rows < 1 || q.cols < 1 || !q.labels || !q.bad || q.n_ch < 1 || (q.n_regions && (!q.out || !q.keys || !q.field)) ||
        (q.hist && q.n_bins < 1))
        return hipErrorInvalidValue;
    const int64_t N = (int64_t)q.rows * q.cols;
    const unsigned gn = zonal_grid(N, 256), gr = zonal_grid((int64_t)q.n_regions * q.n_ch, 256);
    uint32_t k = 1;
    hipLaunchKernelGGL(mrtx_zn::check_kernel, dim3(gn), dim3(256), 0, st, q.labels, N, q.n_regions, q.bad);
    if (q.n_regions) {
        const unsigned gs = zonal_grid(N, 256 * mrtx_zn::STRETCH);
        hipLaunchKernelGGL(mrtx_zn::zonal_init_kernel, dim3(gr), dim3(256), 0, st, q);
        if (runs) hipLaunchKernelGGL(mrtx_zn::zonal_sum_kernel<true>, dim3(gs), dim3(256), 0, st, q);
        else hipLaunchKernelGGL(mrtx_zn::zonal_sum_kernel<false>, dim3(gs), dim3(256), 0, st, q);
        k += 2;
        if (q.hist) {
            if (runs) hipLaunchKernelGGL(mrtx_zn::zonal_hist_kernel<true>, dim3(gs), dim3(256), 0, st, q);
            else hipLaunchKernelGGL(mrtx_zn::zonal_hist_kernel<false>, dim3(gs), dim3(256), 0, st, q);
            k++;
        }
        hipLaunchKernelGGL(mrtx_zn::zonal_finish_kernel, dim3(gr), dim3(256), 0, st, q);
        k++;
    }
    if (launches) *launches = k;
    return hipGetLastError();
}

hipError_t mrtx_launch_regions_shape(const ShapeC& q, bool runs, hipStream_t st, uint32_t* launches) {
    if (q.rows < 1 || q.cols < 1 || !q.labels || !q.bad || (q.n_regions && !q.out) || (!q.side_ew) != (!q.side_ns))
        return hipErrorInvalidValue;
    const int64_t N = (int64_t)q.rows * q.cols;
    const unsigned gn = zonal_grid(N, 256), gr = zonal_grid(q.n_regions, 256);
    hipLaunchKernelGGL(mrtx_zn::check_kernel, dim3(gn), dim3(256), 0, st, q.labels, N, q.n_regions, q.bad);
    if (q.n_regions) {
        const unsigned gs = zonal_grid(N, 256 * mrtx_zn::STRETCH);
        hipLaunchKernelGGL(mrtx_zn::shape_init_kernel, dim3(gr), dim3(256), 0, st, q);
        if (runs) hipLaunchKernelGGL(mrtx_zn::shape_sum_kernel<true>, dim3(gs), dim3(256), 0, st, q);
        else hipLaunchKernelGGL(mrtx_zn::shape_sum_kernel<false>, dim3(gs), dim3(256), 0, st, q);
        hipLaunchKernelGGL(mrtx_zn::shape_finish_kernel, dim3(gr), dim3(256), 0, st, q);
    }
    if (launches) *launches = q.n_regions ? 4 : 1;
    return hipGetLastError();
}
