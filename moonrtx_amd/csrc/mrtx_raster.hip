// mrtx_raster.hip -- the kernels of the polygon rasterisation (mrtx_rasterise; DESIGN.md sections 3.29, 4.38): rings of (y, x)
// vertices burnt into a label table and one cover record per polygon.  Integers only: the one division is that of two int64.
//
// bins (default): the crossings of every edge with the columns' centre lines are counted per bin (a polygon x a strip of 64
// columns), the counts scanned, and the crossings written bin by bin as (first row, column, sign).  One wave per bin and chunk
// of 64 rows then gathers its lanes' crossings through LDS, one lane per column, and walks the rows down.  brute
// (MOONRT_RASTER=brute): every node tests every edge, the rings grouped by polygon; the same arithmetic and the same bytes.
#include "mrtx_raster.h"

#include "mrtx_lattice_dev.h"

namespace mrtx_rs {

using u64 = unsigned long long;
using mrtx_lat::xor64;

__device__ __forceinline__ u64 wave_sum(u64 v) {
    for (int m = 32; m; m >>= 1) v += xor64(v, m);
    return v;
}
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
    for (int m = 32; m; m >>= 1) v = min(v, (uint32_t)__shfl_xor(v, m));
    return v;
}
__device__ __forceinline__ int32_t wave_max(int32_t v) {
    for (int m = 32; m; m >>= 1) v = max(v, __shfl_xor(v, m));
    return v;
}

// ---- the rule's arithmetic, in doubled units ---------------------------------------------------------
struct Edge {
    long long Y0, X0, Y1, X1;
};

// edge k of a ring that passed the check: from vertex k to vertex k + 1, the last one to the first vertex wind times round
__device__ __forceinline__ Edge ring_edge(const RasterC& q, const RasterRing& g, uint32_t k) {
    const int32_t* a = q.vertices + 2 * (g.first + k);
    Edge e;
    e.Y0 = 2 * (long long)a[0];
    e.X0 = 2 * (long long)a[1];
    if (k + 1 < g.n_vertices) {
        e.Y1 = 2 * (long long)a[2];
        e.X1 = 2 * (long long)a[3];
    } else {
        const int32_t* f = q.vertices + 2 * g.first;
        e.Y1 = 2 * (long long)f[0];
        e.X1 = 2 * ((long long)f[1] + (long long)g.wind * ((long long)q.cols << q.s));
    }
    return e;
}

// the unwrapped columns ju with min(X0, X1) <= (2 ju + 1) S < max(X0, X1): *lo .. *hi, false when there is none
__device__ __forceinline__ bool edge_span(const Edge& e, int s, long long* lo, long long* hi) {
    const long long S = 1ll << s, mn = e.X0 < e.X1 ? e.X0 : e.X1, mx = e.X0 < e.X1 ? e.X1 : e.X0;
    *lo = (mn + S - 1) >> (s + 1);              // ceil((mn - S) / 2 S)
    *hi = ((mx + S - 1) >> (s + 1)) - 1;
    return *hi >= *lo;
}

// the span clipped to the lattice without wrap
__device__ __forceinline__ bool edge_columns(const RasterC& q, const Edge& e, long long* lo, long long* hi) {
    if (!edge_span(e, q.s, lo, hi)) return false;
    if (!q.wrap) {
        if (*lo < 0) *lo = 0;
        if (*hi > q.cols - 1) *hi = q.cols - 1;
    }
    return *hi >= *lo;
}

// the first row a crossing of column ju counts for, not yet clipped: ceil((y* - S) / 2 S), y* = Y0 + (xc - X0)(Y1 - Y0) / (X1 - X0)
__device__ __forceinline__ long long first_row(const Edge& e, long long ju, int s) {
    const long long S = 1ll << s, xc = (2 * ju + 1) * S;
    long long den = e.X1 - e.X0, num = (xc - e.X0) * (e.Y1 - e.Y0);
    if (den < 0) { den = -den; num = -num; }
    const long long A = (e.Y0 - S) * den + num, B = 2 * S * den;
    long long d = A / B;                        // towards zero
    if (A % B > 0) d++;
    return d;
}

// the ring of edge e: the last one whose first edge is at or before e (every ring has an edge)
__device__ __forceinline__ uint32_t ring_of(const RasterC& q, uint32_t e) {
    u64 lo = 0, hi = q.n_rings;
    while (hi - lo > 1) {
        const u64 mid = (lo + hi) >> 1;
        if (q.edge_off[mid] <= e) lo = mid;
        else hi = mid;
    }
    return (uint32_t)lo;
}

// ---- the check of the caller's tables ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) check_kernel(const RasterC q) {
    const u64 n = blockIdx.x * 256ull + threadIdx.x;
    if (n < q.n_rings) {
        const RasterRing g = q.rings[n];
        bool ok = g.polygon >= 0 && (uint32_t)g.polygon < q.n_polygons && g.n_vertices >= 1 && g.first <= q.n_vertices &&
                  g.n_vertices <= q.n_vertices - g.first && g.reserved == 0 && (q.wrap ? g.wind >= -1 && g.wind <= 1 : g.wind == 0);
        if (ok && g.wind != 0) {                // the closing point, one turn on, stays within twice the coordinates' range
            const long long x = (long long)q.vertices[2 * g.first + 1] + (long long)g.wind * ((long long)q.cols << q.s);
            ok = x >= -2ll * MRTX_RS_CMAX && x <= 2ll * MRTX_RS_CMAX;
        }
        q.edge_off[n] = ok ? g.n_vertices : 0u;
        if (ok && !q.bins) atomicAdd(&q.poly_off[g.polygon], 1u);
        if (!ok) atomicAdd(&q.head[RS_BAD_RINGS], 1ull);
    }
    if (n < 2 * q.n_vertices) {
        const int32_t v = q.vertices[n];
        if (v < -MRTX_RS_CMAX || v > MRTX_RS_CMAX) atomicAdd(&q.head[RS_BAD_COORDS], 1ull);
    }
}

// ---- the exclusive scan of a table of n uint32 in place, its sum in 64 bits -------------------------------------------------
__global__ void __launch_bounds__(256) chunk_sum_kernel(const uint32_t* a, u64 n, u64* sums) {
    __shared__ u64 sh[4];
    const u64 at = (u64)blockIdx.x * MRTX_RS_CHUNK + 8 * threadIdx.x;
    u64 v = 0;
    for (int k = 0; k < 8; k++)
        if (at + k < n) v += a[at + k];
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) sums[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

// one block: every thread a run of the chunk sums
__global__ void __launch_bounds__(256) scan_sums_kernel(u64* sums, uint32_t chunks, u64* total) {
    __shared__ u64 sh[256];
    const uint32_t per = (chunks + 255) / 256, from = min(chunks, threadIdx.x * per), to = min(chunks, from + per);
    u64 v = 0;
    for (uint32_t k = from; k < to; k++) v += sums[k];
    sh[threadIdx.x] = v;
    __syncthreads();
    u64 base = 0;
    for (uint32_t k = 0; k < threadIdx.x; k++) base += sh[k];
    for (uint32_t k = from; k < to; k++) {
        const u64 s = sums[k];
        sums[k] = base;
        base += s;
    }
    if (threadIdx.x == 255) *total = base;
}

__global__ void __launch_bounds__(256) chunk_scan_kernel(uint32_t* a, u64 n, const u64* sums) {
    __shared__ uint2 sh[4];
    const u64 at = (u64)blockIdx.x * MRTX_RS_CHUNK + 8 * threadIdx.x;
    uint32_t v[8], mine = 0;
    for (int k = 0; k < 8; k++) {
        v[k] = at + k < n ? a[at + k] : 0u;
        mine += v[k];
    }
    uint2 tot;
    uint32_t run = (uint32_t)sums[blockIdx.x] + mrtx_lat::block_scan(make_uint2(mine, 0), sh, &tot).x;
    for (int k = 0; k < 8; k++) {
        if (at + k < n) a[at + k] = run;
        run += v[k];
    }
}

// ---- the crossings of all edges -------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) count_kernel(const RasterC q) {
    const u64 e = blockIdx.x * 256ull + threadIdx.x;
    u64 mine = 0;
    if (e < q.n_edges) {
        const uint32_t r = ring_of(q, (uint32_t)e);
        const RasterRing g = q.rings[r];
        const Edge ed = ring_edge(q, g, (uint32_t)e - q.edge_off[r]);
        long long lo, hi;
        if (edge_columns(q, ed, &lo, &hi)) mine = (u64)(hi - lo + 1);
    }
    mine = wave_sum(mine);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&q.head[RS_CROSSINGS], mine);
}

// One lane per edge, column after column of its span.  !FILL: a count per bin; FILL: the crossing into the bin's next free slot.
// The order inside a bin is that of the atomics: only integer sums are taken over it.
template <bool FILL>
__global__ void __launch_bounds__(256) bin_kernel(const RasterC q, uint32_t n_cross) {
    const u64 e = blockIdx.x * 256ull + threadIdx.x;
    if (e >= q.n_edges) return;
    const uint32_t r = ring_of(q, (uint32_t)e);
    const RasterRing g = q.rings[r];
    const Edge ed = ring_edge(q, g, (uint32_t)e - q.edge_off[r]);
    long long lo, hi;
    if (!edge_columns(q, ed, &lo, &hi)) return;
    long long j = lo % q.cols;
    if (j < 0) j += q.cols;
    const uint32_t bin0 = (uint32_t)g.polygon * (uint32_t)q.strips, neg = ed.X1 < ed.X0 ? 64u : 0u;
    for (long long ju = lo; ju <= hi; ju++) {
        const uint32_t bin = bin0 + ((uint32_t)j >> MRTX_RS_STRIP_SHIFT);
        if (FILL) {
            long long i0 = first_row(ed, ju, q.s);
            i0 = i0 < 0 ? 0 : i0 > q.rows ? q.rows : i0;
            const uint32_t slot = atomicAdd(&q.bin_off[bin], 1u);
            if (slot < n_cross) q.cross[slot] = make_uint2((uint32_t)i0, ((uint32_t)j & 63u) | neg);
        } else {
            atomicAdd(&q.bin_off[bin], 1u);
        }
        if (++j == q.cols) j = 0;
    }
}

// ---- the outputs ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) init_kernel(const RasterC q) {
    const u64 n = blockIdx.x * 256ull + threadIdx.x;
    if (n < (u64)q.rows * (u64)q.cols) q.labels[n] = q.last ? -1 : INT32_MAX;
    if (n < q.n_polygons) {
        CoverRec c;
        c.weight = c.owned_weight = 0;
        c.count = c.owned = 0;
        c.i_min = c.i_max = c.first_at = -1;
        c.reserved = 0;
        q.cover[n] = c;
    }
}

// what one wave found of polygon p, every lane taking part: the covered lanes' sums and extremes into the polygon's record
__device__ __forceinline__ void cover_add(const RasterC& q, int32_t p, bool cov, uint32_t cnt, u64 wt, uint32_t i_min, int32_t i_max,
                                          uint32_t first_at) {
    cnt = (uint32_t)wave_sum(cov ? cnt : 0u);
    if (!cnt) return;
    wt = wave_sum(cov ? wt : 0ull);
    i_min = wave_min(cov ? i_min : UINT32_MAX);
    i_max = wave_max(cov ? i_max : -1);
    first_at = wave_min(cov ? first_at : UINT32_MAX);
    if ((threadIdx.x & 63) == 0) {
        CoverRec* c = q.cover + p;
        atomicAdd(&c->weight, wt);
        atomicAdd(&c->count, cnt);
        atomicMin(reinterpret_cast<uint32_t*>(&c->i_min), i_min);       // -1 is the greatest unsigned
        atomicMax(&c->i_max, i_max);
        atomicMin(reinterpret_cast<uint32_t*>(&c->first_at), first_at);
    }
}

// One wave per bin and chunk of MRTX_RS_ROWS rows, lane = column of the strip.  The bin's crossings pass through LDS
// MRTX_RS_STAGE at a time; a lane keeps those of its own column: the ones above the chunk as the winding it enters with, the
// ones inside as steps in its column of `step`, which no other lane touches.
__global__ void __launch_bounds__(64) cover_kernel(const RasterC q, uint32_t n_cross, u64 n_work, uint32_t row_chunks) {
    __shared__ int32_t step[MRTX_RS_ROWS][64];
    __shared__ uint2 stage[MRTX_RS_STAGE];
    const uint32_t lane = threadIdx.x;
    for (u64 w = blockIdx.x; w < n_work; w += gridDim.x) {
        const uint32_t bin = (uint32_t)(w / row_chunks), rc = (uint32_t)(w % row_chunks);
        const uint32_t from = bin ? min(q.bin_off[bin - 1], n_cross) : 0u, to = min(q.bin_off[bin], n_cross);
        if (from >= to) continue;
        const int32_t p = (int32_t)(bin / (uint32_t)q.strips);
        const int32_t j = (int32_t)((bin % (uint32_t)q.strips) << MRTX_RS_STRIP_SHIFT) + (int32_t)lane;
        const uint32_t r0 = rc * MRTX_RS_ROWS, r1 = min((uint32_t)q.rows, r0 + MRTX_RS_ROWS);
        for (uint32_t r = 0; r < MRTX_RS_ROWS; r++) step[r][lane] = 0;
        int32_t wind = 0;
        for (uint32_t base = from; base < to; base += MRTX_RS_STAGE) {
            const uint32_t n = min((uint32_t)MRTX_RS_STAGE, to - base);
            __syncthreads();
            if (lane < n) stage[lane] = q.cross[base + lane];
            __syncthreads();
            for (uint32_t k = 0; k < n; k++) {
                const uint2 x = stage[k];
                if ((x.y & 63u) != lane) continue;
                const int32_t sg = (x.y & 64u) ? -1 : 1;
                if (x.x < r0) wind += sg;
                else if (x.x < r1) step[x.x - r0][lane] += sg;
            }
        }
        uint32_t cnt = 0, i_min = UINT32_MAX, first_at = UINT32_MAX;
        int32_t i_max = -1;
        u64 wt = 0;
        if (j < q.cols) {
            for (uint32_t r = r0; r < r1; r++) {
                wind += step[r - r0][lane];
                if (q.evenodd ? (wind & 1) : (wind != 0)) {
                    const uint32_t v = r * (uint32_t)q.cols + (uint32_t)j;
                    if (q.last) atomicMax(&q.labels[v], p);
                    else atomicMin(&q.labels[v], p);
                    if (!cnt) { i_min = r; first_at = v; }
                    cnt++;
                    i_max = (int32_t)r;
                    wt += q.row_weight ? q.row_weight[r] : 1u;
                }
            }
        }
        cover_add(q, p, cnt != 0, cnt, wt, i_min, i_max, first_at);
    }
}

// brute: one lane per node, every ring in the order of the polygons, every edge of it
__global__ void __launch_bounds__(256) brute_kernel(const RasterC q) {
    const u64 N = (u64)q.rows * (u64)q.cols, v = blockIdx.x * 256ull + threadIdx.x;
    const bool valid = v < N;
    const long long i = valid ? (long long)(v / (u64)q.cols) : 0, j = valid ? (long long)(v % (u64)q.cols) : 0;
    const u64 rw = q.row_weight ? q.row_weight[i] : 1u;
    int32_t label = -1, cur = -1, wind = 0;
    for (u64 k = 0; k <= q.n_rings; k++) {
        const bool end = k == q.n_rings;
        RasterRing g = {};
        if (!end) g = q.rings[q.order[k]];
        if (end || g.polygon != cur) {
            if (cur >= 0) {
                const bool cov = valid && (q.evenodd ? (wind & 1) : (wind != 0));
                if (cov && (q.last || label < 0)) label = cur;
                cover_add(q, cur, cov, 1u, rw, (uint32_t)i, (int32_t)i, (uint32_t)v);
            }
            if (end) break;
            cur = g.polygon;
            wind = 0;
        }
        for (uint32_t e = 0; e < g.n_vertices; e++) {
            const Edge ed = ring_edge(q, g, e);
            long long lo, hi;
            if (!edge_columns(q, ed, &lo, &hi)) continue;
            const int32_t sg = ed.X1 > ed.X0 ? 1 : -1;
            if (!q.wrap) {
                if (j >= lo && j <= hi && first_row(ed, j, q.s) <= i) wind += sg;
            } else {
                // the columns j + m cols of the span: m from ceil((lo - j) / cols) on
                long long d = lo - j, m = d / q.cols;
                if (d % q.cols > 0) m++;
                for (long long ju = j + m * q.cols; ju <= hi; ju += q.cols)
                    if (first_row(ed, ju, q.s) <= i) wind += sg;
            }
        }
    }
    if (valid) q.labels[v] = label;
}

// brute: the rings grouped by polygon, each into the next free slot of its polygon
__global__ void __launch_bounds__(256) order_kernel(const RasterC q) {
    const u64 n = blockIdx.x * 256ull + threadIdx.x;
    if (n >= q.n_rings) return;
    const uint32_t slot = atomicAdd(&q.poly_off[q.rings[n].polygon], 1u);
    if (slot < q.n_rings) q.order[slot] = (uint32_t)n;
}

// the label table's last pass: a node that no polygon reached gets -1, every other one counts for the polygon that owns it
__global__ void __launch_bounds__(256) owned_kernel(const RasterC q) {
    const u64 N = (u64)q.rows * (u64)q.cols, v = blockIdx.x * 256ull + threadIdx.x;
    int32_t l = -1;
    u64 wt = 0;
    if (v < N) {
        l = q.labels[v];
        if (l == INT32_MAX) {
            l = -1;
            q.labels[v] = -1;
        }
        wt = q.row_weight ? q.row_weight[v / (u64)q.cols] : 1u;
    }
    const bool has = l >= 0;
    const u64 mask = __ballot(has);
    if (!mask) return;
    const int first = __ffsll((long long)mask) - 1;
    const int32_t l0 = __shfl(l, first);
    if (__ballot(has && l != l0) == 0) {        // one owner in the wave: one pair of atomics
        const u64 sum = wave_sum(has ? wt : 0ull);
        if ((int)(threadIdx.x & 63) == first) {
            atomicAdd(&q.cover[l0].owned, (uint32_t)__popcll(mask));
            atomicAdd(&q.cover[l0].owned_weight, sum);
        }
    } else if (has) {
        atomicAdd(&q.cover[l].owned, 1u);
        atomicAdd(&q.cover[l].owned_weight, wt);
    }
}

static uint32_t grid_for(u64 n, u64 per) { return (uint32_t)(n ? (n + per - 1) / per : 1); }

// the scan of a[0 .. n) in place, the sum to *total: three launches
static void scan(uint32_t* a, u64 n, u64* sums, u64* total, hipStream_t st, uint32_t* launches) {
    const uint32_t chunks = (uint32_t)raster_chunks(n);
    hipLaunchKernelGGL(chunk_sum_kernel, dim3(grid_for(n, MRTX_RS_CHUNK)), dim3(256), 0, st, a, n, sums);
    hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(256), 0, st, sums, chunks, total);
    hipLaunchKernelGGL(chunk_scan_kernel, dim3(grid_for(n, MRTX_RS_CHUNK)), dim3(256), 0, st, a, n, sums);
    if (launches) *launches += 3;
}

}  // namespace mrtx_rs

hipError_t mrtx_launch_raster_check(const RasterC& q, hipStream_t st, uint32_t* launches) {
    using namespace mrtx_rs;
    const u64 n = q.n_rings > 2 * q.n_vertices ? q.n_rings : 2 * q.n_vertices;
    hipLaunchKernelGGL(check_kernel, dim3(grid_for(n, 256)), dim3(256), 0, st, q);
    if (launches) *launches += 1;
    scan(q.edge_off, q.n_rings, q.sums, q.head + RS_EDGES, st, launches);
    return hipGetLastError();
}

hipError_t mrtx_launch_raster_count(const RasterC& q, hipStream_t st, uint32_t* launches) {
    using namespace mrtx_rs;
    hipLaunchKernelGGL(count_kernel, dim3(grid_for(q.n_edges, 256)), dim3(256), 0, st, q);
    if (launches) *launches += 1;
    return hipGetLastError();
}

hipError_t mrtx_launch_raster_cover(const RasterC& q, hipStream_t st, uint32_t* launches) {
    using namespace mrtx_rs;
    const u64 N = (u64)q.rows * (u64)q.cols;
    const u64 n_init = N > q.n_polygons ? N : q.n_polygons;
    if (q.bins) {
        const uint32_t C = q.n_cross;
        hipLaunchKernelGGL(bin_kernel<false>, dim3(grid_for(q.n_edges, 256)), dim3(256), 0, st, q, C);
        scan(q.bin_off, q.n_bins, q.sums, q.head + RS_BINNED, st, launches);
        hipLaunchKernelGGL(bin_kernel<true>, dim3(grid_for(q.n_edges, 256)), dim3(256), 0, st, q, C);
        hipLaunchKernelGGL(init_kernel, dim3(grid_for(n_init, 256)), dim3(256), 0, st, q);
        const uint32_t row_chunks = (uint32_t)((q.rows + MRTX_RS_ROWS - 1) / MRTX_RS_ROWS);
        const u64 n_work = (u64)q.n_bins * row_chunks;
        hipLaunchKernelGGL(cover_kernel, dim3((uint32_t)(n_work < ((u64)1 << 22) ? (n_work ? n_work : 1) : (u64)1 << 22)), dim3(64), 0, st,
                           q, C, n_work, row_chunks);
        if (launches) *launches += 4;
    } else {
        scan(q.poly_off, q.n_polygons, q.sums, q.head + RS_BINNED, st, launches);
        hipLaunchKernelGGL(order_kernel, dim3(grid_for(q.n_rings, 256)), dim3(256), 0, st, q);
        hipLaunchKernelGGL(init_kernel, dim3(grid_for(n_init, 256)), dim3(256), 0, st, q);
        hipLaunchKernelGGL(brute_kernel, dim3(grid_for(N, 256)), dim3(256), 0, st, q);
        if (launches) *launches += 3;
    }
    hipLaunchKernelGGL(owned_kernel, dim3(grid_for(N, 256)), dim3(256), 0, st, q);
    if (launches) *launches += 1;
    return hipGetLastError();
}
