// mrtx_relief.hip -- gfx950 kernels of the terrain relief stage (mrtx_relief, mrtx_relief_share; DESIGN.md sections 3.14, 4.15).
//
// Per node of a window of the DEM's texel lattice: the least-squares plane through the (2 ri + 1) x (2 rj + 1) lattice nodes
// around it, and the residual about that plane.  The sums are float64 left folds in a fixed order (rows of the footprint
// first, then down its columns), so a sliding window is not allowed; what the kernels share between nodes is the row pass:
//   relief_tile_kernel<TH, TW>  one 256-lane workgroup per tile of TH x TW nodes: the tile's D and its halo of ri rows and rj
//                               columns staged in LDS, the row sums r0, r1, r2 of every staged row at the tile's TW columns
//                               into LDS (each is shared by the 2 ri + 1 nodes above and below it), then one lane per node
//                               folds its column of row sums and writes the float4
//   relief_direct_kernel        one lane per node, the footprint read straight from global memory: the yardstick the
//                               staged kernel is measured against (tools/relief_bench.py), and the same bits
// and the safe share of a landing ellipse, integer box sums of a predicate through a summed-area table:
//   share_rows_kernel           one workgroup per row: the predicate's inclusive prefix sums along the row
//   share_cols_kernel           one lane per column: the running sum down the rows
//   share_box_kernel            one lane per node: its box from at most eight table entries, safe / total
// Own translation unit: the existing kernels are compiled exactly as before.  Build flags as there (-ffp-contract=off,
// correctly rounded sqrtf): the device does float64 + and *, float32 sqrtf and *, and casts.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mrtx_device.h"

namespace mrtx_rl {

// D of the texel in DEM row r (inside [0, dem_h)) at lattice column node_col counted from the window's column 0 (it may be
// negative); the column wraps modulo W; 64-bit element offsets
__device__ __forceinline__ float texel_D(const ReliefC& q, int64_t r, int64_t node_col) {
    int64_t c = ((int64_t)q.col0 + node_col * q.stride) % q.dem_w;
    if (c < 0) c += q.dem_w;
    const uint64_t e = (uint64_t)(r + 2) * (uint64_t)q.dem_pitch + (uint64_t)(c + 2);
    return q.dem[e * (MRTX_DEM_ELEM_BYTES / 4)];
}

// does the footprint of window row i stay inside the DEM's rows?
__device__ __forceinline__ bool rows_inside(const ReliefC& q, int64_t i) {
    return (int64_t)q.row0 + (i - q.ri) * q.stride >= 0 && (int64_t)q.row0 + (i + q.ri) * q.stride < q.dem_h;
}

// the plane, the residual and the metric gradients of node (i, j) from its four sums (section 3.14, operation by operation)
__device__ __forceinline__ void finish_node(const ReliefC& q, int64_t i, int64_t j, double S0, double Sj, double Si, double S2) {
    const double c = S0 * q.inv_n, aj = Sj * q.inv_xj, ai = Si * q.inv_xi;
    const double E = fmax(((S2 - c * S0) - aj * Sj) - ai * Si, 0.0);
    const double ge = aj * q.scale[2 * i], gn = -(ai * q.scale[2 * i + 1]);
    float4 o;
    o.x = sqrtf((float)(ge * ge + gn * gn));
    o.y = sqrtf((float)(E * q.inv_n)) * q.rm;
    o.z = (float)ge;
    o.w = (float)gn;
    q.out[i * q.cols + j] = o;
}

__device__ __forceinline__ void nan_node(const ReliefC& q, int64_t i, int64_t j) {
    const float n = __builtin_nanf("");
    q.out[i * q.cols + j] = make_float4(n, n, n, n);
}

template <int TH, int TW>
__global__ void __launch_bounds__(256) relief_tile_kernel(const ReliefC q) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int ri = q.ri, rj = q.rj;
    const int64_t ty = blockIdx.x / (unsigned)q.tiles_x, tx = blockIdx.x % (unsigned)q.tiles_x;
    const int64_t i0 = ty * TH, j0 = tx * TW;
    const int th = (int)min((int64_t)TH, q.rows - i0), tw = (int)min((int64_t)TW, q.cols - j0);
    const int hh = th + 2 * ri, hw = tw + 2 * rj;       // the staged rows and columns: the tile's nodes and their halo
    const int dp = hw | 1;                              // pitch of the staged D (odd: rows start on different banks)
    double* s0 = reinterpret_cast<double*>(smem);       // the row sums, hh x TW each
    double* s1 = s0 + (TH + 2 * ri) * TW;
    double* s2 = s1 + (TH + 2 * ri) * TW;
    float* sD = reinterpret_cast<float*>(s2 + (TH + 2 * ri) * TW);
    const int lane = threadIdx.x;

    // stage D: staged row a = lattice row i0 + a - ri, staged column b = lattice column j0 + b - rj; rows outside the DEM
    // are not read (the nodes that would use them are NaN)
    for (int p = lane; p < hh * hw; p += 256) {
        const int a = p / hw, b = p % hw;
        const int64_t r = (int64_t)q.row0 + (i0 + a - ri) * q.stride;
        float D = 1.0f;
        if (r >= 0 && r < q.dem_h) D = texel_D(q, r, j0 + b - rj);
        sD[a * dp + b] = D;
    }
    __syncthreads();
    // the row pass: for staged row a and tile column b, the folds over dj = -rj .. rj ascending, from their first term
    for (int p = lane; p < hh * tw; p += 256) {
        const int a = p / tw, b = p % tw;
        const float* row = sD + a * dp + b;             // row[k] = the node at dj = k - rj
        double z = (double)row[0] - 1.0;
        double r0 = z, r1 = (double)(-rj) * z, r2 = z * z;
        for (int k = 1; k <= 2 * rj; k++) {
            z = (double)row[k] - 1.0;
            r0 = r0 + z;
            r1 = r1 + (double)(k - rj) * z;
            r2 = r2 + z * z;
        }
        s0[a * TW + b] = r0; s1[a * TW + b] = r1; s2[a * TW + b] = r2;
    }
    __syncthreads();
    // the column pass: one lane per node, the folds over di = -ri .. ri ascending
    unsigned long long valid = 0;
    for (int p = lane; p < th * tw; p += 256) {
        const int a = p / tw, b = p % tw;
        const int64_t i = i0 + a, j = j0 + b;
        if (!rows_inside(q, i)) { nan_node(q, i, j); continue; }
        const int o = a * TW + b;                       // the row sums of di = -ri
        double S0 = s0[o], Sj = s1[o], Si = (double)(-ri) * s0[o], S2 = s2[o];
        for (int k = 1; k <= 2 * ri; k++) {
            const double r0 = s0[o + k * TW];
            S0 = S0 + r0;
            Sj = Sj + s1[o + k * TW];
            Si = Si + (double)(k - ri) * r0;
            S2 = S2 + s2[o + k * TW];
        }
        finish_node(q, i, j, S0, Sj, Si, S2);
        valid++;
    }
    if (q.fetches && valid) atomicAdd(q.fetches, valid * (unsigned long long)((2 * ri + 1) * (2 * rj + 1)));
}

__global__ void __launch_bounds__(256) relief_direct_kernel(const ReliefC q) {
    const int64_t n_nodes = (int64_t)q.rows * q.cols;
    const int ri = q.ri, rj = q.rj;
    unsigned long long valid = 0;
    for (int64_t n = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; n < n_nodes; n += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = n / q.cols, j = n % q.cols;
        if (!rows_inside(q, i)) { nan_node(q, i, j); continue; }
        double S0 = 0.0, Sj = 0.0, Si = 0.0, S2 = 0.0;
        for (int di = -ri; di <= ri; di++) {
            const int64_t r = (int64_t)q.row0 + (i + di) * q.stride;
            double z = (double)texel_D(q, r, j - rj) - 1.0;
            double r0 = z, r1 = (double)(-rj) * z, r2 = z * z;
            for (int dj = -rj + 1; dj <= rj; dj++) {
                z = (double)texel_D(q, r, j + dj) - 1.0;
                r0 = r0 + z;
                r1 = r1 + (double)dj * z;
                r2 = r2 + z * z;
            }
            if (di == -ri) {
                S0 = r0; Sj = r1; Si = (double)di * r0; S2 = r2;
            } else {
                S0 = S0 + r0; Sj = Sj + r1; Si = Si + (double)di * r0; S2 = S2 + r2;
            }
        }
        finish_node(q, i, j, S0, Sj, Si, S2);
        valid++;
    }
    if (q.fetches && valid) atomicAdd(q.fetches, valid * (unsigned long long)((2 * ri + 1) * (2 * rj + 1)));
}

// ---- the safe share of a landing ellipse
// a NaN fails both comparisons: unsafe
__device__ __forceinline__ uint32_t safe_node(const ShareC& q, int64_t n) {
    const float4 v = q.relief[n];
    return (v.x <= q.gmax && v.y <= q.smax) ? 1u : 0u;
}

// one workgroup per row (grid-stride over the rows): inclusive prefix sums of the predicate along the row, 256 columns at a
// time with a carry
__global__ void __launch_bounds__(256) share_rows_kernel(const ShareC q) {
    __shared__ uint32_t s[256];
    const int lane = threadIdx.x;
    for (int64_t i = blockIdx.x; i < q.rows; i += gridDim.x) {
        uint32_t carry = 0;
        for (int64_t j0 = 0; j0 < q.cols; j0 += 256) {
            const int64_t j = j0 + lane;
            uint32_t v = j < q.cols ? safe_node(q, i * q.cols + j) : 0u;
            s[lane] = v;
            __syncthreads();
            for (int d = 1; d < 256; d <<= 1) {
                const uint32_t u = lane >= d ? s[lane - d] : 0u;
                __syncthreads();
                v += u;
                s[lane] = v;
                __syncthreads();
            }
            if (j < q.cols) q.sat[i * q.cols + j] = carry + v;
            carry += s[255];
            __syncthreads();
        }
    }
}

// one lane per column: the running sum down the rows turns the row prefixes into the summed-area table
__global__ void __launch_bounds__(256) share_cols_kernel(const ShareC q) {
    for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < q.cols; j += (int64_t)gridDim.x * blockDim.x) {
        uint32_t run = 0;
        for (int64_t i = 0; i < q.rows; i++) {
            run += q.sat[i * q.cols + j];
            q.sat[i * q.cols + j] = run;
        }
    }
}

// safe nodes in rows [a0, a1] x columns [b0, b1] (all inside the map) from the table; uint32 arithmetic is exact modulo 2^32
__device__ __forceinline__ uint32_t box_count(const ShareC& q, int64_t a0, int64_t a1, int64_t b0, int64_t b1) {
    const uint32_t A = q.sat[a1 * q.cols + b1];
    const uint32_t B = a0 > 0 ? q.sat[(a0 - 1) * q.cols + b1] : 0u;
    const uint32_t C = b0 > 0 ? q.sat[a1 * q.cols + b0 - 1] : 0u;
    const uint32_t D = a0 > 0 && b0 > 0 ? q.sat[(a0 - 1) * q.cols + b0 - 1] : 0u;
    return (A - B) - (C - D);
}

__global__ void __launch_bounds__(256) share_box_kernel(const ShareC q) {
    const int64_t n_nodes = (int64_t)q.rows * q.cols;
    for (int64_t n = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; n < n_nodes; n += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = n / q.cols, j = n % q.cols;
        const int64_t a0 = max(i - q.Ri, (int64_t)0), a1 = min(i + q.Ri, (int64_t)q.rows - 1);
        int64_t b0 = j - q.Rj, b1 = j + q.Rj;
        uint32_t safe, width;
        if (q.wrap && 2 * (int64_t)q.Rj + 1 >= q.cols) {        // the box goes round the circle: every column once
            safe = box_count(q, a0, a1, 0, q.cols - 1);
            width = (uint32_t)q.cols;
        } else if (q.wrap && (b0 < 0 || b1 >= q.cols)) {        // the box crosses the seam: two pieces
            if (b0 < 0) { b0 += q.cols; } else { b1 -= q.cols; }        // now b1 < b0: columns [b0, cols) and [0, b1]
            safe = box_count(q, a0, a1, b0, q.cols - 1) + box_count(q, a0, a1, 0, b1);
            width = (uint32_t)(2 * q.Rj + 1);
        } else {
            b0 = max(b0, (int64_t)0); b1 = min(b1, (int64_t)q.cols - 1);
            safe = box_count(q, a0, a1, b0, b1);
            width = (uint32_t)(b1 - b0 + 1);
        }
        const uint32_t total = (uint32_t)(a1 - a0 + 1) * width;
        q.out[n] = (float)safe / (float)total;
    }
}

}  // namespace mrtx_rl

static unsigned relief_grid(int64_t n, int per_block) {
    const int64_t b = (n + per_block - 1) / per_block;
    return (unsigned)(b < 1 ? 1 : b > 65536 ? 65536 : b);
}

// LDS bytes of relief_tile_kernel<TH, TW> at a footprint: the three tables of row sums and the staged D
size_t mrtx_relief_tile_lds(int th, int tw, int ri, int rj) {
    const size_t hh = (size_t)th + 2 * (size_t)ri, dp = ((size_t)tw + 2 * (size_t)rj) | 1;
    return 3 * sizeof(double) * hh * (size_t)tw + sizeof(float) * hh * dp;
}

template <int TH, int TW>
static hipError_t launch_relief_tile(ReliefC q, hipStream_t st) {
    const size_t lds = mrtx_relief_tile_lds(TH, TW, q.ri, q.rj);
    const int64_t tiles_x = ((int64_t)q.cols + TW - 1) / TW, tiles_y = ((int64_t)q.rows + TH - 1) / TH;
    if (lds > 160 * 1024 || tiles_x * tiles_y > 0x7FFFFFFFll) return hipErrorInvalidValue;
    q.tiles_x = (int32_t)tiles_x;
    hipError_t e = hipSuccess;
    if (lds > 64 * 1024)        // above the default limit of a workgroup: ask for the CU's whole LDS
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(&mrtx_rl::relief_tile_kernel<TH, TW>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e == hipSuccess) {
        hipLaunchKernelGGL((mrtx_rl::relief_tile_kernel<TH, TW>), dim3((unsigned)(tiles_x * tiles_y)), dim3(256), lds, st, q);
        e = hipGetLastError();
    }
    // a runtime that does not grant a workgroup that much LDS refuses the launch at once: the 16 x 16 shape (at most 55.3 KB)
    // gives the same bits
    if (e != hipSuccess && lds > 64 * 1024 && (TH != 16 || TW != 16)) return launch_relief_tile<16, 16>(q, st);
    return e;
}

// tile: 0 = the direct kernel; 16 = 16 x 16 nodes, 32 = 32 x 32, 64 = 64 rows x 16 columns per workgroup
hipError_t mrtx_launch_relief(const ReliefC& q, int tile, hipStream_t st) {
    if (q.rows < 1 || q.cols < 1 || q.ri < 1 || q.rj < 1 || q.ri > 32 || q.rj > 32 || !q.dem || !q.scale || !q.out)
        return hipErrorInvalidValue;
    switch (tile) {
        case 0: {
            const int64_t n = (int64_t)q.rows * q.cols;
            hipLaunchKernelGGL(mrtx_rl::relief_direct_kernel, dim3(relief_grid(n, 256)), dim3(256), 0, st, q);
            return hipGetLastError();
        }
        case 16: return launch_relief_tile<16, 16>(q, st);
        case 32: return launch_relief_tile<32, 32>(q, st);
        case 64: return launch_relief_tile<64, 16>(q, st);
        default: return hipErrorInvalidValue;
    }
}

hipError_t mrtx_launch_relief_share(const ShareC& q, hipStream_t st) {
    if (q.rows < 1 || q.cols < 1 || q.Ri < 0 || q.Rj < 0 || !q.relief || !q.sat || !q.out) return hipErrorInvalidValue;
    const int64_t n = (int64_t)q.rows * q.cols;
    hipLaunchKernelGGL(mrtx_rl::share_rows_kernel, dim3(relief_grid(q.rows, 1)), dim3(256), 0, st, q);
    hipLaunchKernelGGL(mrtx_rl::share_cols_kernel, dim3(relief_grid(q.cols, 256)), dim3(256), 0, st, q);
    hipLaunchKernelGGL(mrtx_rl::share_box_kernel, dim3(relief_grid(n, 256)), dim3(256), 0, st, q);
    return hipGetLastError();
}
