// mrtx_lattice_dev.h -- the device helpers that the lattice stages' kernels share word for word.
// Everything here is __forceinline__: no function of its own reaches a code object, and a kernel that was built from one of
// these bodies keeps its name, its namespace and its instructions (tools/asm_same.py).  The __shared__ arrays stay in the
// kernels, which hand them in.  The two scan_chunks_kernel (mrtx_outline.hip, mrtx_contour.hip) are the same text and stay two:
// built from one body they compile to other instructions.  Device code only: included by the stages' .hip files, never by the host units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mrtx_lat {

__device__ __forceinline__ bool label_ok(uint32_t n_regions, int32_t l) { return l >= 0 && (uint32_t)l < n_regions; }

// a record's field as every workgroup of the device sees it
__device__ __forceinline__ unsigned long long value_now(const unsigned long long* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int32_t value_now(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// a 64-bit value from lane ^ m
__device__ __forceinline__ unsigned long long xor64(unsigned long long v, int m) {
    const uint32_t lo = __shfl_xor((uint32_t)v, m), hi = __shfl_xor((uint32_t)(v >> 32), m);
    return ((unsigned long long)hi << 32) | lo;
}

// The body of a check_kernel (blocks of 256): the count of entries outside -1 .. n_regions - 1, added to *out.
__device__ __forceinline__ void check_labels(const int32_t* labels, int64_t N, uint32_t n_regions, uint32_t* out) {
    uint32_t bad = 0;
    for (int64_t n = blockIdx.x * (int64_t)256 + threadIdx.x; n < N; n += (int64_t)gridDim.x * 256) {
        const int32_t l = labels[n];
        bad += l < -1 || (l >= 0 && (uint32_t)l >= n_regions);
    }
    if (bad) atomicAdd(out, bad);
}

__device__ __forceinline__ uint2 add2(uint2 a, uint2 b) { return make_uint2(a.x + b.x, a.y + b.y); }

// the exclusive scan of v over the block's 256 threads; *total receives the block's sum.  sh: 4 entries.
__device__ __forceinline__ uint2 block_scan(uint2 v, uint2* sh, uint2* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint2 inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t ax = __shfl_up(inc.x, d), ay = __shfl_up(inc.y, d);
        if (lane >= d) { inc.x += ax; inc.y += ay; }
    }
    __syncthreads();            // sh may still be read from the call before
    if (lane == 63) sh[w] = inc;
    __syncthreads();
    uint2 off = make_uint2(0, 0), tot = make_uint2(0, 0);
    for (int k = 0; k < 4; k++) {
        const uint2 s = sh[k];
        if (k < w) off = add2(off, s);
        tot = add2(tot, s);
    }
    *total = tot;
    return make_uint2(off.x + inc.x - v.x, off.y + inc.y - v.y);
}

}  // namespace mrtx_lat
