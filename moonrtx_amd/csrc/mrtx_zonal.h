// mrtx_zonal.h -- launch blocks of the zonal statistics and outlines of labelled regions (mrtx_regions_zonal,
// mrtx_regions_shape; DESIGN.md sections 3.21, 4.27), shared by mrtx_zonal.hip and the host side.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// MrtxZonal, field for field (56 bytes); min .. max_at are written by zonal_finish_kernel from the packed keys
struct ZonalRec {
    unsigned long long wcount;
    unsigned long long wsum, sum;           // int64 sums, added modulo 2^64
    uint32_t count, n_nan, n_clipped;
    float min, max;
    int32_t min_at, max_at;
    uint32_t reserved;
};

struct ZonalC {
    const int32_t* labels;      // rows x cols, the caller's own: every entry is bound-checked
    const float* field;         // rows x cols x n_ch
    const uint32_t* row_weight; // rows, or null: every node weighs 1
    ZonalRec* out;              // n_regions x n_ch records
    unsigned long long* keys;   // n_regions x n_ch x 2: (key(x) << 32 | index) under min, (key(x) << 32 | ~index) under max
    unsigned long long* hist;   // n_regions x (n_bins + 2), or null
    uint32_t* bad;              // entries outside -1 .. n_regions - 1
    double scale, hist_lo, hist_inv_w;
    int32_t rows, cols, n_ch, hist_ch, n_bins;
    uint32_t n_regions;
};

// MrtxRegionShape, field for field (32 bytes)
struct ShapeRec {
    unsigned long long perimeter;
    uint32_t sides_ns, sides_ew, q1, q3, qd;
    int32_t euler;
};

struct ShapeC {
    const int32_t* labels;
    const uint32_t* side_ew;    // rows, or null: every side counts 1
    const uint32_t* side_ns;    // rows + 1, or null
    ShapeRec* out;              // n_regions records
    uint32_t* bad;
    int32_t rows, cols, wrap, conn8;
    uint32_t n_regions;
};

hipError_t mrtx_launch_regions_zonal(const ZonalC& q, bool runs, hipStream_t st, uint32_t* launches);
hipError_t mrtx_launch_regions_shape(const ShapeC& q, bool runs, hipStream_t st, uint32_t* launches);
