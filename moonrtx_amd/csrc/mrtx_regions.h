// mrtx_regions.h -- launch blocks of the regions stage (mrtx_regions_label, mrtx_regions_stats; DESIGN.md sections 3.20, 4.26),
// shared by mrtx_regions.hip and the host side.  A header of its own: the other translation units do not see it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// a tile of the label pass: one 256-lane workgroup, four nodes per lane; a wave reads 64 consecutive columns of a row
#define MRTX_RG_TH 16
#define MRTX_RG_TW 64
// nodes per workgroup of the flatten, rank and relabel passes (256 lanes x 16)
#define MRTX_RG_CHUNK 4096

struct RegionsC {
    const float* field;         // rows x cols x n_ch, or null
    const uint8_t* mask;        // rows x cols, or null: exactly one of the two
    int32_t* parent;            // rows x cols: the union-find forest, parent[v] <= v, -1 outside the set
    int32_t* labels;            // rows x cols: the output
    uint32_t* sums;             // one per chunk: its roots, then their exclusive prefix
    uint32_t* total;            // K
    int32_t rows, cols, wrap, conn8, n_ch, ch;
    int32_t tiles_x;
    float lo, hi;
    uint32_t n_chunks;
};

// MrtxRegion, field for field (56 bytes); root_i holds the root's node index until stats_finish_kernel splits it
struct RegionRec {
    unsigned long long weight;
    unsigned long long sum_i, sum_dj;       // int64 sums, added modulo 2^64
    uint32_t count;
    int32_t root_i, root_j, i_min, i_max, dj_min, dj_max;
    uint32_t reserved;
};

struct RegionStatsC {
    const int32_t* labels;      // rows x cols, the caller's own: every entry is bound-checked
    const uint32_t* row_weight; // rows, or null: every node weighs 1
    RegionRec* out;             // n_regions records
    uint32_t* bad;              // entries outside -1 .. n_regions - 1
    int32_t rows, cols, wrap;
    uint32_t n_regions;
};

hipError_t mrtx_launch_regions_label(const RegionsC& q, hipStream_t st, uint32_t* launches);
hipError_t mrtx_launch_regions_stats(const RegionStatsC& q, bool runs, hipStream_t st, uint32_t* launches);
