// mrtx_fill.h -- launch blocks of the terrain depressions (mrtx_fill, mrtx_fill_basins; DESIGN.md sections 3.24, 4.30),
// shared by mrtx_fill.hip and the host side.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// every height lies in -MRTX_FILL_ZMAX .. MRTX_FILL_ZMAX, so a depth fits an int32 wherever the fill is a height
#define MRTX_FILL_ZMAX (1 << 30)
// the tile edge of fill_relax_kernel (the only one instantiated)
#define MRTX_FILL_TS 32
// relaxation launches per read of the change counter
#define MRTX_FILL_BATCH 8

struct FillC {
    const int32_t* z;           // rows x cols, the caller's own: every height is clamped where it is read
    const uint8_t* outlet;      // rows x cols, or null
    int32_t* w;                 // rows x cols: the fill
    int32_t* w_in;              // sweep only: the table a Jacobi step reads (w is the one it writes)
    uint32_t* flag_in;          // tiles only: one word per tile, the tiles of this launch
    uint32_t* flag_out;         //             and those of the next
    unsigned long long* visits; // [0]: tile visits (tiles), node updates (sweep)
    uint32_t* bad;              // heights outside +-MRTX_FILL_ZMAX
    uint32_t* changed;          // MRTX_FILL_BATCH per-launch change counters
    int32_t rows, cols, wrap, conn8, edge_outlets;
    int32_t tiles_x, tiles_y, slot;
};

// MrtxBasin, field for field (48 bytes); depth_max .. pour_level are written by basins_finish_kernel from the packed keys
struct BasinRec {
    unsigned long long weight, volume;
    uint32_t count;
    int32_t level_min, level_max, depth_max, deepest_at, pour_at, pour_level;
    uint32_t reserved;
};

struct BasinC {
    const int32_t* labels;      // rows x cols, the caller's own: every entry is bound-checked
    const int32_t* z;           // rows x cols, clamped where it is read
    const int32_t* fill;        // rows x cols, any table
    const uint32_t* row_weight; // rows, or null: every node weighs 1
    BasinRec* out;              // n_regions records
    unsigned long long* keys;   // n_regions x 2: (fill[u] + 2^31) << 32 | u under min, depth << 32 | ~v under max
    uint32_t* bad;              // [0] labels outside -1 .. n_regions - 1, [1] heights outside +-MRTX_FILL_ZMAX
    int32_t rows, cols, wrap, conn8;
    uint32_t n_regions;
};

hipError_t mrtx_launch_fill_init(const FillC& q, bool tiles, hipStream_t st);
hipError_t mrtx_launch_fill_relax(const FillC& q, hipStream_t st);
hipError_t mrtx_launch_fill_sweep(const FillC& q, hipStream_t st);
hipError_t mrtx_launch_fill_basins(const BasinC& q, hipStream_t st, uint32_t* launches);
