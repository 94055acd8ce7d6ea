// mrtx_proximity.h -- launch blocks of the proximity maps and the reach of labelled regions (mrtx_proximity,
// mrtx_regions_reach; DESIGN.md sections 3.22, 4.28), shared by mrtx_proximity.hip and the host side.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// a lattice tile: MRTX_PX_TW x MRTX_PX_TW nodes, one per lane of a wave
#define MRTX_PX_TW 8
#define MRTX_PX_TILE 64
// every coordinate lies in -MRTX_PX_CMAX .. MRTX_PX_CMAX, so a difference fits 31 bits and d2 is at most 3 x 2^60
#define MRTX_PX_CMAX (1 << 29)

// one feature of a tile's list: its position and its node index
struct ProxFeat {
    int32_t x, y, z, v;
};

// the bounding box of the positions of a tile's features, and their number; lo > hi when there is none
struct ProxBox {
    int32_t lo[3], hi[3];
    int32_t n;
    int32_t pad;
};

struct ProxC {
    const int32_t* pos;         // rows x cols x 3, the caller's own: every coordinate is checked and clamped
    const int32_t* labels;      // rows x cols
    int32_t* nearest;           // rows x cols
    unsigned long long* dist2;  // rows x cols
    ProxBox* box;               // one per tile
    ProxFeat* feat;             // MRTX_PX_TILE per tile: the tile's features first, in the order of their lanes
    unsigned long long* pairs;  // [0]: (node, feature) distance evaluations
    uint32_t* bad;              // coordinates outside +-MRTX_PX_CMAX
    int32_t rows, cols, outside;
    int32_t tiles_x, tiles_y;
};

// Where a call's scratch lies, in bytes from the start of one block: 32 bytes of counters (pairs, bad), the tiles' boxes, their
// feature lists, and the outputs the caller wants on the host.  All in size_t: at 2^31 nodes the lists alone are 32 GiB.
struct ProxLayout {
    int32_t tiles_x, tiles_y;
    size_t tiles, box_at, feat_at, near_at, d2_at, end;
};
static inline ProxLayout prox_layout(int32_t rows, int32_t cols, bool host_nearest, bool host_dist2) {
    ProxLayout l;
    l.tiles_x = (int32_t)(((int64_t)cols + MRTX_PX_TW - 1) / MRTX_PX_TW);
    l.tiles_y = (int32_t)(((int64_t)rows + MRTX_PX_TW - 1) / MRTX_PX_TW);
    l.tiles = (size_t)l.tiles_x * (size_t)l.tiles_y;
    const size_t N = (size_t)rows * (size_t)cols;
    l.box_at = 32;
    l.feat_at = l.box_at + sizeof(ProxBox) * l.tiles;
    l.near_at = l.feat_at + sizeof(ProxFeat) * MRTX_PX_TILE * l.tiles;
    l.d2_at = l.near_at + (host_nearest ? (4 * N + 7) & ~(size_t)7 : 0);
    l.end = l.d2_at + (host_dist2 ? 8 * N : 0);
    return l;
}

// MrtxRegionReach, field for field (32 bytes)
struct ReachRec {
    unsigned long long d2_max, d2_min;
    int32_t max_at, min_at, min_nearest;
    uint32_t count;
};

struct ReachC {
    const int32_t* labels;      // rows x cols, the caller's own: every entry is bound-checked
    const unsigned long long* dist2;
    const int32_t* nearest;
    ReachRec* out;              // n_regions records
    uint32_t* bad;              // entries outside -1 .. n_regions - 1
    int32_t rows, cols;
    uint32_t n_regions;
};

hipError_t mrtx_launch_proximity(const ProxC& q, bool prune, hipStream_t st, uint32_t* launches);
hipError_t mrtx_launch_regions_reach(const ReachC& q, hipStream_t st, uint32_t* launches);
