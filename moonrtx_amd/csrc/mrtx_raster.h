// mrtx_raster.h -- launch blocks of the polygon rasterisation (mrtx_rasterise; DESIGN.md sections 3.29, 4.38), shared by
// mrtx_raster.hip and the host side.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// at most 2^28 nodes, as the outlines: every node index fits an int32
#define MRTX_RS_MAX_NODES ((int64_t)1 << 28)
// every vertex coordinate lies within +-2^24 units of 2^-s of a cell, s <= 8
#define MRTX_RS_CMAX (1 << 24)
#define MRTX_RS_MAX_SUBCELL 8
// the items one block of 256 threads scans, eight in a row per thread
#define MRTX_RS_CHUNK 2048
// a bin is a polygon x a strip of 64 columns; a call holds at most 2^28 of them
#define MRTX_RS_STRIP_SHIFT 6
#define MRTX_RS_MAX_BINS ((uint64_t)1 << 28)
// the rows one wave of the cover launch walks, and the crossings it stages in LDS at a time
#define MRTX_RS_ROWS 64
#define MRTX_RS_STAGE 64
// a ring table, a vertex table, the edges of all rings and the crossings each stay below 2^31
#define MRTX_RS_MAX_COUNT (((uint64_t)1 << 31) - 1)

// MrtxRasterRing, field for field (24 bytes)
struct RasterRing {
    unsigned long long first;
    uint32_t n_vertices;
    int32_t polygon, wind;
    uint32_t reserved;
};

// MrtxPolygonCover, field for field (40 bytes)
struct CoverRec {
    unsigned long long weight, owned_weight;
    uint32_t count, owned;
    int32_t i_min, i_max, first_at;
    uint32_t reserved;
};

// the counters at the head of the scratch block, 8 bytes each
enum { RS_BAD_RINGS = 0, RS_BAD_COORDS = 1, RS_EDGES = 2, RS_CROSSINGS = 3, RS_BINNED = 4, RS_HEAD = 8 };

struct RasterC {
    const RasterRing* rings;        // the caller's own: every record is checked
    const int32_t* vertices;        // (y, x) pairs
    const uint32_t* row_weight;     // rows, or null: every row weighs 1
    int32_t* labels;                // rows x cols
    CoverRec* cover;                // n_polygons
    unsigned long long* head;       // RS_HEAD counters
    uint32_t* edge_off;             // per ring: its edges (0 for a bad ring), scanned: the number of its first edge
    uint32_t* bin_off;              // bins: per bin its crossings, scanned, and after the fill the end of the bin
    uint32_t* poly_off;             // brute: per polygon its rings, scanned, and after the ordering the end of the polygon
    uint32_t* order;                // brute: the rings grouped by polygon
    unsigned long long* sums;       // the scans' chunk sums
    uint2* cross;                   // bins: per crossing (first row, column in the strip | 64 when the sign is -1)
    unsigned long long n_rings, n_vertices;
    uint32_t n_polygons, n_edges, n_bins;
    uint32_t n_cross;               // the crossings, known after mrtx_launch_raster_count
    int32_t rows, cols, wrap, s, evenodd, last, strips, bins;
};

static inline size_t raster_up16(size_t n) { return (n + 15) & ~(size_t)15; }
static inline size_t raster_chunks(size_t n) { return (n + MRTX_RS_CHUNK - 1) / MRTX_RS_CHUNK; }
static inline int32_t raster_strips(int32_t cols) { return (cols + (1 << MRTX_RS_STRIP_SHIFT) - 1) >> MRTX_RS_STRIP_SHIFT; }

// Where the scratch lies, in bytes from the start of one block: 64 bytes of counters, then the tables, then the outputs a
// caller wants on the host.  All in size_t.
struct RasterLayout {
    size_t edge_at, bin_at, poly_at, order_at, sums_at, labels_at, cover_at, end;
};
static inline RasterLayout raster_layout(int32_t rows, int32_t cols, uint64_t n_rings, uint32_t n_polygons, bool bins, bool host_labels,
                                         bool host_cover) {
    const size_t N = (size_t)rows * (size_t)cols, R = (size_t)n_rings, P = n_polygons;
    const size_t B = bins ? P * (size_t)raster_strips(cols) : 0;
    RasterLayout l;
    l.edge_at = 8 * RS_HEAD;
    l.bin_at = l.edge_at + raster_up16(4 * R);
    l.poly_at = l.bin_at + raster_up16(4 * B);
    l.order_at = l.poly_at + raster_up16(bins ? 0 : 4 * P);
    l.sums_at = l.order_at + raster_up16(bins ? 0 : 4 * R);
    l.labels_at = l.sums_at + raster_up16(8 * (raster_chunks(R > B ? (R > P ? R : P) : (B > P ? B : P)) + 1));
    l.cover_at = l.labels_at + (host_labels ? raster_up16(4 * N) : 0);
    l.end = l.cover_at + (host_cover ? raster_up16(sizeof(CoverRec) * P) : 0) + 16;
    return l;
}

// check: every ring record and coordinate, and the number of each ring's first edge (sets RS_BAD_*, RS_EDGES).  count: the
// crossings of all edges (needs q.n_edges; sets RS_CROSSINGS).  cover: the labels and the cover records (needs q.cross for the
// bins variant).
hipError_t mrtx_launch_raster_check(const RasterC& q, hipStream_t st, uint32_t* launches);
hipError_t mrtx_launch_raster_count(const RasterC& q, hipStream_t st, uint32_t* launches);
hipError_t mrtx_launch_raster_cover(const RasterC& q, hipStream_t st, uint32_t* launches);
