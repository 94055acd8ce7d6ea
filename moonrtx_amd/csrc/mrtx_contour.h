// mrtx_contour.h -- launch blocks and scratch layouts of the contour lines (mrtx_contours; DESIGN.md sections 3.26, 4.32), shared
// by mrtx_contour.hip and the host side.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// at most 2^28 nodes: an edge id 2 v + k then stays below 2^29, and every node, edge and compact index fits an int32
#define MRTX_CT_MAX_NODES ((int64_t)1 << 28)
#define MRTX_CT_MAX_LEVELS 65536
// every height lies in -MRTX_CT_ZMAX .. MRTX_CT_ZMAX or is MRTX_CT_VOID (MRTX_FILL_NONE); every level in -MRTX_CT_ZMAX + 1 .. MRTX_CT_ZMAX
#define MRTX_CT_ZMAX (1 << 30)
#define MRTX_CT_VOID 2147483647
// the items (nodes or elements) one block of 256 threads scans, eight per thread
#define MRTX_CT_CHUNK 2048
// the level table lies in LDS up to this many levels (16 KiB), beyond it the searches read global memory
#define MRTX_CT_LDS_LEVELS 4096
// the rank of a void node (a valid node's is 0 .. n_levels)
#define MRTX_CT_NORANK 0xFFFFFFFFu

// MrtxContourLine, field for field (32 bytes)
struct ContourLineRec {
    unsigned long long first;
    uint32_t n_vertices;
    int32_t level_index, level, head, tail;
    uint32_t closed;
};

// One element's window of the pointer jumping: itself and the 2^r - 1 elements before it along the predecessor map, or fewer
// when the window reaches the start of an open line.  x: the element right before the window, or -1 once the window holds a
// start; y: that start, else the least compact index in the window, at its first occurrence z elements back; w: the window's
// length (used only while the window has neither reached a start nor gone round its cycle).
typedef int4 ContourJump;

struct ContourC {
    const int32_t* z;               // rows x cols, the caller's own: every value is checked
    const int32_t* levels;          // n_levels, ascending (checked by the host)
    // per node
    uint32_t* rank;                 // the number of levels <= z, so the node is above level l iff l < rank; MRTX_CT_NORANK: void
    // per edge e = 2 v + k: the elements of all edges before it = the compact index of its first (after the count kernel and
    // before the base kernel: its own number of elements)
    uint32_t* base;
    unsigned long long* node_sums;  // per chunk of nodes
    // per element, by compact index (ascending (e, l))
    int32_t* eid;                   // the edge id
    int32_t* succ;                  // the successor, or -1
    uint32_t* len;                  // at a head: its line's length
    int32_t* tailat;                // at a head: its line's last element
    uint32_t* lineno;               // at a head: its line's number
    uint2* side_sums;               // per chunk of elements: (heads, vertices)
    ContourJump* jump[2];
    const ContourJump* fin;         // per element after the trace: jump[rounds & 1]
    // counters: bad[0] = heights outside the range, bad[1] = broken successors, heads or positions (never); totals[0] = B,
    // totals[2] = lines, totals[3] = vertices
    uint32_t* bad;
    unsigned long long* totals;
    ContourLineRec* lines;
    int32_t* vertices;              // edge ids
    int32_t rows, cols, wrap, n_levels;
    uint32_t B;                     // elements, known after mrtx_launch_contour_count
    int32_t rounds;                 // ceil(log2 B)
};

static inline size_t contour_up16(size_t n) { return (n + 15) & ~(size_t)15; }
static inline size_t contour_chunks(size_t n) { return (n + MRTX_CT_CHUNK - 1) / MRTX_CT_CHUNK; }
static inline int32_t contour_rounds(uint32_t B) {
    int32_t r = 0;
    while (((uint64_t)1 << r) < B) r++;
    return r;
}

// Where the per-node scratch lies, in bytes from the start of one block: 64 bytes of counters (bad at 0, totals at 16), the
// level table, the heights when they come from the host, then the tables.  All in size_t.
struct ContourNodeLayout {
    size_t levels_at, z_at, rank_at, base_at, sums_at, end;
};
static inline ContourNodeLayout contour_node_layout(int32_t rows, int32_t cols, int32_t n_levels, bool host_z) {
    const size_t N = (size_t)rows * (size_t)cols;
    ContourNodeLayout l;
    l.levels_at = 64;
    l.z_at = l.levels_at + contour_up16(4 * (size_t)n_levels);
    l.rank_at = l.z_at + (host_z ? contour_up16(4 * N) : 0);
    l.base_at = l.rank_at + contour_up16(4 * N);
    l.sums_at = l.base_at + contour_up16(8 * N);
    l.end = l.sums_at + contour_up16(8 * contour_chunks(N));
    return l;
}

// Where the per-element scratch lies in a second block: 52 bytes per element
struct ContourSideLayout {
    size_t eid_at, succ_at, len_at, tailat_at, lineno_at, sums_at, jump_at[2], end;
};
static inline ContourSideLayout contour_side_layout(uint32_t B) {
    const size_t b = B;
    ContourSideLayout l;
    l.eid_at = 0;
    l.succ_at = l.eid_at + contour_up16(4 * b);
    l.len_at = l.succ_at + contour_up16(4 * b);
    l.tailat_at = l.len_at + contour_up16(4 * b);
    l.lineno_at = l.tailat_at + contour_up16(4 * b);
    l.sums_at = l.lineno_at + contour_up16(4 * b);
    l.jump_at[0] = l.sums_at + contour_up16(8 * contour_chunks(b));
    l.jump_at[1] = l.jump_at[0] + sizeof(ContourJump) * b;
    l.end = l.jump_at[1] + sizeof(ContourJump) * b;
    return l;
}
// the host-bound tables in a third block: lines at 0, vertices behind them
static inline size_t contour_host_vertices_at(uint64_t n_lines) { return contour_up16(sizeof(ContourLineRec) * (size_t)n_lines); }

// count: the ranks, the check of the heights and the compaction (sets totals[0] = B).  trace: the elements' edges, successors
// and predecessors, the pointer jumping and the count of lines (needs q.B, q.rounds).  fill: the line records and the vertex
// table (needs the number of lines).
hipError_t mrtx_launch_contour_count(const ContourC& q, hipStream_t st, uint32_t* launches);
hipError_t mrtx_launch_contour_trace(const ContourC& q, hipStream_t st, uint32_t* launches);
hipError_t mrtx_launch_contour_fill(const ContourC& q, uint64_t n_lines, hipStream_t st, uint32_t* launches);
