// mrtx_outline.h -- launch blocks of the region outlines (mrtx_regions_outline; DESIGN.md sections 3.23, 4.29), shared by
// mrtx_outline.hip and the host side.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// at most 2^28 nodes: a side id 4 v + k then stays below 2^30, and every node, side and compact index fits an int32
#define MRTX_OL_MAX_NODES ((int64_t)1 << 28)
// the items (nodes or sides) one block of 256 threads scans, eight in a row per thread
#define MRTX_OL_CHUNK 2048

// MrtxRing, field for field (48 bytes)
struct RingRec {
    long long area, warea;
    unsigned long long first;
    uint32_t n_sides, n_vertices;
    int32_t label, head, wind;
    uint32_t reserved;
};

// the tile of nodes inside which the contract variant joins boundary sides into chains: the label pass's 16 x 64
#define MRTX_OL_TILE_H_SHIFT 4
#define MRTX_OL_TILE_W_SHIFT 6
// no chain is longer than a tile has sides
#define MRTX_OL_CHAIN_MAX 4096
// the default of MOONRT_REGIONS_OUTLINE (DESIGN.md section 4.29 has the measurement behind it)
#define MRTX_OL_DEFAULT_CONTRACT true

// One element's window of the pointer jumping: 2^r elements from itself on along the successor map.  An element is a boundary
// side (jump) or a chain of them (contract).  jump: the element right after the window; mn: the least compact index among the
// elements' first sides, at its first occurrence d sides on; sf, sx: the vertex flags and column steps of the d sides before
// that; tf, tx, tl: those of the whole window and its number of sides (meaningless once the window has gone round its ring,
// and not used from then on).  After the last round, per side: mn, d, sf, sx alone.
struct alignas(16) OutlineJump {
    int32_t jump, mn, d, sf;
    int32_t sx, tf, tx, tl;
};

struct OutlineC {
    const int32_t* labels;          // rows x cols, the caller's own: every entry is bound-checked
    const unsigned long long* cw;   // rows + 1: the exclusive prefix sum of row_weight, or null: every row weighs 1
    // per node
    uint8_t* bits;                  // bit k: side k is a boundary side
    uint32_t* base;                 // the boundary sides of all nodes before this one = the compact index of its first
    uint2* node_sums;               // per chunk of nodes
    // per boundary side, by compact index (ascending side id)
    int32_t* sid;                   // the side id 4 v + k
    int32_t* next;                  // the successor
    uint32_t* ringno;               // at a head: its ring's number
    uint8_t* flag;                  // the side contributes its start corner
    uint8_t* jflag;                 // contract: the side starts a chain
    uint32_t* jidx;                 // contract: at a chain's first side, the chain's number
    uint2* side_sums;               // per chunk of sides: (heads, vertices)
    OutlineJump* jump[2];
    const OutlineJump* fin;         // per side after the trace: jump[rounds & 1] (jump), the other buffer (contract)
    // counters: bad[0] = entries outside -1 .. n_regions - 1, bad[1] = broken successors or chains (never); totals[0] = B,
    // totals[2] = rings, totals[3] = vertices, totals[4] = chains
    uint32_t* bad;
    unsigned long long* totals;
    RingRec* rings;
    int32_t* vertices;              // (y, x) pairs
    int32_t rows, cols, wrap, conn8, all, contract;
    uint32_t n_regions;
    uint32_t B;                     // boundary sides, known after mrtx_launch_outline_mark
    int32_t rounds;                 // ceil(log2 B)
};

static inline size_t outline_up16(size_t n) { return (n + 15) & ~(size_t)15; }
static inline size_t outline_chunks(size_t n) { return (n + MRTX_OL_CHUNK - 1) / MRTX_OL_CHUNK; }
static inline int32_t outline_rounds(uint32_t B) {
    int32_t r = 0;
    while (((uint64_t)1 << r) < B) r++;
    return r;
}

// Where the per-node scratch lies, in bytes from the start of one block: 64 bytes of counters (bad at 0, totals at 16), then the
// tables.  All in size_t.
struct OutlineNodeLayout {
    size_t bits_at, base_at, sums_at, end;
};
static inline OutlineNodeLayout outline_node_layout(int32_t rows, int32_t cols) {
    const size_t N = (size_t)rows * (size_t)cols;
    OutlineNodeLayout l;
    l.bits_at = 64;
    l.base_at = l.bits_at + outline_up16(N);
    l.sums_at = l.base_at + outline_up16(4 * N);
    l.end = l.sums_at + outline_up16(8 * outline_chunks(N));
    return l;
}

// Where the per-side scratch lies in a second block.  After the trace one jump buffer holds the per-side result and the other
// is dead (jump: the one the last round read; contract: the elements' last one): its 32 B bytes take the tables a caller wants
// on the host, at most B / 3 rings of 48 bytes (a ring has at least three sides) and B vertices of 8.
struct OutlineSideLayout {
    size_t sid_at, next_at, ringno_at, jidx_at, flag_at, jflag_at, sums_at, jump_at[2], end;
};
static inline OutlineSideLayout outline_side_layout(uint32_t B) {
    const size_t b = B;
    OutlineSideLayout l;
    l.sid_at = 0;
    l.next_at = l.sid_at + outline_up16(4 * b);
    l.ringno_at = l.next_at + outline_up16(4 * b);
    l.jidx_at = l.ringno_at + outline_up16(4 * b);
    l.flag_at = l.jidx_at + outline_up16(4 * b);
    l.jflag_at = l.flag_at + outline_up16(b);
    l.sums_at = l.jflag_at + outline_up16(b);
    l.jump_at[0] = l.sums_at + outline_up16(8 * outline_chunks(b));
    l.jump_at[1] = l.jump_at[0] + sizeof(OutlineJump) * b;
    l.end = l.jump_at[1] + sizeof(OutlineJump) * b;
    return l;
}
// the host-bound tables inside the dead jump buffer: rings at 0, vertices behind them
static inline size_t outline_host_vertices_at(uint64_t n_rings) { return outline_up16(sizeof(RingRec) * (size_t)n_rings); }

// mark: the boundary bits, the label check and the compaction (sets totals[0] = B).  trace: successors, pointer jumping and the
// count of rings and vertices (needs q.B, q.rounds).  fill: the ring records and the vertex table (needs the two counts).
hipError_t mrtx_launch_outline_mark(const OutlineC& q, hipStream_t st, uint32_t* launches);
hipError_t mrtx_launch_outline_trace(const OutlineC& q, hipStream_t st, uint32_t* launches);
hipError_t mrtx_launch_outline_fill(const OutlineC& q, uint64_t n_rings, hipStream_t st, uint32_t* launches);
