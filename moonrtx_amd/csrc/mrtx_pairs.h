// mrtx_pairs.h -- launch blocks of the joint availability of mask rows (mrtx_mask_pairs; DESIGN.md sections 3.28, 4.37), shared
// by mrtx_pairs.hip and the host side.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// a tile of B rows: one row per lane of a wave; a tile of A rows: MRTX_PAIRS_TA rows, each against every lane's B row
#define MRTX_PAIRS_TB 64
#define MRTX_PAIRS_TA 8
// the words of a row that are staged in LDS at a time (_lib.PAIRS_CHUNK_WORDS mirrors it)
#define MRTX_PAIRS_CHUNK 32
// every coordinate lies in -MRTX_PAIRS_CMAX .. MRTX_PAIRS_CMAX, as mrtx_proximity's: a difference fits 31 bits, d2 is at most 3 x 2^60
#define MRTX_PAIRS_CMAX (1 << 29)
// the workgroups a BEST call aims at when it splits B (the split depends on n_a and n_b alone)
#define MRTX_PAIRS_SPLIT_GROUPS 2048

// MrtxMaskPairs' BEST and ROWS record, field for field (16 bytes)
struct PairRec {
    int32_t partner;
    uint32_t count, gap;
    int32_t gap_first;
};
// the TABLE record (8 bytes)
struct PairCell {
    uint32_t count, gap;
};

// a BEST candidate while it is being reduced (16 bytes): the rank's key of (count, gap), the partner and the gap's first epoch
struct PairPick {
    unsigned long long key;
    int32_t partner, first;
};

// the bounding box of the positions of a tile of rows
struct PairBox {
    int32_t lo[3], hi[3];
};

struct PairsC {
    const unsigned long long* a;        // n_a x w64
    const unsigned long long* b;        // n_b x w64 (a itself when self)
    const unsigned long long* base;     // w64, or null
    const int32_t* pos_a;               // n_a x 3 or null, the caller's own: every coordinate is checked and clamped
    const int32_t* pos_b;               // n_b x 3 (pos_a itself when self)
    void* out;                          // PairRec[n_a] (ROWS, BEST) or PairCell[n_a x n_b] (TABLE)
    PairPick* part;                     // BEST with splits > 1: n_a x splits partial candidates
    PairBox* box_a;                     // one per tile of MRTX_PAIRS_TA rows of A
    PairBox* box_b;                     // one per tile of MRTX_PAIRS_TB rows of B
    unsigned long long* pairs;          // [0]: eligible pairs evaluated
    uint32_t* bad;                      // coordinates outside +-MRTX_PAIRS_CMAX
    unsigned long long d2_min, d2_max;
    int32_t n_a, n_b, m, w64;
    int32_t op_and, mode, by_gap, self; // mode: MRTX_PAIRS_ROWS / BEST / TABLE
    int32_t splits;
};

// Where a call's scratch lies, in bytes from the start of one block: 32 bytes of counters (pairs, bad), the tiles' boxes and
// the partial records of a split BEST call.  split: the call walks B (BEST, TABLE) and may share it out over `splits`
// workgroups per tile of A; partials: it is BEST, whose shares meet in a second launch.
struct PairsLayout {
    size_t tiles_a, tiles_b, box_a_at, box_b_at, part_at, end;
    int32_t splits;
};
static inline PairsLayout pairs_layout(int32_t n_a, int32_t n_b, bool split, bool partials, bool positions) {
    PairsLayout l;
    l.tiles_a = ((size_t)n_a + MRTX_PAIRS_TA - 1) / MRTX_PAIRS_TA;
    l.tiles_b = ((size_t)n_b + MRTX_PAIRS_TB - 1) / MRTX_PAIRS_TB;
    size_t s = 1;
    if (split && l.tiles_a < MRTX_PAIRS_SPLIT_GROUPS) {
        s = (MRTX_PAIRS_SPLIT_GROUPS + l.tiles_a - 1) / l.tiles_a;
        if (s > l.tiles_b) s = l.tiles_b;
        if (s < 1) s = 1;
    }
    l.splits = (int32_t)s;
    l.box_a_at = 32;
    l.box_b_at = l.box_a_at + (positions ? sizeof(PairBox) * l.tiles_a : 0);
    l.part_at = (l.box_b_at + (positions ? sizeof(PairBox) * l.tiles_b : 0) + 7) & ~(size_t)7;
    l.end = l.part_at + (partials && s > 1 ? sizeof(PairPick) * (size_t)n_a * s : 0);
    return l;
}

// prune: skip the tile pairs whose integer box-to-box bounds prove every pair ineligible.  *launches depends on the block alone.
hipError_t mrtx_launch_mask_pairs(const PairsC& q, bool prune, hipStream_t st, uint32_t* launches);
