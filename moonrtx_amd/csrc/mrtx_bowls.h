// mrtx_bowls.h -- launch blocks of the depression hierarchy (mrtx_bowls; DESIGN.md sections 3.25, 4.31), shared by
// mrtx_bowls.hip and the host side.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// every height lies in -MRTX_BOWLS_ZMAX .. MRTX_BOWLS_ZMAX (mrtx_fill's bound), so z + 2^30 fits the high word of a packed key
#define MRTX_BOWLS_ZMAX (1 << 30)
// pointer-jumping launches per read of the change counter
#define MRTX_BOWLS_BATCH 4
// no hook: the component stays a root in this round
#define MRTX_BOWLS_NOHOOK 0xFFFFFFFFu

// The packed key of node v: (z'[v] + 2^30) << 32 | v, z' = -z with invert.  Ascending packed keys are ascending (z', v).
// Ids of catchments and components are node indices as uint32; the outside is N = rows x cols (at most 2^31).

// one edge of the spanning forest: the pass node's key and the catchments (minima, or N for the outside) of its two ends
struct BowlEdge {
    unsigned long long pass;
    uint32_t a, b;
};

// what the label walk needs of a bowl: the key of its spill node (~0: never spills), its parent (-1: none), and for a leaf the
// node it was born at (-1 for a meta bowl)
struct BowlWalk {
    unsigned long long spill;
    int32_t parent, leaf_at;
};

struct BowlC {
    const int32_t* z;           // rows x cols, the caller's own: every height is clamped where it is read
    const uint8_t* outlet;      // rows x cols, or null
    const uint32_t* row_weight; // rows, or null: every node weighs 1
    uint32_t* ptr;              // N + 1: the steepest-descent pointer by key, after the jumps the catchment (a minimum, or N)
    uint32_t* cpar;             // N + 1: the component of a catchment, flat between rounds; afterwards the leaf bowl of a minimum
    unsigned long long* best;   // N + 1, per component: the least pass key among its cross edges
    uint32_t* best2;            // N + 1, per component: the least low end among the cross edges with that pass key
    unsigned long long* list;   // n_min: the packed keys of the minima, in no order; entry n_min of the kernels stands for N
    uint32_t* hook;             // n_min + 1: where each listed component hooks in this round, or MRTX_BOWLS_NOHOOK
    BowlEdge* edges;            // n_min: the chosen edges, in no order
    uint32_t* counters;         // [0] heights beyond the bound, [1] minima, [2] edges, [3] list cursor, [4] edges past the
                                // table, [8 ..] MRTX_BOWLS_BATCH per-launch change counters
    const BowlWalk* walk;       // n_bowls
    int32_t* label;             // rows x cols, or null: no label table
    unsigned long long* own;    // n_bowls x 3: nodes, weight and the sum of w z' (modulo 2^64) of the nodes labelled with a bowl
    int32_t rows, cols, wrap, conn8, edge_outlets, invert, slot;
    uint32_t n_min, n_bowls;
};

hipError_t mrtx_launch_bowls_init(const BowlC& q, hipStream_t st);
hipError_t mrtx_launch_bowls_jump(const BowlC& q, hipStream_t st);
hipError_t mrtx_launch_bowls_list(const BowlC& q, hipStream_t st);
hipError_t mrtx_launch_bowls_round(const BowlC& q, hipStream_t st, uint32_t* launches);
hipError_t mrtx_launch_bowls_label(const BowlC& q, hipStream_t st, uint32_t* launches);
