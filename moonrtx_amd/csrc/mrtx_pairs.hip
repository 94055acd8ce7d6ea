// mrtx_pairs.hip -- gfx950 kernels of the joint availability of mask rows (mrtx_mask_pairs; DESIGN.md sections 3.28, 4.37).
//
// Rows of w64 uint64 words in mrtx_horizon_mask's layout.  For a pair (a, b) the joint word is J = ((A op B) | base) & V and
// the pair's record is the number of set bits of J and the longest run of clear bits in [0, m) with its earliest start.  All
// integers; no result depends on the order of evaluation.
//   pairs_box_kernel       per tile of rows the int32 bounding box of their positions; every coordinate checked against
//                          +-2^29 (counted) and clamped to it wherever it is read
//   pairs_kernel<MODE>     one wave per workgroup.  The workgroup owns a tile of TA rows of A and a share of the tiles of TB
//                          rows of B; each lane owns one B row against the TA rows of A.  A chunk of CHUNK words of both tiles
//                          (and of base) is staged in LDS: B rows at a stride of CHUNK + 1 words, so that the half-wave's
//                          ds_read_b64 of lane-own rows fall on 32 different bank pairs; an A word is one address for all
//                          lanes, a broadcast.  Per pair (count, carry, best, first) stay in registers across the chunks.  With
//                          positions a lane first decides which of its TA pairs are eligible by the exact d2; a tile in which
//                          no lane has one is not walked.  With prune a tile whose box-to-box bounds prove that is not even
//                          looked at: least possible d2 > d2_max or greatest possible d2 < d2_min.  BEST: every lane keeps the
//                          first record under the rank per A row over its B rows, the wave reduces them at the end (ties to the
//                          least b) -- no atomics; with splits > 1 the workgroup's record is a partial one.  TABLE: every
//                          cell of the tile is written, the ineligible ones (skipped tiles included) as all ones.
//   pairs_combine_kernel   BEST with splits > 1: per A row the first partial record under the rank, shares in ascending order
//   pairs_rows_kernel      ROWS: 64 rows per workgroup through the same LDS layout, each lane walks its own row
// The word walk: z = ~J & V are the clear epochs of a word.  z == 0 closes the running gap, z == all ones extends it by 64, and
// a mixed word gives the run that comes in (carry + trailing ones of z), the longest run strictly inside (z &= z >> 1 until it
// is empty: the last non-empty iterate marks the starts of the longest runs) and the run that goes out (leading ones of z).  A
// run is compared when it forms and each time it grows, with a strict >, so the earliest of equal runs stays.  The bits past
// m - 1 of the last word are 0 in z: a gap ends at m.  Own translation unit: the existing kernels are compiled exactly as before.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/moonrt.h"
#include "mrtx_pairs.h"

namespace mrtx_pr {

typedef unsigned long long u64;

constexpr int TA = MRTX_PAIRS_TA;
constexpr int TB = MRTX_PAIRS_TB;
constexpr int CH = MRTX_PAIRS_CHUNK;
constexpr int BS = CH + 1;              // the stride of a B row in LDS, words: odd, so 32 lanes hit 32 bank pairs
constexpr int32_t CMAX = MRTX_PAIRS_CMAX;
static_assert(TB == 64, "one B row per lane of a wave");
static_assert(CH == 32, "a chunk's word index is idx & 31");
static_assert(TA <= 32, "a lane's eligible pairs are the bits of a word");

__device__ __forceinline__ int32_t clampc(int32_t c) { return c < -CMAX ? -CMAX : c > CMAX ? CMAX : c; }
__device__ __forceinline__ u64 sq(int64_t d) { return (u64)(d * d); }      // |d| <= 2^30

// the least and the greatest squared distance between a point of box p and one of box b
__device__ __forceinline__ u64 box_near(const PairBox& p, const PairBox& b) {
    u64 s = 0;
    for (int k = 0; k < 3; k++) {
        const int64_t u = (int64_t)b.lo[k] - p.hi[k], v = (int64_t)p.lo[k] - b.hi[k];
        const int64_t g = u > v ? u : v;
        s += sq(g > 0 ? g : 0);
    }
    return s;
}
__device__ __forceinline__ u64 box_far(const PairBox& p, const PairBox& b) {
    u64 s = 0;
    for (int k = 0; k < 3; k++) {
        const int64_t u = (int64_t)b.hi[k] - p.lo[k], v = (int64_t)p.hi[k] - b.lo[k];
        s += sq(u > v ? u : v);
    }
    return s;
}

// one thread per tile of `tile` rows
__global__ void __launch_bounds__(256) pairs_box_kernel(const int32_t* pos, int32_t n, int32_t tile, PairBox* box, uint32_t* bad) {
    const int64_t t = blockIdx.x * (int64_t)256 + threadIdx.x;
    const int64_t r0 = t * tile;
    if (r0 >= n) return;
    const int64_t r1 = r0 + tile < n ? r0 + tile : n;
    PairBox b;
    for (int k = 0; k < 3; k++) { b.lo[k] = INT32_MAX; b.hi[k] = INT32_MIN; }
    uint32_t nbad = 0;
    for (int64_t r = r0; r < r1; r++)
        for (int k = 0; k < 3; k++) {
            const int32_t c = pos[3 * r + k], cc = clampc(c);
            nbad += cc != c;
            b.lo[k] = cc < b.lo[k] ? cc : b.lo[k];
            b.hi[k] = cc > b.hi[k] ? cc : b.hi[k];
        }
    box[t] = b;
    if (bad && nbad) atomicAdd(bad, nbad);
}

// what a pair holds across the words of its rows
struct Run {
    uint32_t count, carry, best;
    int32_t first;
};

// word j (masked by v already) whose first epoch is p
__device__ __forceinline__ void walk(Run& r, u64 j, u64 v, int32_t p) {
    r.count += (uint32_t)__popcll(j);
    const u64 z = ~j & v;
    if (z == 0ull) { r.carry = 0; return; }
    if (z == ~0ull) {
        r.carry += 64u;
        if (r.carry > r.best) { r.best = r.carry; r.first = p + 64 - (int32_t)r.carry; }
        return;
    }
    const int lo = __builtin_ctzll(~z), hi = __builtin_clzll(~z);       // ~z != 0, and lo + hi < 64
    const uint32_t in = r.carry + (uint32_t)lo;
    if (in > r.best) { r.best = in; r.first = p - (int32_t)r.carry; }
    u64 x = z & ~((1ull << lo) - 1ull);
    if (hi) x &= ~0ull >> hi;
    if (x) {
        uint32_t len = 0;
        u64 last;
        do { last = x; x &= x >> 1; len++; } while (x);
        if (len > r.best) { r.best = len; r.first = p + __builtin_ctzll(last); }
    }
    r.carry = (uint32_t)hi;
    if (r.carry > r.best) { r.best = r.carry; r.first = p + 64 - hi; }
}

// the valid bits of the row's last word
__device__ __forceinline__ u64 last_valid(int32_t m, int32_t w64) {
    const int rem = m - 64 * (w64 - 1);
    return rem >= 64 ? ~0ull : (1ull << rem) - 1ull;
}

// A candidate under the rank is one number: the greater key is first, and of equal keys the lesser partner.  ~gap is at
// least 2^32 - 1 - 2^24, so a pair's key is never 0: key 0 with partner -1 is "no partner", last under the same compare.
__device__ __forceinline__ u64 rank_key(int by_gap, uint32_t count, uint32_t gap) {
    const u64 g = 0xFFFFFFFFull - gap;
    return by_gap ? (g << 32) | count : ((u64)count << 32) | g;
}
__device__ __forceinline__ PairPick no_partner() {
    PairPick r;
    r.key = 0ull; r.partner = -1; r.first = -1;
    return r;
}
// x becomes o if o is first under the rank: every field by the one decision
__device__ __forceinline__ void keep_first(PairPick& x, u64 key, int32_t partner, int32_t first) {
    const bool t = key > x.key || (key == x.key && partner < x.partner);
    x.key = t ? key : x.key;
    x.partner = t ? partner : x.partner;
    x.first = t ? first : x.first;
}
__device__ __forceinline__ PairRec record_of(int by_gap, const PairPick& x) {
    PairRec r;
    const uint32_t hi = (uint32_t)(x.key >> 32), lo = (uint32_t)x.key;
    r.partner = x.partner;
    r.count = x.partner < 0 ? 0u : by_gap ? lo : hi;
    r.gap = x.partner < 0 ? 0u : ~(by_gap ? hi : lo);
    r.gap_first = x.partner < 0 ? -1 : x.first;
    return r;
}

// Stage words [w0, w0 + wn) of `rows` rows from row0 on (rows past n_rows as zeros) at stride `stride` words.
__device__ __forceinline__ void stage(u64* s, int stride, const u64* t, int64_t row0, int rows, int64_t n_rows, int32_t w64, int32_t w0,
                                      int wn, int lane) {
    if (wn == CH) {
        for (int idx = lane; idx < rows * CH; idx += 64) {
            const int r = idx >> 5, w = idx & (CH - 1);
            s[r * stride + w] = row0 + r < n_rows ? t[(row0 + r) * w64 + w0 + w] : 0ull;
        }
    } else {
        for (int idx = lane; idx < rows * wn; idx += 64) {
            const int r = idx / wn, w = idx - r * wn;
            s[r * stride + w] = row0 + r < n_rows ? t[(row0 + r) * w64 + w0 + w] : 0ull;
        }
    }
}

template <int MODE>
__global__ void __launch_bounds__(64) pairs_kernel(const PairsC q, const int prune) {
    __shared__ u64 sa[TA * CH];
    __shared__ u64 sb[TB * BS];
    __shared__ u64 sbase[CH];
    __shared__ int32_t spa[TA * 3];
    const int lane = threadIdx.x;
    const int64_t a0 = (int64_t)blockIdx.x * TA;
    const int na = q.n_a - a0 < TA ? (int)(q.n_a - a0) : TA;
    const bool pos = q.pos_a != nullptr;
    const int32_t w64 = q.w64;
    const u64 vlast = last_valid(q.m, w64);
    const int64_t T = ((int64_t)q.n_b + TB - 1) / TB;
    const int64_t t_begin = blockIdx.y * T / q.splits, t_end = (blockIdx.y + 1) * T / q.splits;
    PairCell* cells = static_cast<PairCell*>(q.out);
    PairCell none;
    none.count = 0xFFFFFFFFu; none.gap = 0xFFFFFFFFu;

    PairBox qa;
    if (pos) {
        qa = q.box_a[blockIdx.x];
        if (lane < 3 * na) spa[lane] = clampc(q.pos_a[3 * a0 + lane]);
    }
    PairPick best[TA];
#pragma unroll
    for (int k = 0; k < TA; k++) best[k] = no_partner();
    uint32_t npairs = 0;
    bool a_staged = false;
    __syncthreads();

    // every cell of B tile t as ineligible
    auto blank = [&](int64_t t) {
        const int64_t b = t * TB + lane;
        if (b < q.n_b)
            for (int k = 0; k < na; k++) cells[(size_t)(a0 + k) * (size_t)q.n_b + (size_t)b] = none;
    };

    auto tile = [&](int64_t t) {
        const int64_t b = t * TB + lane;
        const bool bvalid = b < q.n_b;
        int32_t bx = 0, by = 0, bz = 0;
        if (pos && bvalid) { bx = clampc(q.pos_b[3 * b]); by = clampc(q.pos_b[3 * b + 1]); bz = clampc(q.pos_b[3 * b + 2]); }
        uint32_t elig = 0;
        for (int k = 0; k < na; k++) {
            bool e = bvalid && !(q.self && a0 + k == b);
            if (pos && e) {
                const int32_t dx = spa[3 * k] - bx, dy = spa[3 * k + 1] - by, dz = spa[3 * k + 2] - bz;
                const u64 d2 = (u64)((int64_t)dx * dx + (int64_t)dy * dy + (int64_t)dz * dz);
                e = d2 >= q.d2_min && d2 <= q.d2_max;
            }
            elig |= (uint32_t)e << k;
        }
        npairs += (uint32_t)__popc(elig);
        if (!__any(elig != 0u)) {               // the wave's decision: nothing to walk
            if (MODE == MRTX_PAIRS_TABLE) blank(t);
            return;
        }
        Run r[TA];
#pragma unroll
        for (int k = 0; k < TA; k++) { r[k].count = 0; r[k].carry = 0; r[k].best = 0; r[k].first = -1; }
        for (int32_t w0 = 0; w0 < w64; w0 += CH) {
            const int wn = w64 - w0 < CH ? w64 - w0 : CH;
            const bool restage = w64 > CH || !a_staged;         // a row of one chunk stays where it is
            __syncthreads();                                    // the last chunk has been read
            if (restage) {
                stage(sa, CH, q.a, a0, TA, q.n_a, w64, w0, wn, lane);
                if (lane < wn) sbase[lane] = q.base ? q.base[w0 + lane] : 0ull;
                a_staged = true;
            }
            stage(sb, BS, q.b, t * TB, TB, q.n_b, w64, w0, wn, lane);
            __syncthreads();
            for (int w = 0; w < wn; w++) {
                const u64 v = w0 + w == w64 - 1 ? vlast : ~0ull;
                const u64 bw = sb[lane * BS + w], bs = sbase[w];
                const int32_t p = (w0 + w) * 64;
#pragma unroll
                for (int k = 0; k < TA; k++) {
                    const u64 aw = sa[k * CH + w];
                    walk(r[k], ((q.op_and ? aw & bw : aw | bw) | bs) & v, v, p);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < TA; k++) {
            const bool e = (elig >> k) & 1u;
            if (MODE == MRTX_PAIRS_TABLE) {
                if (bvalid && k < na) {
                    PairCell c;
                    c.count = r[k].count; c.gap = r[k].best;
                    cells[(size_t)(a0 + k) * (size_t)q.n_b + (size_t)b] = e ? c : none;
                }
            } else {
                // an ineligible pair enters as "no partner", which is never first
                keep_first(best[k], e ? rank_key(q.by_gap, r[k].count, r[k].best) : 0ull, e ? (int32_t)b : -1, r[k].first);
            }
        }
    };

    for (int64_t t0 = t_begin; t0 < t_end; t0 += 64) {
        const int64_t t = t0 + lane;
        const bool mine = t < t_end;
        bool take = mine;
        if (pos && prune && mine) {
            const PairBox bb = q.box_b[t];
            take = !(box_near(qa, bb) > q.d2_max || box_far(qa, bb) < q.d2_min);
        }
        if (MODE == MRTX_PAIRS_TABLE)
            for (u64 s = __ballot(mine && !take); s; s &= s - 1ull) blank(t0 + __ffsll((long long)s) - 1);
        for (u64 s = __ballot(take); s; s &= s - 1ull) tile(t0 + __ffsll((long long)s) - 1);
    }

    if (MODE == MRTX_PAIRS_BEST) {
#pragma unroll
        for (int k = 0; k < TA; k++) {
            PairPick x = best[k];
            for (int d = 32; d >= 1; d >>= 1) {
                const uint32_t lo = __shfl_xor((uint32_t)x.key, d), hi = __shfl_xor((uint32_t)(x.key >> 32), d);
                const int32_t partner = __shfl_xor(x.partner, d), first = __shfl_xor(x.first, d);
                keep_first(x, ((u64)hi << 32) | lo, partner, first);
            }
            if (lane == 0 && k < na) {
                if (q.splits > 1) q.part[(size_t)(a0 + k) * (size_t)q.splits + blockIdx.y] = x;
                else static_cast<PairRec*>(q.out)[a0 + k] = record_of(q.by_gap, x);
            }
        }
    }
    u64 total = npairs;
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)total, d), hi = __shfl_xor((uint32_t)(total >> 32), d);
        total += ((u64)hi << 32) | lo;
    }
    if (lane == 0 && total) atomicAdd(q.pairs, total);
}

__global__ void __launch_bounds__(256) pairs_combine_kernel(const PairsC q) {
    const int64_t a = blockIdx.x * (int64_t)256 + threadIdx.x;
    if (a >= q.n_a) return;
    PairPick x = no_partner();
    for (int s = 0; s < q.splits; s++) {
        const PairPick o = q.part[(size_t)a * (size_t)q.splits + s];
        keep_first(x, o.key, o.partner, o.first);
    }
    static_cast<PairRec*>(q.out)[a] = record_of(q.by_gap, x);
}

__global__ void __launch_bounds__(64) pairs_rows_kernel(const PairsC q) {
    __shared__ u64 sb[TB * BS];
    __shared__ u64 sbase[CH];
    const int lane = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * TB, row = row0 + lane;
    const int32_t w64 = q.w64;
    const u64 vlast = last_valid(q.m, w64);
    Run r;
    r.count = 0; r.carry = 0; r.best = 0; r.first = -1;
    for (int32_t w0 = 0; w0 < w64; w0 += CH) {
        const int wn = w64 - w0 < CH ? w64 - w0 : CH;
        __syncthreads();
        stage(sb, BS, q.a, row0, TB, q.n_a, w64, w0, wn, lane);
        if (lane < wn) sbase[lane] = q.base ? q.base[w0 + lane] : 0ull;
        __syncthreads();
        for (int w = 0; w < wn; w++) {
            const u64 v = w0 + w == w64 - 1 ? vlast : ~0ull;
            walk(r, (sb[lane * BS + w] | sbase[w]) & v, v, (w0 + w) * 64);
        }
    }
    if (row < q.n_a) {
        PairRec c;
        c.partner = -1; c.count = r.count; c.gap = r.best; c.gap_first = r.first;
        static_cast<PairRec*>(q.out)[row] = c;
    }
}

}  // namespace mrtx_pr

static unsigned blocks_of(size_t n, unsigned per) { return (unsigned)((n + per - 1) / per); }

// ROWS: one launch.  BEST and TABLE: the pair launch, two box launches before it with positions (one when B is A's own table
// cut into other tiles: still two), and BEST's combine launch after it when B is shared out.  None depends on the data or on prune.
hipError_t mrtx_launch_mask_pairs(const PairsC& q, bool prune, hipStream_t st, uint32_t* launches) {
    using namespace mrtx_pr;
    if (q.n_a < 1 || q.m < 1 || q.w64 != (q.m + 63) / 64 || !q.a || !q.out || !q.pairs || !q.bad) return hipErrorInvalidValue;
    uint32_t n = 0;
    if (q.mode == MRTX_PAIRS_ROWS) {
        hipLaunchKernelGGL(pairs_rows_kernel, dim3(blocks_of((size_t)q.n_a, TB)), dim3(64), 0, st, q);
        n = 1;
    } else {
        if (q.mode != MRTX_PAIRS_BEST && q.mode != MRTX_PAIRS_TABLE) return hipErrorInvalidValue;
        const bool pos = q.pos_a != nullptr;
        const PairsLayout at = pairs_layout(q.n_a, q.n_b, true, q.mode == MRTX_PAIRS_BEST, pos);
        if (q.n_b < 1 || !q.b || q.splits != at.splits || (pos && (!q.pos_b || !q.box_a || !q.box_b))) return hipErrorInvalidValue;
        if (q.mode == MRTX_PAIRS_BEST && q.splits > 1 && !q.part) return hipErrorInvalidValue;
        if (pos) {
            hipLaunchKernelGGL(pairs_box_kernel, dim3(blocks_of(at.tiles_a, 256)), dim3(256), 0, st, q.pos_a, q.n_a, TA, q.box_a, q.bad);
            hipLaunchKernelGGL(pairs_box_kernel, dim3(blocks_of(at.tiles_b, 256)), dim3(256), 0, st, q.pos_b, q.n_b, TB, q.box_b,
                               q.self ? nullptr : q.bad);
            n += 2;
        }
        const dim3 grid((unsigned)at.tiles_a, (unsigned)q.splits);
        if (q.mode == MRTX_PAIRS_BEST) hipLaunchKernelGGL(pairs_kernel<MRTX_PAIRS_BEST>, grid, dim3(64), 0, st, q, prune ? 1 : 0);
        else hipLaunchKernelGGL(pairs_kernel<MRTX_PAIRS_TABLE>, grid, dim3(64), 0, st, q, prune ? 1 : 0);
        n++;
        if (q.mode == MRTX_PAIRS_BEST && q.splits > 1) {
            hipLaunchKernelGGL(pairs_combine_kernel, dim3(blocks_of((size_t)q.n_a, 256)), dim3(256), 0, st, q);
            n++;
        }
    }
    if (launches) *launches = n;
    return hipGetLastError();
}
