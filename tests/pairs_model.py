"""The model of mrtx_mask_pairs, and the kernel's word walk restated with named defects.

The definition works on unpacked booleans: `stats_loop` is the plain loop over one joint row, `row_stats` the same numbers for many
rows at once (test_pairs_host.py holds the two together), and `mask_pairs` is TerrainCalls.mask_pairs argument for argument, so
that a stub renderer can stand in for the device.  `word_walk` and `walk_pairs` restate what the kernels do -- 64-bit words,
chunks of CHUNK words, a carry from word to word, the three cases of a word of clear bits, the rank with its tie to the least
b -- and take one of MUTANTS, a deliberate defect each; `patterns` builds the rows that tell every one of them from the
correct walk.  `pool_pairs` is mask_pairs for rows drawn from a small pool, vectorised, for shapes of 10^8 pairs; `layout` and
`walk_shares` restate how pairs_kernel shares the tiles of B out and walks the several tiles of a share, and take one of
TILE_MUTANTS (tests/pairs_tile_cases.py builds the shapes that tell those apart)."""
import numpy as np

CHUNK = 32                      # words per LDS chunk: _lib.PAIRS_CHUNK_WORDS, csrc/mrtx_pairs.h's MRTX_PAIRS_CHUNK
PAIR_DTYPE = np.dtype([("partner", "<i4"), ("count", "<u4"), ("gap", "<u4"), ("gap_first", "<i4")])
PAIR_TABLE_DTYPE = np.dtype([("count", "<u4"), ("gap", "<u4")])
NONE = 0xFFFFFFFF
M64 = (1 << 64) - 1


def words_of(m):
    return (int(m) + 63) // 64


def pack(bits):
    """(..., m) booleans to (..., W64) uint64, the bits past m - 1 zero."""
    b = np.asarray(bits, bool)
    m = b.shape[-1]
    pad = np.zeros(b.shape[:-1] + (words_of(m) * 64,), np.uint8)
    pad[..., :m] = b
    return np.ascontiguousarray(np.packbits(pad, axis=-1, bitorder="little")).view("<u8")


def unpack(words, m):
    """(..., W64) uint64 to (..., m) booleans: whatever lies past epoch m - 1 is dropped."""
    w = np.ascontiguousarray(words, "<u8")
    assert w.shape[-1] == words_of(m), (w.shape, m)
    return np.unpackbits(w.view(np.uint8), axis=-1, bitorder="little")[..., :int(m)].astype(bool)


def with_garbage(words, m, rng):
    """A copy of the rows with random bits past epoch m - 1 (none when m is a multiple of 64)."""
    w = np.array(words, "<u8", copy=True)
    rem = int(m) % 64
    if rem:
        junk = rng.integers(0, 1 << 63, w.shape[:-1], dtype=np.uint64) * np.uint64(2) + np.uint64(1)
        w[..., -1] |= junk << np.uint64(rem)
    return w


# ---- the definition -------------------------------------------------------------------------------------------------------------
def stats_loop(bits):
    """(count, gap, gap_first) of one joint row of booleans, by the plain loop."""
    count = gap = run = 0
    first = -1
    for k, b in enumerate(bits):
        if b:
            count += 1
            run = 0
        else:
            run += 1
            if run > gap:
                gap, first = run, k - run + 1
    return count, gap, first


def row_stats(J):
    """count, gap, gap_first of every row of the (..., m) booleans J."""
    J = np.asarray(J, bool)
    m = J.shape[-1]
    idx = np.arange(m, dtype=np.int64)
    last_set = np.maximum.accumulate(np.where(J, idx, -1), axis=-1)
    run = idx - last_set                                    # the clear run that ends at each epoch, 0 where it is set
    gap = run.max(axis=-1)
    end = run.argmax(axis=-1)                               # the first epoch at which the longest run is complete
    first = np.where(gap > 0, end - gap + 1, -1)
    return J.sum(axis=-1).astype(np.uint32), gap.astype(np.uint32), first.astype(np.int32)


def d2_table(pos_a, pos_b):
    """(n_a, n_b) exact squared distances of int positions within +-2^29 (at most 3 x 2^60, so int64 holds them)."""
    a = np.asarray(pos_a, np.int64)[:, None, :]
    b = np.asarray(pos_b, np.int64)[None, :, :]
    d = a - b
    return (d * d).sum(-1)


def eligible(n_a, n_b, same, pos_a=None, pos_b=None, d2_min=0, d2_max=M64, exclusive=False):
    """(n_a, n_b) booleans: the pairs that count."""
    ok = np.ones((n_a, n_b), bool)
    if same:
        ok &= ~np.eye(n_a, dtype=bool)
    if pos_a is not None:
        d2 = d2_table(pos_a, pos_a if same else pos_b).astype(object)
        lo, hi = int(d2_min), int(d2_max)
        ok &= np.array([[(lo < v < hi) if exclusive else (lo <= v <= hi) for v in row] for row in d2], bool).reshape(n_a, n_b)
    return ok


def before(rank, c, g, b, c2, g2, b2):
    """Is (count c, gap g, partner b) first under the rank?"""
    k, k2 = ((-c, g) if rank == "count" else (g, -c)), ((-c2, g2) if rank == "count" else (g2, -c2))
    return (k, b) < (k2, b2)


def mask_pairs(mask_a, n_epochs, mask_b=None, op="any", mode="best", rank="count", base=None, positions_a=None,
               positions_b=None, d2_min=0, d2_max=M64, out=None, stats=None, **_ignored):
    """TerrainCalls.mask_pairs on the host: the same arguments, the same arrays, stats["pairs"] as well."""
    m = int(n_epochs)
    A = unpack(np.atleast_2d(np.asarray(mask_a, "<u8")), m)
    same = mask_b is None
    B = A if same else unpack(np.atleast_2d(np.asarray(mask_b, "<u8")), m)
    base_bits = np.zeros(m, bool) if base is None else unpack(np.asarray(base, "<u8").reshape(-1), m)
    n_a, n_b = A.shape[0], B.shape[0]
    if mode == "rows":
        c, g, f = row_stats(A | base_bits)
        rec = np.zeros(n_a, PAIR_DTYPE)
        rec["partner"], rec["count"], rec["gap"], rec["gap_first"] = -1, c, g, f
        if isinstance(stats, dict):
            stats["pairs"] = stats.get("pairs", 0) + n_a
        return rec
    ok = eligible(n_a, n_b, same, positions_a, positions_b, d2_min, d2_max)
    table = np.zeros((n_a, n_b), PAIR_TABLE_DTYPE)
    rec = np.zeros(n_a, PAIR_DTYPE)
    for a in range(n_a):
        J = ((A[a] | B) if op == "any" else (A[a] & B)) | base_bits
        c, g, f = row_stats(J)
        table["count"][a] = np.where(ok[a], c, NONE)
        table["gap"][a] = np.where(ok[a], g, NONE)
        pick = (-1, 0, 0, -1)
        for b in np.flatnonzero(ok[a]):
            if pick[0] < 0 or before(rank, int(c[b]), int(g[b]), int(b), pick[1], pick[2], pick[0]):
                pick = (int(b), int(c[b]), int(g[b]), int(f[b]))
        rec[a] = pick
    if isinstance(stats, dict):
        stats["pairs"] = stats.get("pairs", 0) + int(ok.sum())
    return table if mode == "table" else rec


def reduce_table(table, first, rank):
    """BEST from a TABLE and the (n_a, n_b) gap_first of its pairs: the reduction the device must agree with."""
    n_a, n_b = table.shape
    rec = np.zeros(n_a, PAIR_DTYPE)
    for a in range(n_a):
        pick = (-1, 0, 0, -1)
        for b in range(n_b):
            c, g = int(table["count"][a, b]), int(table["gap"][a, b])
            if c == NONE and g == NONE:
                continue
            if pick[0] < 0 or before(rank, c, g, b, pick[1], pick[2], pick[0]):
                pick = (b, c, g, int(first[a, b]))
        rec[a] = pick
    return rec


# ---- the kernel's scheme, restated, with named defects -------------------------------------------------------------------------
MUTANTS = ("no_carry",              # every word starts a new run: no carry across words
           "chunk_carry_lost",      # the carry is dropped at the first word of every chunk
           "later_of_equals",       # >= where > belongs: the later of equal runs is taken
           "garbage_counted",       # the bits past m - 1 are counted
           "last_word_open",        # the last word's clear bits past m - 1 extend the gap
           "interior_missed",       # a mixed word's runs strictly inside it are not looked for
           "d2_exclusive",          # d2_min < d2 < d2_max
           "tie_later_b")           # the later of equal partners is taken


def ctz(x):
    return (x & -x).bit_length() - 1


def clz(x):
    return 64 - x.bit_length()


def word_walk(words, m, chunk=CHUNK, mutant=None):
    """(count, gap, gap_first) of one row of joint words (Python ints or uint64, base and op applied, not yet masked), word by
    word as pairs_kernel does."""
    w64 = words_of(m)
    rem = m - 64 * (w64 - 1)
    count = carry = best = 0
    first = -1

    def take(run, start):
        nonlocal best, first
        if run > best or (mutant == "later_of_equals" and run == best and run > 0):
            best, first = run, start

    for w in range(w64):
        v = M64 if w < w64 - 1 or rem == 64 else (1 << rem) - 1
        j = int(words[w])
        count += bin(j if mutant == "garbage_counted" else j & v).count("1")
        z = ~j & (M64 if mutant == "last_word_open" else v) & M64
        p = 64 * w
        if mutant == "no_carry" or (mutant == "chunk_carry_lost" and w % chunk == 0):
            carry = 0
        if z == 0:
            carry = 0
            continue
        if z == M64:
            carry += 64
            take(carry, p + 64 - carry)
            continue
        lo, hi = ctz(~z & M64), clz(~z & M64)
        take(carry + lo, p - carry)
        x = z & ~((1 << lo) - 1) & (M64 >> hi)
        if x and mutant != "interior_missed":
            n = 0
            while x:
                last, x, n = x, x & (x >> 1), n + 1
            take(n, p + ctz(last))
        carry = hi
        take(carry, p + 64 - hi)
    return count, best, first


def walk_pairs(mask_a, n_epochs, mask_b=None, op="any", rank="count", base=None, positions_a=None, positions_b=None,
               d2_min=0, d2_max=M64, chunk=CHUNK, mutant=None):
    """BEST by the kernel's scheme: (records, TABLE, pairs)."""
    m = int(n_epochs)
    A = np.atleast_2d(np.asarray(mask_a, "<u8"))
    same = mask_b is None
    B = A if same else np.atleast_2d(np.asarray(mask_b, "<u8"))
    w64 = words_of(m)
    bs = [0] * w64 if base is None else [int(x) for x in np.asarray(base, "<u8").reshape(-1)]
    n_a, n_b = A.shape[0], B.shape[0]
    ok = eligible(n_a, n_b, same, positions_a, positions_b, d2_min, d2_max, exclusive=mutant == "d2_exclusive")
    rec = np.zeros(n_a, PAIR_DTYPE)
    table = np.zeros((n_a, n_b), PAIR_TABLE_DTYPE)
    table["count"], table["gap"] = NONE, NONE
    for a in range(n_a):
        pick = (-1, 0, 0, -1)
        for b in range(n_b):
            if not ok[a, b]:
                continue
            aw, bw = [int(x) for x in A[a]], [int(x) for x in B[b]]
            joint = [((x | y) if op == "any" else (x & y)) | s for x, y, s in zip(aw, bw, bs)]
            c, g, f = word_walk(joint, m, chunk, mutant)
            table[a, b] = (c & NONE, g)
            tie = mutant == "tie_later_b" and pick[0] >= 0 and (c, g) == (pick[1], pick[2])
            if pick[0] < 0 or tie or before(rank, c, g, b, pick[1], pick[2], pick[0]):
                pick = (b, c, g, f)
        rec[a] = (pick[0], pick[1] & NONE, pick[2], pick[3])
    return rec, table, int(ok.sum())


# ---- the designed patterns ---------------------------------------------------------------------------------------------------
def row(m, clear):
    """m booleans, all set but the half-open intervals of `clear`, clipped to [0, m)."""
    r = np.ones(m, bool)
    for s, e in clear:
        r[max(s, 0):max(min(e, m), 0)] = False
    return r


def patterns(m, chunk=CHUNK):
    """The designed rows for m epochs, (n, m) booleans: all clear and all set; a gap touching epoch 0 and one touching m - 1; a
    gap ending exactly at a word edge and one starting there; a gap spanning three words; two equal longest gaps; an interior
    gap inside a mixed word, longer than its leading and trailing runs; gaps that end at, start at and cross the chunk edge, two
    equal ones of which the later crosses it; and complementary rows whose union is full."""
    E = 64 * chunk
    k = np.arange(m)
    rows = [row(m, []), row(m, [(0, m)]), row(m, [(0, 5)]), row(m, [(m - 5, m)]), row(m, [(m - 1, m)]), row(m, [(0, 1)]),
            row(m, [(50, 64)]), row(m, [(64, 80)]), row(m, [(60, 135)]), row(m, [(3, 10), (20, 27)]),
            row(m, [(3, 10), (70, 77)]), row(m, [(0, 2), (10, 20), (62, 64)]), row(m, [(64, 67), (80, 95), (125, 128)]),
            row(m, [(0, 3), (10, 20), (61, 70)]), row(m, [(E - 30, E + 30)]), row(m, [(E - 64, E)]), row(m, [(E, E + 64)]),
            row(m, [(E - 100, E - 36), (E - 20, E + 44)]), row(m, [(m - 70, m - 40), (m - 30, m)]),
            k % 2 == 0, k % 2 == 1, k < m // 2, k >= m // 2]
    return np.array(rows, bool)


# ---- a reference that can afford 10^8 pairs: rows drawn from a small pool ------------------------------------------------------
POOL_MAX = 16
I64_MAX = (1 << 63) - 1


def pool_table(pool_a, pool_b, op, base_bits):
    """(Pa, Pb) count, gap and gap_first of every row of pool_a against every row of pool_b: row_stats on unpacked booleans."""
    A, B = np.asarray(pool_a, bool), np.asarray(pool_b, bool)
    J = (A[:, None, :] | B[None, :, :]) if op == "any" else (A[:, None, :] & B[None, :, :])
    return row_stats(J | np.asarray(base_bits, bool))


def rank_number(count, gap, rank, m):
    """One int64 per (count, gap) whose ascending order is the rank's: the lesser number is first.  count and gap are at most m
    <= 2^24, so the number stays below 2^52."""
    c, g = np.asarray(count, np.int64), np.asarray(gap, np.int64)
    return ((m - c) * (m + 1) + g) if rank == "count" else (g * (m + 1) + (m - c))


def eligible_rows(a0, a1, n_b, same, pos_a=None, pos_b=None, d2_min=0, d2_max=M64):
    """(a1 - a0, n_b) booleans: the eligible partners of rows a0 .. a1 - 1, by the exact int64 d2 (at most 3 x 2^60) and, when
    B is A itself, without the diagonal."""
    ok = np.ones((a1 - a0, n_b), bool)
    if same:
        ok[np.arange(a1 - a0), np.arange(a0, a1)] = False
    if pos_a is not None:
        pa, pb = np.asarray(pos_a, np.int64), np.asarray(pos_a if same else pos_b, np.int64)
        d2 = np.zeros((a1 - a0, n_b), np.int64)
        for k in range(3):
            d = pa[a0:a1, k, None] - pb[None, :, k]
            d2 += d * d
        lo, hi = int(d2_min), int(d2_max)
        ok &= (d2 >= lo) & (d2 <= min(hi, I64_MAX)) if lo <= I64_MAX else False
    return ok


def pool_pairs_many(ids_a, ids_b, pool_bits, m, calls, base=None, positions_a=None, positions_b=None, d2_min=0, d2_max=M64,
                    stats=None, block_cells=1 << 22):
    """pool_pairs for several (op, mode, rank) at once: the eligibility of a block of A rows is worked out once for all of
    them.  A list of results in the order of `calls`; stats["pairs"] grows once."""
    m = int(m)
    pool = np.asarray(pool_bits, bool)
    assert pool.ndim == 2 and pool.shape[1] == m and len(pool) <= POOL_MAX and all(c[1] in ("best", "table") for c in calls)
    ia = np.asarray(ids_a, np.intp)
    same = ids_b is None
    ib = ia if same else np.asarray(ids_b, np.intp)
    n_a, n_b = len(ia), len(ib)
    base_bits = np.zeros(m, bool) if base is None else unpack(np.asarray(base, "<u8").reshape(-1), m)
    never = np.int64(I64_MAX)
    work = []
    for op, mode, rank in calls:
        C, G, F = pool_table(pool, pool, op, base_bits)
        if mode == "table":
            work.append((mode, C[:, ib], G[:, ib], np.empty((n_a, n_b), PAIR_TABLE_DTYPE)))     # (P, n_b): a pool row of A
        else:                                                                                   # against every row of B
            rec = np.zeros(n_a, PAIR_DTYPE)
            rec["partner"], rec["gap_first"] = -1, -1
            work.append((mode, rank_number(C, G, rank, m)[:, ib], (C, G, F), rec))
    pairs = 0
    step = max(1, block_cells // n_b)
    for a0 in range(0, n_a, step):
        a1 = min(a0 + step, n_a)
        ok = eligible_rows(a0, a1, n_b, same, positions_a, positions_b, d2_min, d2_max)
        pairs += int(ok.sum())
        ida = ia[a0:a1]
        for mode, x, y, out in work:
            if mode == "table":
                out["count"][a0:a1] = np.where(ok, x[ida], NONE)
                out["gap"][a0:a1] = np.where(ok, y[ida], NONE)
                continue
            b = np.where(ok, x[ida], never).argmin(axis=1)
            has = ok[np.arange(a1 - a0), b]
            pa, pb = ida[has], ib[b[has]]
            at = np.arange(a0, a1)[has]
            out["partner"][at], out["count"][at], out["gap"][at], out["gap_first"][at] = b[has], y[0][pa, pb], y[1][pa, pb], y[2][pa, pb]
    if isinstance(stats, dict):
        stats["pairs"] = stats.get("pairs", 0) + pairs
    return [w[3] for w in work]


def pool_pairs(ids_a, ids_b, pool_bits, m, op="any", mode="best", rank="count", base=None, positions_a=None, positions_b=None,
               d2_min=0, d2_max=M64, stats=None, block_cells=1 << 22):
    """mask_pairs (BEST and TABLE) for rows drawn from a pool of at most POOL_MAX distinct rows: row a is pool_bits[ids_a[a]],
    row b pool_bits[ids_b[b]] (ids_b None: the rows of A against each other).  A pair's record is a gather from the pool's own
    P x P table; eligibility is the exact d2 by blocks of A rows; BEST is the least (rank number, b) of a row's eligible pairs
    (numpy's argmin returns the first of equal minima: the least b).  It knows nothing of tiles, lanes, shares or chunks."""
    return pool_pairs_many(ids_a, ids_b, pool_bits, m, [(op, mode, rank)], base, positions_a, positions_b, d2_min, d2_max, stats,
                           block_cells)[0]


def reduce_table_fast(table, rank, m):
    """reduce_table's partner, count and gap, vectorised: per row the least (rank number, b) of the cells that are not all ones."""
    n_a, n_b = table.shape
    rec = np.zeros(n_a, PAIR_DTYPE)
    rec["partner"], rec["gap_first"] = -1, -1
    step = max(1, (1 << 22) // n_b)
    for a0 in range(0, n_a, step):
        c, g = table["count"][a0:a0 + step], table["gap"][a0:a0 + step]
        ok = ~((c == NONE) & (g == NONE))
        x = np.where(ok, rank_number(np.where(ok, c, 0), np.where(ok, g, 0), rank, m), np.int64(I64_MAX))
        b = x.argmin(axis=1)
        k = np.arange(len(b))
        has = ok[k, b]
        at = a0 + k[has]
        rec["partner"][at], rec["count"][at], rec["gap"][at] = b[has], c[k, b][has], g[k, b][has]
    return rec


# ---- the kernel's tile scheme, restated, with named defects ----------------------------------------------------------------------
TA, TB, SPLIT_GROUPS = 8, 64, 2048      # csrc/mrtx_pairs.h's MRTX_PAIRS_TA, MRTX_PAIRS_TB and MRTX_PAIRS_SPLIT_GROUPS
UNWRITTEN = 0xA5A5A5A5                  # what a TABLE cell holds that no workgroup wrote

TILE_MUTANTS = ("best_reset_per_tile",          # a lane's candidates start anew at every tile: only the last walked tile counts
                "tie_later_tile",               # of equal partners in one lane the later tile's wins
                "run_not_reset",                # a pair's count starts from the previous walked tile's
                "second_round_lost",            # only the first round of tiles of a share is walked
                "share_end_dropped",            # the last tile of a share of several tiles is not walked
                "share_bounds_even",            # every share holds T // splits tiles: the remainder is nobody's
                "combine_last_share_wins",      # of equal partial candidates the later share's wins
                "a_stale_chunk",                # w64 > chunk: tiles after a workgroup's first walked one see A's (and base's) last
                                                # chunk where the first belongs
                "a_never_staged_after_skip",    # w64 <= chunk: A and base are staged at the share's first tile only, so a share
                                                # whose first tile is skipped walks zeros
                "skipped_tile_not_blanked",     # TABLE: the cells of a pruned or empty tile are left as they were
                "pairs_first_tile_only")        # the eligible pairs of a share's first tile only are counted


class Layout:
    """pairs_layout's tiling of a BEST or TABLE call: tiles of ta rows of A and tb rows of B; `splits` workgroups per A tile,
    of which share y owns B's tiles bounds[y] .. bounds[y + 1] - 1."""

    def __init__(self, n_a, n_b, ta=TA, tb=TB, groups=SPLIT_GROUPS):
        self.tiles_a, self.tiles_b = -(-n_a // ta), -(-n_b // tb)
        s = 1
        if self.tiles_a < groups:
            s = max(1, min(-(-groups // self.tiles_a), self.tiles_b))
        self.splits = s
        self.bounds = [y * self.tiles_b // s for y in range(s + 1)]
        self.sizes = [self.bounds[y + 1] - self.bounds[y] for y in range(s)]


def layout(n_a, n_b, ta=TA, tb=TB, groups=SPLIT_GROUPS):
    return Layout(n_a, n_b, ta, tb, groups)


def tile_boxes(pos, tile):
    """Per tile of `tile` rows the bounding box (lo[3], hi[3]) of their positions."""
    p = np.asarray(pos, np.int64)
    return [(p[r:r + tile].min(axis=0).tolist(), p[r:r + tile].max(axis=0).tolist()) for r in range(0, len(p), tile)]


def box_takes(p, b, d2_min, d2_max):
    """May a point of box p and one of box b be d2_min <= d2 <= d2_max apart?  The prune bound: the least possible d2 (per
    axis the gap between the boxes) and the greatest (per axis the larger far-corner difference)."""
    near = sum(max(b[0][k] - p[1][k], p[0][k] - b[1][k], 0) ** 2 for k in range(3))
    far = sum(max(b[1][k] - p[0][k], p[1][k] - b[0][k]) ** 2 for k in range(3))
    return not (near > d2_max or far < d2_min)


def stale_words(words, chunk):
    """What the first chunk's place in LDS holds after a walk over every chunk: per word index the word of the last chunk
    that has one there."""
    w = np.array(words, "<u8", copy=True)
    w64 = w.shape[-1]
    n = -(-w64 // chunk)
    last = w64 - (n - 1) * chunk
    for k in range(min(chunk, w64)):
        w[..., k] = np.asarray(words)[..., ((n - 1) if k < last else (n - 2)) * chunk + k]
    return w


def first_of(x, o, later_of_equals=False):
    """keep_first: the candidate (number, partner, count, gap, first) o or x, whichever is first; None is "no partner"."""
    if o is None:
        return x
    if x is None or o[0] < x[0]:
        return o
    if o[0] == x[0] and ((o[1] > x[1]) if later_of_equals else (o[1] < x[1])):
        return o
    return x


def walk_shares(ids_a, ids_b, pool_bits, m, op="any", rank="count", base=None, positions_a=None, positions_b=None, d2_min=0,
                d2_max=M64, prune=True, ta=TA, tb=TB, groups=SPLIT_GROUPS, chunk=CHUNK, mutant=None):
    """BEST and TABLE by pairs_kernel's tile scheme: (records, TABLE, pairs, BEST's launches).  A workgroup per (A tile, share)
    of tb lanes; rounds of tb tiles, in which lane j decides by the boxes whether tile t0 + j is taken; the taken tiles one
    after the other, lane j owning row b = tb * t + j against the ta rows of A; a tile in which no lane has an eligible pair is
    not walked; per lane one candidate per A row over its tiles, the wave's first of them, then the first over the shares in
    ascending order.  A pair's record is a gather from the pool's table: the word walk is word_walk's business."""
    m = int(m)
    assert mutant is None or mutant in TILE_MUTANTS
    pool = np.asarray(pool_bits, bool)
    ia = [int(i) for i in ids_a]
    same = ids_b is None
    ib = ia if same else [int(i) for i in ids_b]
    n_a, n_b = len(ia), len(ib)
    w64 = words_of(m)
    base_w = np.zeros(w64, "<u8") if base is None else np.asarray(base, "<u8").reshape(-1)
    tables = {}

    def stats_of(variant):
        if variant not in tables:
            if variant == "staged":
                A, bw = pool, base_w
            elif variant == "stale":
                A, bw = unpack(stale_words(pack(pool), chunk), m), stale_words(base_w, chunk)
            else:
                A, bw = np.zeros_like(pool), np.zeros(w64, "<u8")
            c, g, f = pool_table(A, pool, op, unpack(bw, m))
            tables[variant] = (c.tolist(), g.tolist(), f.tolist())
        return tables[variant]

    def number(c, g):                                       # rank_number in Python integers: a defect's count may pass m
        big = m * (n_b + 1)
        return (big - c) * (big + 1) + g if rank == "count" else g * (big + 1) + (big - c)

    L = layout(n_a, n_b, ta, tb, groups)
    T, splits = L.tiles_b, L.splits
    pos = positions_a is not None
    lo, hi = int(d2_min), int(d2_max)
    if pos:
        pa = np.asarray(positions_a, np.int64).tolist()
        pb = pa if same else np.asarray(positions_b, np.int64).tolist()
        box_a, box_b = tile_boxes(pa, ta), tile_boxes(pb, tb)
    table = np.zeros((n_a, n_b), PAIR_TABLE_DTYPE)
    table["count"], table["gap"] = UNWRITTEN, UNWRITTEN
    part = [[None] * splits for _ in range(n_a)]
    pairs = 0

    for x in range(L.tiles_a):
        a0 = x * ta
        na = min(ta, n_a - a0)
        for y in range(splits):
            t_begin, t_end = L.bounds[y], L.bounds[y + 1]
            if mutant == "share_bounds_even":
                t_begin, t_end = y * (T // splits), (y + 1) * (T // splits)
            if mutant == "share_end_dropped" and t_end - t_begin > 1:
                t_end -= 1
            best = [[None] * ta for _ in range(tb)]
            prev = [[0] * ta for _ in range(tb)]            # run_not_reset: what the last walked tile left in the registers
            a_staged = False
            walked = 0

            def blank(t):
                if mutant != "skipped_tile_not_blanked":
                    table[a0:a0 + na, t * tb:min((t + 1) * tb, n_b)] = (NONE, NONE)

            def tile(t):
                nonlocal pairs, a_staged, walked
                elig = []
                for lane in range(tb):
                    b = t * tb + lane
                    e = [b < n_b and not (same and a0 + k == b) for k in range(na)]
                    if pos and b < n_b:
                        e = [ek and lo <= sum((u - v) ** 2 for u, v in zip(pa[a0 + k], pb[b])) <= hi for k, ek in enumerate(e)]
                    elig.append(e)
                if not (mutant == "pairs_first_tile_only" and t != t_begin):
                    pairs += sum(map(sum, elig))
                if not any(map(any, elig)):
                    blank(t)
                    return
                variant = "staged"
                if w64 > chunk:
                    if mutant == "a_stale_chunk" and walked:
                        variant = "stale"
                elif not a_staged:
                    if mutant == "a_never_staged_after_skip" and t != t_begin:
                        variant = "never"
                    else:
                        a_staged = True
                walked += 1
                C, G, F = stats_of(variant)
                for lane in range(tb):
                    b = t * tb + lane
                    if mutant == "best_reset_per_tile":
                        best[lane] = [None] * ta
                    if b >= n_b:
                        continue
                    for k in range(na):
                        i, j = ia[a0 + k], ib[b]
                        c, g, f = C[i][j], G[i][j], F[i][j]
                        if mutant == "run_not_reset":
                            c += prev[lane][k]
                            prev[lane][k] = c
                        table[a0 + k, b] = (c, g) if elig[lane][k] else (NONE, NONE)
                        if elig[lane][k]:
                            best[lane][k] = first_of(best[lane][k], (number(c, g), b, c, g, f), mutant == "tie_later_tile")

            for t0 in range(t_begin, t_end, tb):
                if mutant == "second_round_lost" and t0 > t_begin:
                    break
                mine = range(t0, min(t0 + tb, t_end))
                take = [not (pos and prune) or box_takes(box_a[x], box_b[t], lo, hi) for t in mine]
                for t, tk in zip(mine, take):
                    if not tk:
                        blank(t)
                for t, tk in zip(mine, take):
                    if tk:
                        tile(t)
            for k in range(na):
                cand = None
                for lane in range(tb):
                    cand = first_of(cand, best[lane][k])
                part[a0 + k][y] = cand

    rec = np.zeros(n_a, PAIR_DTYPE)
    for a in range(n_a):
        cand = None
        for y in range(splits):                             # with one share the pair kernel writes the record itself
            cand = first_of(cand, part[a][y], mutant == "combine_last_share_wins")
        rec[a] = (-1, 0, 0, -1) if cand is None else cand[1:]
    return rec, table, pairs, (2 if pos else 0) + 1 + (1 if splits > 1 else 0)
