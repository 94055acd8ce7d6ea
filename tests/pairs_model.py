"""The model of mrtx_mask_pairs, and the kernel's word walk restated with named defects.

The definition works on unpacked booleans: `stats_loop` is the plain loop over one joint row, `row_stats` the same numbers for many
rows at once (test_pairs_host.py holds the two together), and `mask_pairs` is TerrainCalls.mask_pairs argument for argument, so
that a stub renderer can stand in for the device.  `word_walk` and `walk_pairs` restate what the kernels do -- 64-bit words,
chunks of CHUNK words, a carry from word to word, the three cases of a word of clear bits, the rank with its tie to the least
b -- and take one of MUTANTS, a deliberate defect each; `patterns` builds the rows that tell every one of them from the
correct walk."""
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
