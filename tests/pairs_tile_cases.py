"""The shapes that give a workgroup of pairs_kernel more than one tile of B, shared by
test_pairs_tiles_host.py and test_gpu_pairs_tiles.py.  Every case exists at two scales: FULL, the kernel's own constants, and
SMALL, the same share structure under a smaller TA, TB, SPLIT_GROUPS and chunk, which the restated scheme (pairs_model.
walk_shares) walks pair by pair.  A case's builder and `Case.common_conditions` assert, from pairs_model.layout and the
reference pool_pairs alone, that its inputs hold what it is for.

Masks.  Rows are drawn from a pool of 16 (pairs_model.pool_pairs): ZERO and ONES; H1 and H2, whose union alone is complete;
Q1 and Q2, two clear epochs each, equal in count and gap and different in gap_first; and ten common rows, several of them equal in
(count, gap) against a given row of A.  B is drawn from ZERO and the common rows; H1, H2, Q1 and Q2 stand only where a case plants
them, so that the first partner of A's H1 rows (an H2: count m, gap 0, under either rank) and of its ZERO rows (a Q1 or Q2) lies
in the tiles the case is about.  Words carry garbage past epoch m - 1, and so does `base`.

Positions.  B's rows lie in compact blocks of one tile each, BLOCK apart on x, on a 10-unit lattice inside (d2 = 0, 100, 200,
400, ...); A's tile x lies on block x mod tiles_b (B is A itself: a row lies in the block of its B tile).  Under BOUNDS[0] = (100,
400), met exactly at both ends, only a tile's own block is in range and every other tile is provably out of it; a few far rows
blow their tiles' boxes up, so those tiles are looked at and found empty; BOUNDS[1] excludes every pair and BOUNDS[2] none."""
import numpy as np

import pairs_model as pm

FULL = dict(ta=pm.TA, tb=pm.TB, groups=pm.SPLIT_GROUPS, chunk=pm.CHUNK)
SMALL = dict(ta=2, tb=4, groups=16, chunk=2)
ZERO, ONES, H1, H2, Q1, Q2 = range(6)
COMMON = tuple(range(6, 16))
BOUNDS = ((100, 400), (1, 99), (0, 2 ** 64 - 1))
BLOCK = 1000


def pool(m, rng):
    """The 16 pool rows for m >= 40 epochs."""
    k = np.arange(m)
    q = m // 4
    rows = [pm.row(m, [(0, m)]), pm.row(m, []), pm.row(m, [(0, m // 2)]), pm.row(m, [(m // 2, m)]),
            pm.row(m, [(5, 6), (m - 6, m - 5)]), pm.row(m, [(7, 8), (m - 4, m - 3)]),
            pm.row(m, [(2, 8)]), pm.row(m, [(12, 18)]), pm.row(m, [(m - 8, m - 2)]),       # equal but for gap_first
            pm.row(m, [(2, 5), (20, 23)]),                                                  # the same count, another gap
            pm.row(m, [(10, 10 + q)]), pm.row(m, [(m // 3 + 3, m // 3 + 3 + q)]), k % 2 == 0, k % 3 != 0]
    for _ in range(2):
        s = int(rng.integers(0, m - 8))
        rows.append(pm.row(m, [(s, s + int(rng.integers(3, 8 + m // 3)))]) & (rng.random(m) < 0.9))
    assert len(rows) == pm.POOL_MAX
    rows = np.array(rows, bool)
    rows[len(rows) - len(COMMON):, [0, m - 1]] = False      # no common row completes H1 or H2
    return rows


class Case:
    """One call: ids and pool, the packed tables, positions, and the scale it is built for.  n_b == 0: B is A itself.
    plants: (B tile, lane, pool row) placed after the draw; tie: the two equal first partners b < b' of A's H1 rows, in one
    lane; late: the tile that holds the one H1 of B, the first partner of A's H2 rows."""

    def __init__(self, name, scale, n_a, n_b, m, plants, tie_tiles, late, seed=0, with_base=True):
        self.name, self.scale, self.n_a, self.n_b, self.m = name, dict(scale), n_a, n_b, m
        ta, tb = scale["ta"], scale["tb"]
        self.cols = n_b or n_a
        self.layout = pm.layout(n_a, self.cols, ta, tb, scale["groups"])
        rng = np.random.default_rng(seed)
        self.pool = pool(m, rng)
        ids_b = rng.choice(np.array(COMMON + (ZERO,)), self.cols)
        for t, lane, p in plants:
            assert t * tb + lane < self.cols
            ids_b[t * tb + lane] = p
        if n_b:
            ids_a = rng.integers(0, pm.POOL_MAX, n_a)
            for at, p in ((1, H1), (ta + 1, H2), (2 * ta, ZERO), (3 * ta + 1, ONES), (n_a - 1, H1), (n_a - 2, ZERO)):
                ids_a[at] = p
        else:
            ids_a = ids_b
        self.ids_a, self.ids_b = ids_a, (ids_b if n_b else None)
        words = pm.pack(self.pool)
        self.mask_a = pm.with_garbage(words[ids_a], m, rng)
        self.mask_b = pm.with_garbage(words[ids_b], m, rng) if n_b else None
        base_bits = np.zeros(m, bool)
        base_bits[[9, m // 2]] = True
        self.base = pm.with_garbage(pm.pack(base_bits), m, rng) if with_base else None
        # positions
        far_b = [tb + 3, self.cols // 2 + 1]
        pb = self.blocks(np.arange(self.cols) // tb, np.arange(self.cols) % tb, far_b, -1)
        if n_b:
            r = np.arange(n_a)
            self.pos_a, self.pos_b = self.blocks((r // ta) % self.layout.tiles_b, r % ta, [2 * ta + 1, n_a - 1], 1), pb
        else:
            self.pos_a, self.pos_b = pb, None
        self.far_a = far_b if not n_b else [2 * ta + 1, n_a - 1]
        self.tie = tuple(t * tb + 1 for t in tie_tiles)
        self.late = late

    @staticmethod
    def blocks(block, i, far, sign):
        pos = np.stack([BLOCK * block + 10 * (i % 8), 10 * (i // 8), 0 * i], -1).astype(np.int32)
        for j, r in enumerate(far):
            pos[r] = (-10 ** 6 * (j + 1), sign * 10 ** 6, 7)
        return pos

    def pos(self, bounds):
        """The position arguments of mask_pairs / pool_pairs / walk_shares."""
        return dict(positions_a=self.pos_a, positions_b=self.pos_b, d2_min=bounds[0], d2_max=bounds[1])

    def reference(self, op="any", mode="best", rank="count", bounds=None, stats=None):
        return pm.pool_pairs(self.ids_a, self.ids_b, self.pool, self.m, op=op, mode=mode, rank=rank, base=self.base, stats=stats,
                             **(self.pos(bounds) if bounds else {}))

    def references(self, calls, bounds=None, stats=None):
        """reference() for several (op, mode, rank) in one pass over the pairs."""
        return pm.pool_pairs_many(self.ids_a, self.ids_b, self.pool, self.m, calls, base=self.base, stats=stats,
                                  **(self.pos(bounds) if bounds else {}))

    def walk(self, op="any", rank="count", bounds=None, prune=True, mutant=None):
        return pm.walk_shares(self.ids_a, self.ids_b, self.pool, self.m, op=op, rank=rank, base=self.base, prune=prune,
                              mutant=mutant, **self.scale, **(self.pos(bounds) if bounds else {}))

    def share_of(self, t):
        return max(y for y in range(self.layout.splits) if self.layout.bounds[y] <= t)

    # ---- what the inputs hold, from the layout and the reference alone --------------------------------------------------------
    def common_conditions(self):
        """No share is a single-tile scheme in disguise; H1 rows of A tie between the two planted H2 and the reference takes the
        lesser; H2 rows of A find the one H1 of B in the late tile; ZERO rows of A tie between Q1 and Q2 where a case plants them
        (equal count and gap, the lesser b's gap_first); with BOUNDS[0] both ends are met exactly, far rows have no partner, for
        some A tile a share's first tile holds no eligible pair while a later one does, in one round of some workgroup the boxes
        prune some tiles and take others, and some taken tile is then found empty."""
        L, tb, ta = self.layout, self.scale["tb"], self.scale["ta"]
        assert L.splits < L.tiles_b and max(L.sizes) > 1, "some workgroup owns several tiles of B"
        ib = self.ids_a if self.ids_b is None else self.ids_b
        C, G, F = pm.pool_table(self.pool, self.pool, "any", pm.unpack(self.base, self.m) if self.base is not None else False)
        for rank in ("count", "gap"):
            ref = self.reference(rank=rank)
            b, b2 = self.tie
            assert b % tb == b2 % tb and b2 > b and ib[b] == ib[b2] == H2
            a = np.flatnonzero((self.ids_a == H1) & (ref["partner"] == b))
            assert len(a) and (ref["count"][a] == self.m).all() and (ref["gap"][a] == 0).all(), "the tie goes to the lesser b"
            a = np.flatnonzero(self.ids_a == H2)
            a = a[a != self.late * tb] if self.ids_b is None else a
            assert len(a) and (ref["partner"][a] == self.late * tb).all() and ib[self.late * tb] == H1
            q1, q2 = np.flatnonzero(ib == Q1), np.flatnonzero(ib == Q2)
            if len(q1):
                assert q1[0] % tb == q2[0] % tb and q1[0] < q2[0] and (C[ZERO, Q1], G[ZERO, Q1]) == (C[ZERO, Q2], G[ZERO, Q2])
                a = np.flatnonzero((self.ids_a == ZERO) & (ref["partner"] == q1[0]))
                assert len(a) and (ref["gap_first"][a] == F[ZERO, Q1]).all() and F[ZERO, Q1] != F[ZERO, Q2]
        lo, hi = BOUNDS[0]
        ref = self.reference(bounds=BOUNDS[0])
        assert (ref["partner"][self.far_a] == -1).all() and (ref["partner"] >= 0).any()
        met = dict(lo=False, hi=False, late_first=False, mixed=False, empty=False)
        box_a, box_b = pm.tile_boxes(self.pos_a, ta), pm.tile_boxes(self.pos_a if self.pos_b is None else self.pos_b, tb)
        # A's tiles repeat over B's blocks: two rounds of them and the last tile hold every kind
        for x in sorted(set(range(min(L.tiles_a, 2 * L.tiles_b + 3))) | {L.tiles_a - 1}):
            ok = pm.eligible_rows(x * ta, min((x + 1) * ta, self.n_a), self.cols, self.ids_b is None, self.pos_a, self.pos_b, lo, hi)
            d2 = pm.d2_table(self.pos_a[x * ta:(x + 1) * ta], self.pos_a if self.pos_b is None else self.pos_b)
            met["lo"] |= bool((d2 == lo).any())
            met["hi"] |= bool((d2 == hi).any())
            some = [bool(ok[:, t * tb:(t + 1) * tb].any()) for t in range(L.tiles_b)]
            take = [pm.box_takes(box_a[x], box_b[t], lo, hi) for t in range(L.tiles_b)]
            assert all(tk or not s for tk, s in zip(take, some)), "the boxes never prune an eligible pair"
            for y in range(L.splits):
                t0, t1 = L.bounds[y], L.bounds[y + 1]
                met["late_first"] |= not some[t0] and any(some[t0 + 1:t1])
                for r0 in range(t0, t1, tb):
                    r1 = min(r0 + tb, t1)
                    met["mixed"] |= not all(take[r0:r1]) and any(take[r0:r1])
                    met["empty"] |= any(tk and not s for tk, s in zip(take[r0:r1], some[r0:r1]))
        assert all(met.values()), met
        st = {}
        assert self.reference(bounds=BOUNDS[1], stats=st)["partner"].max() == -1 and st["pairs"] == 0


def case_a(scale, m_index):
    """Case A, uneven multi-tile shares, A x B.  FULL: n_a = 424 = 53 tiles of 8, so ceil(2048 / 53) = 39 workgroups per A tile
    are aimed at; n_b = 2 500 = 40 tiles of 64 (the last of 4 rows), one more than that, so splits = 39 and the shares y * 40 //
    39 hold one tile each but the last, which holds tiles 38 and 39.  It is the smallest B for these 53 A tiles at which a share
    holds two tiles: with 39 tiles or fewer splits == tiles_b.  m = 70, 64 * 32 and 64 * 32 + 70: the tail of one chunk, exactly
    one chunk (A stays staged over the share's two tiles) and two chunks (A's first chunk is staged again for the second tile).
    SMALL: 5 tiles of A, ceil(16 / 5) = 4, 5 tiles of B."""
    full = scale["tb"] == pm.TB
    n_a, n_b = (424, 2500) if full else (10, 19)
    m = ((70, 64 * 32, 64 * 32 + 70) if full else (40, 128, 168))[m_index]
    last = -(-n_b // scale["tb"]) - 1
    c = Case(f"A, m = {m}", scale, n_a, n_b, m, [(last - 1, 1, H2), (last, 1, H2), (last, 0, H1), (last - 1, 2, Q1), (last, 2, Q2)],
             (last - 1, last), last, seed=10 + m_index)
    L = c.layout
    assert L.splits == L.tiles_b - 1 and L.sizes == [1] * (L.splits - 1) + [2]
    w64, ch = pm.words_of(m), scale["chunk"]
    assert (w64 < ch, w64 == ch, ch < w64 <= 2 * ch)[m_index]
    assert c.share_of(c.tie[0] // scale["tb"]) == c.share_of(c.tie[1] // scale["tb"]) == L.splits - 1      # b and b + TB
    assert c.late == L.bounds[-1] - 1 and c.tie[1] - c.tie[0] == scale["tb"]       # the share's second tile holds the best
    return c


def case_b(scale):
    """Case B, multi-tile shares, B is A itself.  FULL: n = 2 000 = 250 tiles of A, ceil(2048 / 250) = 9, and 32 tiles of B
    (the last of 16 rows): splits = 9, the shares y * 32 // 9 hold 3 or 4 tiles.  With B = A, splits = ceil(2048 / ceil(n / 8)) falls as
    tiles_b = ceil(n / 64) grows: a share holds two tiles from n = 1 025 on and never fewer than three from n = 1 817 on,
    which the planted partners one tile apart and past their share's first tile need.  m = 129.  The
    diagonal falls in every share.  SMALL: n = 26 = 13 tiles of A, 2 shares of 3 and 4 tiles."""
    full = scale["tb"] == pm.TB
    n, m = (2000, 129) if full else (26, 100)
    t = pm.layout(n, n, scale["ta"], scale["tb"], scale["groups"]).bounds[1]
    c = Case("B", scale, n, 0, m, [(t + 1, 1, H2), (t + 2, 1, H2), (t + 2, 0, H1), (t + 1, 2, Q1), (t + 2, 2, Q2)], (t + 1, t + 2),
             t + 2, seed=20)
    L = c.layout
    assert len(set(L.sizes)) > 1 and min(L.sizes) >= 3, "uneven shares of several tiles"
    assert pm.words_of(m) <= scale["chunk"]
    diag = {c.share_of(a // scale["tb"]) for a in range(n)}                      # row a meets itself in B tile a // TB
    assert diag == set(range(L.splits))
    assert c.share_of(t + 1) == c.share_of(t + 2) == 1 and L.bounds[1] == t         # neither is its share's first tile
    return c


def case_c(scale):
    """Case C, two shares of several tiles.  FULL: n_a = 8 187 = 1 024 tiles of A, the last of 3 rows, so ceil(2048 / 1024) =
    2; n_b = 300 = 5 tiles (the last of 44 rows): shares [0, 2) and [2, 5).  1 024 is the least number of A tiles with two
    shares, and 5 B tiles the least that gives one of them three.  m = 70, no base.  SMALL: 8 tiles of A, the last of one row."""
    full = scale["tb"] == pm.TB
    n_a, n_b = (8187, 300) if full else (15, 19)
    c = Case("C", scale, n_a, n_b, 70, [(2, 1, H2), (4, 1, H2), (3, 0, H1), (0, 2, Q1), (1, 2, Q2)], (2, 4), 3, seed=30,
             with_base=False)
    assert c.layout.splits == 2 and c.layout.bounds == [0, 2, 5] and n_a % scale["ta"]
    return c


def case_d(scale):
    """Case D, splits == 1 with many B tiles: the direct write and the second round.  FULL: n_a = 16 380 = exactly 2 048 tiles
    of A (the last of 4 rows), from where on B is not shared out; n_b = 4 130 = 65 tiles, the last of 34 rows: one more than a
    round of 64.  A share of more than 64 tiles needs splits < tiles_b / 64, and with fewer than 2 048 tiles of A splits is at
    least 2, which takes 130 tiles of B against at least 1 024 of A: no shape reaches the second round with fewer than 2 048
    x 65 pairs of tiles, and this one reaches the direct write with them.  Both last tiles are ragged.  m = 70.  The planted H2 lie at b = 1 and b = 1 + 64 * 64, the one H1 at b = 4 096.  SMALL: 16 tiles of A, 5
    of B, rounds of 4."""
    full = scale["tb"] == pm.TB
    tb = scale["tb"]
    n_a, n_b = (16380, 4130) if full else (31, 18)
    c = Case("D", scale, n_a, n_b, 70, [(0, 1, H2), (tb, 1, H2), (tb, 0, H1), (1, 2, Q1), (3, 2, Q2)], (0, tb), tb, seed=40)
    L = c.layout
    assert L.splits == 1 and L.tiles_a == scale["groups"] and L.tiles_b == tb + 1
    assert c.tie[1] == c.tie[0] + tb * tb and c.late * tb == tb * tb
    # with positions: for A tile 0 the second round is pruned whole and some of the first taken; for A tile tb the reverse
    box_a, box_b = pm.tile_boxes(c.pos_a, scale["ta"]), pm.tile_boxes(c.pos_b, tb)
    lo, hi = BOUNDS[0]
    first = [pm.box_takes(box_a[0], box_b[t], lo, hi) for t in range(tb + 1)]
    second = [pm.box_takes(box_a[tb], box_b[t], lo, hi) for t in range(tb + 1)]
    assert first[0] and not first[tb] and second == [False] * tb + [True]
    return c


def case_e(scale, wide):
    """Case E, the edge at which B stops being shared out.  FULL: n_a = 16 376 = 2 047 tiles of A, so splits = 2 and a combine
    launch; n_a = 16 377 = 2 048 tiles, so splits = 1 and none.  n_b = 130 = 3 tiles (the last of 2 rows), m = 64, no base.  The
    first 16 376 rows are the same rows in both.  SMALL: 15 and 16 tiles of A (30 and 31 rows), 3 tiles of B."""
    full = scale["tb"] == pm.TB
    n_a = (16376 if full else 30) + bool(wide)
    c = Case(f"E, n_a = {n_a}", scale, (16377 if full else 31), (130 if full else 10), 64, [(1, 1, H2), (2, 1, H2), (2, 0, H1)],
             (1, 2), 2, seed=50, with_base=False)
    if not wide:                                            # the same rows, one fewer
        c.n_a, c.ids_a, c.mask_a, c.pos_a = n_a, c.ids_a[:n_a], c.mask_a[:n_a], c.pos_a[:n_a]
        c.far_a = c.far_a[:1]
        c.layout = pm.layout(n_a, c.cols, scale["ta"], scale["tb"], scale["groups"])
    assert c.layout.tiles_a == scale["groups"] - 1 + bool(wide) and c.layout.splits == (1 if wide else 2)
    return c


def all_cases(scale):
    """name -> case, built once per scale."""
    cases = [case_a(scale, 0), case_a(scale, 1), case_a(scale, 2), case_b(scale), case_c(scale), case_d(scale)]
    return {c.name: c for c in cases}
