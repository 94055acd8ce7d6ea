"""pairs_kernel's walk over several tiles of B without a GPU: the pool reference against the model pair
by pair, the restated layout against the header's constants, the restated tile scheme against the pool reference on every case
of pairs_tile_cases.py at reduced size, every named defect of the scheme told apart by a named case, and the full-size cases'
own conditions."""
import os
import re

import numpy as np
import pytest

import pairs_model as pm
import pairs_tile_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS, RANKS = ("any", "both"), ("count", "gap")


@pytest.fixture(scope="module")
def small():
    return tc.all_cases(tc.SMALL)


def test_the_layout_is_the_header_s():
    text = open(os.path.join(ROOT, "moonrtx_amd", "csrc", "mrtx_pairs.h")).read()
    const = {k: int(re.search(r"#define\s+MRTX_PAIRS_" + k + r"\s+(\d+)", text).group(1)) for k in ("TA", "TB", "SPLIT_GROUPS", "CHUNK")}
    assert (const["TA"], const["TB"], const["SPLIT_GROUPS"], const["CHUNK"]) == (pm.TA, pm.TB, pm.SPLIT_GROUPS, pm.CHUNK)
    assert tc.FULL == dict(ta=pm.TA, tb=pm.TB, groups=pm.SPLIT_GROUPS, chunk=pm.CHUNK)
    # pairs_layout's own sentences, on the header's numbers
    for n_a, n_b in ((1, 1), (200, 576), (424, 2500), (424, 2496), (2000, 2000), (8187, 300), (16376, 130), (16377, 130), (16380, 4130),
                     (8 * 2047, 64 * 5), (65536, 65536), (9, 64 * 300)):
        L = pm.layout(n_a, n_b)
        ta, tb = -(-n_a // const["TA"]), -(-n_b // const["TB"])
        want = 1 if ta >= const["SPLIT_GROUPS"] else max(1, min(-(-const["SPLIT_GROUPS"] // ta), tb))
        assert (L.tiles_a, L.tiles_b, L.splits) == (ta, tb, want), (n_a, n_b)
        assert L.bounds[0] == 0 and L.bounds[-1] == tb and len(L.bounds) == L.splits + 1
        assert all(L.bounds[y] == y * tb // L.splits for y in range(L.splits + 1)) and min(L.sizes) >= 1
    assert pm.layout(424, 2500).splits == 39 and pm.layout(424, 2496).splits == 39 == pm.layout(424, 2496).tiles_b
    assert pm.layout(2000, 2000).sizes == [3, 4, 3, 4, 3, 4, 3, 4, 4]
    assert pm.layout(8187, 300).bounds == [0, 2, 5] and pm.layout(16380, 4130).bounds == [0, 65]
    assert (pm.layout(16376, 130).splits, pm.layout(16377, 130).splits) == (2, 1)


def test_the_pool_reference_agrees_with_the_model_pair_by_pair():
    rng = np.random.default_rng(17)
    seen = dict(no_partner=0, ties=0)
    for trial in range(24):
        m = int(rng.choice([40, 64, 65, 130, 200]))
        pool = tc.pool(m, rng)
        same, with_pos, with_base = trial % 2 == 0, trial % 4 < 2, trial % 3 != 0
        n_a, n_b = int(rng.integers(1, 40)), int(rng.integers(1, 70))
        ids_a = rng.integers(0, len(pool), n_a)
        ids_b = None if same else rng.integers(0, len(pool), n_b)
        words = pm.pack(pool)
        A = pm.with_garbage(words[ids_a], m, rng)
        B = None if same else pm.with_garbage(words[ids_b], m, rng)
        base = pm.with_garbage(pm.pack(rng.random(m) < 0.1), m, rng) if with_base else None
        pos = {}
        if with_pos:
            pa = rng.integers(-4, 5, (n_a, 3)) * 10
            pa[0] = (10 ** 6, 0, -2 ** 29)                 # a row without an eligible partner
            pos = dict(positions_a=pa, positions_b=None if same else rng.integers(-4, 5, (n_b, 3)) * 10,
                       d2_min=(100, 0, 200)[trial % 3], d2_max=(400, 2 ** 64 - 1, 200)[trial % 3])
        for op in OPS:
            st, stm = {}, {}
            table = pm.pool_pairs(ids_a, ids_b, pool, m, op=op, mode="table", base=base, stats=st, **pos)
            want = pm.mask_pairs(A, m, mask_b=B, op=op, mode="table", base=base, stats=stm, **pos)
            assert table.dtype == want.dtype and np.array_equal(table, want) and st == stm
            for rank in RANKS:
                st = {}
                for block_cells in (1, 100, 1 << 22):       # the blocks of A rows are the reference's own business
                    got = pm.pool_pairs(ids_a, ids_b, pool, m, op=op, rank=rank, base=base, stats=st, block_cells=block_cells, **pos)
                    want = pm.mask_pairs(A, m, mask_b=B, op=op, rank=rank, base=base, **pos)
                    assert got.dtype == want.dtype and np.array_equal(got, want), (trial, op, rank)
                assert st["pairs"] == 3 * stm["pairs"]
                red = pm.reduce_table_fast(table, rank, m)
                slow = pm.reduce_table(table, np.full(table.shape, -1, np.int32), rank)
                assert np.array_equal(red, slow) and all(np.array_equal(red[f], got[f]) for f in ("partner", "count", "gap"))
                seen["no_partner"] += int((got["partner"] < 0).sum())
                seen["ties"] += int(sum((table["count"][a] == got["count"][a]).sum() > 1 for a in range(n_a)))
    assert min(seen.values()) > 20, seen


@pytest.mark.parametrize("name", ["A, m = 40", "A, m = 128", "A, m = 168", "B", "C", "D"])
def test_the_restated_scheme_agrees_with_the_pool_reference(small, name):
    c = small[name]
    c.common_conditions()
    for op in OPS:
        for bounds in (None,) + tc.BOUNDS:
            table = c.reference(op=op, mode="table", bounds=bounds)
            for rank in RANKS:
                st = {}
                ref = c.reference(op=op, rank=rank, bounds=bounds, stats=st)
                for prune in (True, False):
                    rec, tab, pairs, launches = c.walk(op=op, rank=rank, bounds=bounds, prune=prune)
                    assert np.array_equal(rec, ref) and np.array_equal(tab, table) and pairs == st["pairs"], (op, rank, bounds, prune)
                    assert launches == (2 if bounds else 0) + 1 + (c.layout.splits > 1)


def test_the_edge_where_b_stops_being_shared_out():
    narrow, wide = tc.case_e(tc.SMALL, False), tc.case_e(tc.SMALL, True)
    for bounds in (None, tc.BOUNDS[0]):
        for op in OPS:
            for rank in RANKS:
                got = [c.walk(op=op, rank=rank, bounds=bounds) for c in (narrow, wide)]
                assert [g[3] for g in got] == ([4, 3] if bounds else [2, 1])
                for c, g in zip((narrow, wide), got):
                    st = {}
                    assert np.array_equal(g[0], c.reference(op=op, rank=rank, bounds=bounds, stats=st)) and g[2] == st["pairs"]
                    assert np.array_equal(g[1], c.reference(op=op, mode="table", bounds=bounds))
                assert np.array_equal(got[0][0], got[1][0][:narrow.n_a])


# the case (at reduced size), and whether with positions, that is designed to show each defect, and in which of (records, TABLE,
# pairs) it must show
TOLD_BY = {"best_reset_per_tile": ("C", False, 0),                  # the first H2 lies two tiles before its share's last
           "tie_later_tile": ("A, m = 40", False, 0),               # b and b + TB in the two-tile share
           "run_not_reset": ("B", False, 1),                        # shares of 3 and 4 tiles: every cell after a share's first
           "second_round_lost": ("D", False, 0),                    # the one H1 of B lies in the tile after the first round
           "share_end_dropped": ("A, m = 128", False, 0),           # the two-tile share's second tile holds the one H1
           "share_bounds_even": ("A, m = 128", False, 0),           # T // splits = 1: the last tile is nobody's
           "combine_last_share_wins": ("B", False, 0),              # common rows tie across shares
           "a_stale_chunk": ("A, m = 168", False, 0),               # two chunks, and a second tile in the last share
           "a_never_staged_after_skip": ("B", True, 0),             # a block's own tile is rarely its share's first
           "skipped_tile_not_blanked": ("B", True, 1),
           "pairs_first_tile_only": ("C", False, 2)}


def test_every_named_tile_defect_is_told_apart_by_its_case(small):
    assert set(TOLD_BY) == set(pm.TILE_MUTANTS)
    for mu, (name, with_pos, part) in TOLD_BY.items():
        c = small[name]
        bounds = tc.BOUNDS[0] if with_pos else None
        shown = 0
        for op in OPS:
            for rank in RANKS:
                good, bad = c.walk(op=op, rank=rank, bounds=bounds), c.walk(op=op, rank=rank, bounds=bounds, mutant=mu)
                assert np.array_equal(good[0], c.reference(op=op, rank=rank, bounds=bounds))
                shown += not np.array_equal(good[part], bad[part])
        assert shown, (mu, name)
        # ... and what the GPU test compares with the reference sees it: the H1 / H2 / ZERO rows' records under "any"
        if part == 0 and mu not in ("combine_last_share_wins", "a_stale_chunk", "a_never_staged_after_skip"):
            bad = c.walk(mutant=mu)[0]
            rows = np.isin(c.ids_a, (tc.H1, tc.H2, tc.ZERO))
            assert not np.array_equal(bad[rows], c.reference()[rows]), mu


FULL_CASES = {"A, m = 70": lambda: tc.case_a(tc.FULL, 0), "A, m = 2048": lambda: tc.case_a(tc.FULL, 1),
              "A, m = 2118": lambda: tc.case_a(tc.FULL, 2), "B": lambda: tc.case_b(tc.FULL), "C": lambda: tc.case_c(tc.FULL),
              "D": lambda: tc.case_d(tc.FULL)}


@pytest.mark.parametrize("name", list(FULL_CASES))
def test_the_full_size_cases_hold_what_they_are_for(name):
    c = FULL_CASES[name]()
    assert c.name == name and c.scale == tc.FULL
    c.common_conditions()
    L = c.layout
    assert L.splits != L.tiles_b                            # no workgroup scheme the older tests already run
    if name == "D":
        ref = c.reference()
        assert (ref["partner"] >= 4096).any()               # some first partner lies in the second round
        a = np.flatnonzero(c.ids_a == tc.H1)
        assert (ref["partner"][a] == 1).all() and c.ids_b[1] == c.ids_b[1 + 4096] == tc.H2       # b before b + 4 096


def test_the_full_size_edge_cases():
    narrow, wide = tc.case_e(tc.FULL, False), tc.case_e(tc.FULL, True)
    assert (narrow.n_a, wide.n_a, narrow.n_b, narrow.m) == (16376, 16377, 130, 64)
    assert (narrow.layout.tiles_a, narrow.layout.splits, wide.layout.tiles_a, wide.layout.splits) == (2047, 2, 2048, 1)
    assert np.array_equal(narrow.mask_a, wide.mask_a[:16376]) and np.array_equal(narrow.pos_a, wide.pos_a[:16376])
    assert np.array_equal(narrow.reference(), wide.reference()[:16376])
