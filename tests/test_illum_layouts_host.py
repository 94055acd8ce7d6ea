"""The illumination stage's wave layouts without a GPU (tests/illum_layout_cases.py; DESIGN.md sections 4.8 and 4.9): the
restated lane map holds every (node, sample) of every case exactly once and reports the float64 model's lit; the launch rule
gives the documented PW x PH at every n_sun and the window lengths reach every branch of the series' narrowing; the built
scene keeps the GPU comparison from being vacuous (the caps); and the cases tell every named defect of the mapping from the
true one at every n_sun where it is one."""
import numpy as np
import pytest

import illum_layout_cases as lc
import illum_model as im

# where a defect is none: the mutant's lane map and everything it reports equal the true mapping's in every case
IDENTITY = {("pw_ph_swapped", 64),              # 1 x 1, and one node per wave in a one-row band
            ("one_row_ignored", 32),            # the grid's 2 x 1 is the one-row block already
            ("one_row_ignored", 64),
            ("sample_shifted", 1),              # one sample: every index is 0
            ("series_pw_not_narrowed", 64),     # one (point, epoch) per wave: nothing to narrow
            ("edge_lanes_not_zeroed", 64)}      # one node per wave: no wave reaches past an edge
# edge_lanes_not_zeroed cannot show in lit at any n_sun: a node's n_sun lanes are inside or past the edge together, so a
# group_sum over n_sun lanes never mixes the two.  What the stray lanes feed is the wave-wide sum of the counters: the defect
# shows in shadow_rays (asserted below), which is why the GPU tests compare that counter with the model's in every case.
COUNTER_ONLY = ("edge_lanes_not_zeroed",)


def grid_cases():
    """[(name, kind, rows, cols, n_sun -> (V, cos_pos, flagged) flat over the nodes)]"""
    out = []
    for shape in lc.SHAPES:
        m = lc.grid_model(shape)
        out.append((f"grid {shape}", "grid", shape[0], shape[1], {n: (m[n]["V"], m[n]["cos_pos"], m[n]["flagged"]) for n in lc.N_SUN}))
    return out


def all_cases(n_sun):
    """The grid cases and n_sun's series cases: (name, kind, rows, cols, V, cos_pos, flagged)."""
    out = [(name, kind, r, c, *tabs[n_sun]) for name, kind, r, c, tabs in grid_cases()]
    sm = lc.series_model()[n_sun]
    for name, n, k, first, count in lc.series_cases():
        if n == n_sun:
            tabs = [lc.series_window(sm[key], k, first, count).reshape(k * count, n) for key in ("V", "cos_pos", "flagged")]
            out.append((name, "series", k, count, *tabs))
    return out


def test_the_side_by_side_model_is_the_model_of_each_table():
    """One illuminate() over the seven tables, cut into columns, is illuminate() over each table alone."""
    lat, lon = lc.window()
    la, lo = lc.grid_nodes(lat, lon, (5, 1))
    both = lc.grid_model((5, 1))
    for n in (1, 8, 64):
        m = im.illuminate(lc.scene(), lc.dem(), la, lo, lc.sun_table(n).astype(np.float64))
        for key in ("V", "flagged", "cos_pos", "lit", "irr", "mu", "D"):
            assert np.array_equal(both[n][key], m[key]), (n, key)
        assert both[n]["shadow_rays"] == m["shadow_rays"]


def test_the_launch_rule_gives_the_documented_blocks():
    """PW x PH per n_sun as DESIGN.md 4.8 and the launcher's comment state them, a one-row band side by side, and the series'
    block narrowed to the least power of two >= count; COUNTS reaches every width the narrowing can end at."""
    want = {1: (8, 8), 2: (8, 4), 4: (4, 4), 8: (4, 2), 16: (2, 2), 32: (2, 1), 64: (1, 1)}
    for n in lc.N_SUN:
        P = 64 // n
        assert lc.launch(9, 21, n)[:2] == want[n] and want[n][0] * want[n][1] == P
        assert lc.launch(1, 13, n)[:2] == (P, 1)
        assert lc.launch(9, 21, n)[2:] == (-(-21 // want[n][0]), -(-9 // want[n][1]))
        widths = set()
        for count in lc.COUNTS:
            PW, PH, wx, wy = lc.launch(7, count, n, "series")
            assert PW * PH == P and PW & (PW - 1) == 0
            assert PW == P or (PW >= count and PW // 2 < count)          # the least power of two >= count, capped at P
            assert wx == -(-count // PW) and wy == -(-7 // PH)
            widths.add(PW)
        assert widths == {1 << k for k in range(P.bit_length())}, (n, widths)
    # the shapes are ragged against every grid block, and one is wider than two of the widest
    for n in lc.N_SUN:
        PW, PH = want[n]
        for rows, cols in ((9, 21), (13, 7)):
            assert PW == 1 or cols % PW, (n, rows, cols)
            assert PH == 1 or rows % PH, (n, rows, cols)
    assert any(cols > 2 * 8 and rows % 2 for rows, cols in lc.SHAPES)
    # ... and no point count of the series is a multiple of a PH > 1
    assert all(k % ph for k in lc.POINTS for ph in (2, 4, 8, 16, 32, 64))


@pytest.mark.parametrize("n_sun", lc.N_SUN)
def test_the_true_mapping_holds_every_sample_once_and_reports_the_model(n_sun):
    """Every (node, sample) sits in exactly one lane inside the band, every node is stored once, lit is the model's
    V.mean() at every node and shadow_rays its count of cos > 0 -- in every grid and series case, in every band of 1 to 13
    rows at five widths, and in every window of 1 to 70 epochs at 1 to 9 points."""
    for rows in range(1, 14):
        for cols in (1, 7, 13, 19, 21):
            L = lc.lanes(rows, cols, n_sun)
            assert (lc.coverage(L) == 1).all(), (rows, cols)
    for pts in range(1, 10):
        for count in range(1, 71):
            assert (lc.coverage(lc.lanes(pts, count, n_sun, "series")) == 1).all(), (pts, count)
    for name, kind, rows, cols, V, cp, fl in all_cases(n_sun):
        L = lc.lanes(rows, cols, n_sun, kind)
        lit, stores, rays = lc.report(L, V, cp)
        assert (lc.coverage(L) == 1).all() and (stores == 1).all(), name
        assert np.array_equal(lit, V.mean(1)), name
        assert rays == int(cp.sum()), name


def shares(m):
    ok = ~m["flagged"].any(1)
    part = ok & (m["lit"] > 0) & (m["lit"] < 1)
    return ok, part, ok & (m["lit"] == 0), ok & (m["lit"] == 1)


@pytest.mark.parametrize("shape", lc.SHAPES)
def test_the_caps(shape):
    """What keeps the GPU comparison from being vacuous, from the model alone.  Grids of 90 nodes or more: flagged samples
    <= 2 %, unflagged nodes >= 75 %, unflagged nodes with 0 < lit < 1 >= 15 % for n_sun >= 4 and at least one at n_sun = 2,
    dark and lit nodes >= 20 % each at n_sun = 1.  The thin shapes: a dark, a lit and (n_sun >= 4) a partial unflagged node."""
    models = lc.grid_model(shape)
    for n in lc.N_SUN:
        m = models[n]
        ok, part, dark, lit = shares(m)
        print(f"{shape} n_sun {n}: flagged samples {m['flagged'].mean():.2%}, unflagged nodes {ok.mean():.1%}, partial "
              f"{part.mean():.1%}, dark {dark.mean():.1%}, lit {lit.mean():.1%}")
        if shape in lc.THIN:
            assert dark.any() and lit.any(), n
            assert n < 4 or part.any(), n
            continue
        assert shape[0] * shape[1] >= 90
        assert m["flagged"].mean() <= 0.02, n
        assert ok.mean() >= 0.75, n
        if n >= 4:
            assert part.mean() >= 0.15, n
        if n == 2:
            assert part.any()
        if n == 1:
            assert dark.mean() >= 0.2 and lit.mean() >= 0.2


def test_the_series_cross_the_terminator():
    """Every n_sun's series hold dark, lit and (n_sun >= 2) partial unflagged (point, epoch) pairs, and most are unflagged."""
    sm = lc.series_model()
    for n in lc.N_SUN:
        ok = ~sm[n]["flagged"].any(2)
        lit = sm[n]["lit"]
        part = ok & (lit > 0) & (lit < 1)
        print(f"series n_sun {n}: unflagged pairs {ok.mean():.1%}, partial {part.mean():.1%}, dark {(ok & (lit == 0)).mean():.1%}, "
              f"lit {(ok & (lit == 1)).mean():.1%}")
        assert ok.mean() >= 0.75 and (ok & (lit == 0)).mean() >= 0.2 and (ok & (lit == 1)).mean() >= 0.2
        assert n == 1 or part.mean() >= 0.15
    names = [c[0] for c in lc.series_cases()]
    assert len(set(names)) == len(names) == len(lc.N_SUN) * len(lc.COUNTS)
    for n in lc.N_SUN:
        assert {c[2] for c in lc.series_cases() if c[1] == n} == set(lc.POINTS)


def same_map(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("row", "col", "sample", "inside"))


@pytest.mark.parametrize("mutant", lc.MUTANTS)
def test_the_cases_kill_every_mutant_where_it_is_one(mutant):
    """Per n_sun: a pair listed in IDENTITY reports the true mapping's lit, stores and shadow_rays in every case (and has its
    lane map, the reduction defects aside); at every other n_sun some case has an unflagged node whose lit differs -- for
    edge_lanes_not_zeroed, which lit cannot see, a case whose shadow_rays differs while lit and the stores stay."""
    for n in lc.N_SUN:
        kills, ray_kills, differs = [], [], False
        for name, kind, rows, cols, V, cp, fl in all_cases(n):
            true = lc.lanes(rows, cols, n, kind)
            L = lc.lanes(rows, cols, n, kind, mutant)
            differs |= not same_map(true, L)
            want, _, rays = lc.report(true, V, cp)
            got, stores, rays_m = lc.report(L, V, cp)
            ok = ~fl.any(1)
            bad = ok & ~(got == want)                                   # NaN (never stored) differs too
            if bad.any():
                kills.append((name, int(bad.sum())))
            if rays_m != rays:
                ray_kills.append((name, rays_m - rays))
            if (mutant, n) in IDENTITY or mutant in COUNTER_ONLY:
                assert np.array_equal(got, want) and (stores == 1).all(), (n, name)
        if (mutant, n) in IDENTITY:
            assert not differs and not kills and not ray_kills, (n, kills, ray_kills)
            print(f"{mutant}, n_sun {n}: the true mapping")
        elif mutant in COUNTER_ONLY:
            assert ray_kills, f"{mutant} survives every case at n_sun {n}"
            print(f"{mutant}, n_sun {n}: lit unchanged; shadow_rays differs in {len(ray_kills)} case(s), first {ray_kills[0]}")
        else:
            assert kills, f"{mutant} survives every case at n_sun {n}"
            print(f"{mutant}, n_sun {n}: killed by {len(kills)} case(s), first {kills[0]}")


def test_every_mutant_is_named_once():
    assert len(set(lc.MUTANTS)) == len(lc.MUTANTS) == 7
    assert {m for m, _ in IDENTITY} <= set(lc.MUTANTS) and set(COUNTER_ONLY) <= set(lc.MUTANTS)
