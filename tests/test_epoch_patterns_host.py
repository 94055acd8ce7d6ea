"""The designed epoch patterns without a GPU (tests/epoch_patterns.py; DESIGN.md sections 3.9, 3.15 and 4.16): the float64
model returns exactly the designed bits with the horizon far from the disc; the plain-loop expectations equal the numpy
reductions of the models; the Python restatement of the kernel's chunk-and-carry walk equals the truth at every epoch count
of the chunk-edge set; and the pattern set tells every named defect of that walk that can show in an output from a correct
walk."""
import numpy as np
import pytest

import epoch_patterns as ep
import horizon_model as hm
import mast_model as mm
import model_cases as mc
from moonrtx_amd.scene import named_scene

LAT, LON, N_AZ, SEED = 23.0, -57.0, 1024, 0


def scene():
    return named_scene("S1", 16, 16)


@pytest.mark.parametrize("m", ep.M)
def test_the_model_returns_the_designed_bits(m):
    """horizon_model.sun_fraction on lights() and horizon_rows() is exactly 0.0 or 1.0 and equals the designed bit in every
    entry of both tables; every light sits on a sample centre; the horizon stays more than 30 deg from the disc's edge."""
    s, dem = scene(), mc.crater_dem()
    _, a, b = ep.stack(ep.patterns(m, SEED))
    P = a.shape[0]
    hz = ep.horizon_rows(a, b, N_AZ)
    lat, lon = np.full(P, LAT), np.full(P, LON)
    sa, sb = ep.sectors_of(m, N_AZ)
    worst = np.inf
    for sectors, bits, radius in ((sa, a, 0.27), (sb, b, 0.27), (sb, b, 0.0)):
        f, info = hm.sun_fraction(s, dem, lat, lon, hz, ep.lights(s, dem, LAT, LON, sectors, N_AZ, radius_deg=radius))
        assert f.shape == (P, m)
        assert np.array_equal(f, bits.astype(np.float64))       # every entry: nothing is left out
        off = np.abs(info["phi"] / 360.0 * N_AZ - sectors[None, :])
        off = np.minimum(off, N_AZ - off)
        assert off.max() < 1e-9, off.max()
        assert np.allclose(info["alpha"], radius, rtol=0, atol=1e-9) and np.allclose(info["e_s"], 10.0, rtol=0, atol=1e-9)
        margin = float((np.abs(info["h"] - info["e_s"]) - info["alpha"]).min())
        worst = min(worst, margin)
    print(f"m = {m}: {P} patterns; smallest |h - e_s| - alpha = {worst:.2f} deg; excluded share 0")
    assert worst > 30.0


def test_fractional_sectors_lie_between_the_samples():
    """The seam case's light: azimuth sample n_az - 1/2 interpolates the last and the first sample of the row."""
    s, dem = scene(), mc.crater_dem()
    for n_az in (4, 64):
        hz = np.full((1, n_az), 80.0, np.float32)
        hz[:, n_az - 1], hz[:, 0] = 40.0, -40.0
        lights = ep.lights(s, dem, LAT, LON, [n_az - 0.5, n_az - 0.5], n_az, elev_deg=[10.0, -10.0])
        f, info = hm.sun_fraction(s, dem, [LAT], [LON], hz, lights)
        assert np.array_equal(f, [[1.0, 0.0]]) and np.abs(info["h"]).max() < 1e-9
        assert np.array_equal(info["h0"], [[40.0, 40.0]]) and np.array_equal(info["h1"], [[-40.0, -40.0]])


@pytest.mark.parametrize("m", ep.M)
def test_expectations_equal_the_models_reductions(m):
    """expect_windows == mast_model.windows and expect_summary == horizon_model.summarize on the bits taken as float32
    fractions, at both threshold pairs the GPU tests use."""
    _, a, b = ep.stack(ep.patterns(m, SEED))
    fa, fb = a.astype(np.float32), b.astype(np.float32)
    want = ep.expect_windows(a, b)
    for mins in ((1.0, 1.0), (0.5, 0.5)):
        model, cnt = mm.windows(fa, fb, *mins)
        assert np.array_equal(want, model.astype(np.float32))
        assert np.array_equal(cnt, np.stack([a.sum(1), b.sum(1), (a & b).sum(1)], -1))
    for bits, f in ((a, fa), (b, fb)):
        assert np.array_equal(ep.expect_summary(bits), hm.summarize(f).astype(np.float32))
    # SUMMARY forms its shares as count * (1 / m) in float64, the windows as count / m: the same float32 at these m
    c = np.arange(m + 1, dtype=np.float64)
    assert np.array_equal((c * (1.0 / m)).astype(np.float32), (c / m).astype(np.float32))


@pytest.mark.parametrize("m", ep.M)
def test_the_chunked_walk_equals_the_truth(m):
    _, a, b = ep.stack(ep.patterns(m, SEED))
    assert np.array_equal(ep.chunked_windows(a, b), ep.expect_windows(a, b))


def test_pattern_names_are_unique_and_cover_the_edges():
    for m in ep.M:
        names, a, b = ep.stack(ep.patterns(m, SEED))
        assert len(set(names)) == len(names) and a.shape == b.shape == (len(names), m)
    names = set(ep.stack(ep.patterns(512, SEED))[0])
    for want in ("one1@63", "one0@64", "run[64,128)", "run[60,130)", "tie:straddle-then-later", "tie:chunk0-then-straddle",
                 "lane63", "lane0", "1010", "random0.5"):
        assert f"A={want},B=all1" in names and f"A=all1,B={want}" in names, want


# carry_from_lane_63 cannot show in an output.  The carries are read from `last` = min(64, m - k0) - 1, which differs from 63
# only in a chunk that is not full, and only the final chunk can be that: its carries are never read.  The defect is real --
# the carries it leaves after the final chunk differ, shown below -- but no (m, pattern) can tell it from a correct walk, so
# it is asserted EQUAL on every pattern instead of killed.  (Reading lane 63 would start to matter the day a walk continues
# after a partial chunk, e.g. a call resumed from saved carries; nothing does that today.)
UNOBSERVABLE = ("carry_from_lane_63",)


def test_the_patterns_kill_every_observable_mutant():
    """Adequacy: for every named defect of the walk that can change an output there is an (m, pattern) whose eight columns
    differ from the truth -- the first one found is printed with the columns that differ -- so a kernel with that defect
    fails tests/test_gpu_epoch_walks.py."""
    killed = {}
    cases = {m: ep.stack(ep.patterns(m, SEED)) for m in ep.M}
    truth = {m: ep.expect_windows(a, b) for m, (_, a, b) in cases.items()}
    for mutant in ep.MUTANTS:
        kills = []
        for m, (names, a, b) in cases.items():
            got = ep.chunked_windows(a, b, mutant=mutant)
            for p in np.flatnonzero((got != truth[m]).any(1)):
                kills.append((m, names[p], np.flatnonzero(got[p] != truth[m][p]).tolist()))
        killed[mutant] = kills
        if kills:
            m, name, cols = kills[0]
            print(f"{mutant}: killed by {len(kills)} (m, pattern)s at {len({k[0] for k in kills})} epoch counts, first "
                  f"m = {m}, {name}, columns {cols}")
        else:
            print(f"{mutant}: equal to the truth on every (m, pattern)")
    for mutant in ep.MUTANTS:
        if mutant in UNOBSERVABLE:
            assert not killed[mutant], (mutant, killed[mutant][:3])
        else:
            assert killed[mutant], f"{mutant} survives every pattern"
    # the tie rule is caught by the designed ties themselves, in the start index alone, not only by the -1 of "no window"
    ties = {k[1]: k[2] for k in killed["tie_takes_later"] if k[0] == 512}
    for name in ("A=tie:straddle-then-later,B=all1", "A=all1,B=tie:chunk0-then-straddle"):
        assert ties.get(name) == [6], (name, ties.get(name))
    # every epoch count but the trivial ones tells at least one defect apart, and the edges m = 64 k + 1 catch the inactive lanes
    assert {k[0] for k in killed["inactive_lanes_unset"]} >= {1, 2, 63, 65, 127, 129, 191, 193}
    assert {k[0] for k in killed["no_carry"]} >= {65, 127, 128, 129, 191, 192, 193, 512}


def test_the_unobservable_mutant_is_a_real_defect():
    """carry_from_lane_63 leaves other carries after a final partial chunk whose run reaches the last epoch, and the same
    outputs."""
    a = np.ones((1, 65), bool)
    good, left = ep.chunked_windows(a, a, carries=True)
    bad, left_bad = ep.chunked_windows(a, a, mutant="carry_from_lane_63", carries=True)
    assert np.array_equal(good, bad) and left[0, 2] == 65 and left_bad[0, 2] == 0
