"""The pass kernels' wave reductions on the MI355X at every 64-epoch chunk edge (DESIGN.md sections 3.27 and 4.33): designed
in-view sequences (tests/epoch_patterns.py) driven through SUMMARY and LIST.  The horizon rows are constant at -45 deg and epoch
k of a satellite is placed from the point's own frame: at an elevation of 10 deg or more where the bit is set, at -60 deg where
it is clear, three radii away either way (2.19 radii from the centre at -60 deg: outside the bounding sphere).  float32 cannot
flip such a bit, so the expected outputs are plain loops over the bits with no tolerance.  Both addressing builds run every case;
no march runs."""
import numpy as np
import pytest

import epoch_patterns as ep
import horizon_model as hm
import model_cases as mc
import passes_model as pm
from moonrtx_amd import _lib
from test_gpu_illumination import make

pytestmark = pytest.mark.gpu

LAT, LON, N_AZ, SEED = 23.0, -57.0, 16, 0


@pytest.fixture(scope="module", params=[0, _lib.F_FORCE_WIDE], ids=["narrow", "wide"])
def rt(request, native_lib):
    ctx = make(pm.scene(), mc.crater_dem(), request.param)
    yield ctx
    ctx.close()


def place(bits, elev_deg=30.0):
    """(m, 3) Moon-fixed metres: epoch k stands at elevation elev_deg[k] where bits[k] is set and at -60 deg where it is not,
    on an azimuth that turns with k, 3 R from the lifted origin of (LAT, LON)."""
    s = pm.scene()
    o, _, U, N, E = hm.frame(s, mc.crater_dem(), [LAT], [LON])
    o, U, N, E = o[0], U[0], N[0], E[0]
    bits = np.asarray(bits, bool)
    e = np.radians(np.where(bits, np.broadcast_to(np.asarray(elev_deg, np.float64), bits.shape), -60.0))
    phi = 2.0 * np.pi * (np.arange(bits.size) % 37) / 37.0
    d = np.cos(e)[:, None] * (np.cos(phi)[:, None] * N + np.sin(phi)[:, None] * E) + np.sin(e)[:, None] * U
    R = float(s.radius)
    return (o + 3.0 * R * d) / R * pm.RADIUS_M


def runs_of(bits):
    """[(first, count)] of the maximal runs of set bits, by a plain loop."""
    out, start = [], None
    for k, v in enumerate(list(bits) + [False]):
        if v and start is None:
            start = k
        if not v and start is not None:
            out.append((start, k - start))
            start = None
    return out


def expect_summary(a, b):
    """Columns 0-4, 6 and 7 for two sequences, by plain loops."""
    m = len(a)
    c = [int(x) + int(y) for x, y in zip(a, b)]
    any_ = [v >= 1 for v in c]
    runs = runs_of(any_)
    gaps = runs_of([not v for v in any_])
    best = max(runs, key=lambda r: (r[1], -r[0]), default=(-1, 0))
    return {0: np.float32(sum(any_) / float(m)), 1: np.float32(max((g[1] for g in gaps), default=0)), 2: np.float32(best[1]),
            3: np.float32(best[0]), 4: np.float32(len(runs)), 6: np.float32(sum(c) / float(m)),
            7: np.float32(sum(1 for v in c if v >= 2) / float(m))}


@pytest.mark.parametrize("m", ep.M)
def test_designed_sequences(rt, m):
    seqs = ep.structured(m, SEED)
    lat, lon = np.array([LAT]), np.array([LON])
    hz = np.full((1, N_AZ), -45.0, np.float32)
    for i, (name, a) in enumerate(seqs):
        other_name, b = seqs[(i + 5) % len(seqs)]
        pos = np.stack([place(a), place(b)])
        what = f"m = {m}: {name} and {other_name}"
        summ = rt.horizon_passes(lat, lon, hz, pos, mode="summary")[0]
        for j, v in expect_summary(a, b).items():
            assert summ[j] == v, f"{what}: column {j} is {summ[j]!r}, not {v!r}"
        assert summ[5] >= 29.9 if (a.any() or b.any()) else summ[5] == -90.0, what
        recs = rt.horizon_passes(lat, lon, hz, pos, mode="list")
        want = [(0, s, f, n) for s, bits in enumerate((a, b)) for f, n in runs_of(bits)]
        got = [tuple(int(r[k]) for k in ("point", "sat", "first", "count")) for r in recs]
        assert got == want, f"{what}: passes {got[:6]} ..., not {want[:6]} ..."
        flags = [(1 if f == 0 else 0) | (2 if f + n == m else 0) for _, _, f, n in want]
        assert [int(r["flags"]) for r in recs] == flags, what
        for r in recs:
            assert (r["rise_frac"] == 0) == (r["first"] == 0) and (r["set_frac"] == 0) == (r["first"] + r["count"] == m), what
            assert 0 <= r["rise_frac"] <= 1 and 0 <= r["set_frac"] <= 1
            assert r["first"] <= r["max_at"] < r["first"] + r["count"] and 29.9 < r["max_elev_deg"] < 30.1
            assert abs(r["min_range_m"] - 3.0 * pm.RADIUS_M) < 10.0


PEAKS = {"lane 0": (130, [(0, 130)], [0]), "lane 63": (130, [(0, 130)], [63]), "lane 64": (130, [(0, 130)], [64]),
         "the last epoch": (130, [(0, 130)], [129]), "a tie in one chunk": (130, [(0, 130)], [5, 20]),
         "a tie across 63 | 64": (130, [(0, 130)], [63, 64]), "a tie across three chunks": (130, [(0, 130)], [10, 70, 128]),
         "two passes, a tie in each": (192, [(3, 67), (72, 120)], [8, 69, 100, 127, 128, 191]),
         "a pass that starts at lane 63": (192, [(63, 70)], [64, 128, 132])}


@pytest.mark.parametrize("name", sorted(PEAKS))
def test_max_at_takes_the_earliest_of_equal_maxima(rt, name):
    """Every epoch in view stands at 10 deg + its index / 100, except the listed peaks, which all stand at one and the same
    position at 50 deg: the same bits, an exact tie.  The earliest peak inside each pass is its max_at."""
    m, spans, peaks = PEAKS[name]
    bits = np.zeros(m, bool)
    for f, n in spans:
        bits[f:f + n] = True
    elev = 10.0 + np.arange(m) / 100.0
    pos = place(bits, elev)
    peak = place(np.ones(1, bool), 50.0)[0]
    pos[peaks] = peak
    lat, lon = np.array([LAT]), np.array([LON])
    hz = np.full((1, N_AZ), -45.0, np.float32)
    recs = rt.horizon_passes(lat, lon, hz, pos, mode="list")
    full = rt.horizon_passes(lat, lon, hz, pos, mode="full")[0, 0]
    assert [(int(r["first"]), int(r["count"])) for r in recs] == spans
    for r, (f, n) in zip(recs, spans):
        inside = [k for k in peaks if f <= k < f + n]
        assert int(r["max_at"]) == min(inside), (name, int(r["max_at"]), inside)
        assert r["max_elev_deg"] == full[min(inside), 0] and all(full[k, 0] == full[inside[0], 0] for k in inside)
        assert r["min_range_m"] == full[f:f + n, 2].min()
    summ = rt.horizon_passes(lat, lon, hz, pos, mode="summary")[0]
    assert summ[5] == full[peaks[0], 0] and summ[4] == len(spans)
