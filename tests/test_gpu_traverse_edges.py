"""The traverse stage's edge rules and tile hand-offs on the MI355X, on the built cases of
tests/traverse_edge_cases.py at tile edges 8, 16 and 32: pair lattices (some 500 two-node islands per call: the timed edge rule
across 64-epoch words, at the table's end, with ticks on both sides of 2^32 and without a table near 2^62; the cost rule at the
grade limit, at the penalty bounds and where the float64 sum rounds), diagonal corridors that pass from tile to tile through
corners only, and windows with tiles one node wide or high.  Every field is bit-equal to the model's, for both relax kernels.
tests/test_traverse_edges_host.py shows from the model alone what each case exercises."""
import numpy as np
import pytest

import timed_traverse_model as ttm
import traverse_edge_cases as ec
import traverse_model as tm
from moonrtx_amd.renderer import DeviceBuffer
from test_gpu_timed_traverse import assert_field_equal as assert_arrival_equal, gpu_field as gpu_arrival
from test_gpu_traverse import assert_field_equal as assert_cost_equal, ctx, gpu_field as gpu_cost
from test_traverse_edges_host import TABLES, check_corridor, lattice

pytestmark = pytest.mark.gpu

NEVER = np.uint64(ttm.NEVER)
TILES = ("8", "16", "32")
_WANT = {}


def want(key, make):
    """The model's field of a case, computed once and shared by the tile sizes."""
    if key not in _WANT:
        _WANT[key] = make()
    return _WANT[key]


def timed_model(lat, start=None, avail="own"):
    return ttm.field(lat.dem, lat.t, lat.src, lat.start if start is None else start, lat.P, lat.avail if avail == "own" else avail,
                     lat.tpc, lat.tpe)


def check_pair_codes(lat, got):
    """Every reached v has the code of its pair's direction, every u is a source, every walled node is unreachable."""
    A, pred = got
    s = lat.sites
    reached = A[s["vi"], s["vj"]] != NEVER
    assert np.array_equal(pred[s["vi"], s["vj"]][reached], s["k"][reached]) and (pred[s["vi"], s["vj"]][~reached] == 255).all()
    assert (pred[s["ui"], s["uj"]] == 8).all() and (pred[lat.walled()] == 255).all()


@pytest.mark.parametrize("ts", TILES)
@pytest.mark.parametrize("name", list(TABLES))
def test_pair_lattice_arrivals_match_the_model(native_lib, monkeypatch, name, ts):
    lat = lattice(name)
    model = want(("timed", name), lambda: timed_model(lat))
    assert 0.5 < (model[0][lat.sites["vi"], lat.sites["vj"]] != NEVER).mean() < 0.95          # reached and NEVER both occur
    words = ec.packed(lat.avail, seed=5)                    # random garbage past the table's last epoch
    monkeypatch.setenv("MOONRT_TRAVERSE_TILE", ts)
    rt = ctx(lat.dem)
    got = gpu_arrival(rt, lat.t, lat.src, lat.start, lat.P, words, lat.n_epochs, lat.tpe, lat.tpc)
    dev = None
    if name == "n321":
        buf = DeviceBuffer(words.nbytes)
        buf.upload(words)
        dev = gpu_arrival(rt, lat.t, lat.src, lat.start, lat.P, None, lat.n_epochs, lat.tpe, lat.tpc, dev_avail=buf.ptr)
        buf.free()
    rt.close()
    assert_arrival_equal(got, model, f"{name}, tile {ts}")
    check_pair_codes(lat, got)
    if dev is not None:
        assert_arrival_equal(dev, model, f"{name}, tile {ts}: device table")


@pytest.mark.parametrize("ts", TILES)
def test_pair_lattice_ticks_beyond_32_bits_match_the_model(native_lib, monkeypatch, ts):
    """ticks_per_epoch = 2^31 - 1: ticks on both sides of 2^32, durations up to 2^31; and no table with starts just below 2^62."""
    big = want("big-lattice", ec.big_tick_lattice)
    model = want("big", lambda: timed_model(big))
    lat = lattice("n320")
    rng = np.random.default_rng(62)
    back = rng.integers(0, 1 << 31, lat.n).astype(np.uint64)
    back[::4] = 0                                           # every fourth start is 2^62 - 1, the last one accepted
    late = np.uint64(1 << 62) - np.uint64(1) - back
    assert late.max() == (1 << 62) - 1 and late.min() >= (1 << 62) - (1 << 31)
    model_late = want("late", lambda: timed_model(lat, late, None))
    assert (model_late[0][lat.sites["vi"], lat.sites["vj"]][::4] >= np.uint64(1 << 62)).all()     # arrivals past 2^62
    assert (model_late[0][lat.sites["vi"], lat.sites["vj"]] != NEVER).all()
    monkeypatch.setenv("MOONRT_TRAVERSE_TILE", ts)
    rt = ctx(big.dem)
    got = gpu_arrival(rt, big.t, big.src, big.start, big.P, ec.packed(big.avail, seed=8), big.n_epochs, big.tpe, big.tpc)
    got_late = gpu_arrival(rt, lat.t, lat.src, late, lat.P, None, 0, lat.tpe, lat.tpc)
    rt.close()
    assert_arrival_equal(got, model, f"big ticks, tile {ts}")
    check_pair_codes(big, got)
    assert_arrival_equal(got_late, model_late, f"no table, starts near 2^62, tile {ts}")
    check_pair_codes(lat, got_late)


@pytest.mark.parametrize("ts", TILES)
def test_pair_lattice_costs_match_the_model(native_lib, monkeypatch, ts):
    """Penalties at 1e-3, at 1e6 and mixed with start costs 0 and 2^52; the grade limit met exactly and missed by one float32."""
    cases = {"penalties": want("cost-lattice", ec.cost_lattice)}
    for kind in ec.GRADE_KINDS:
        cases[f"grade-{kind}"] = want(("grade", kind), lambda: ec.grade_lattice(kind))
        cases[f"grade-{kind}-tight"] = want(("grade", kind, "tight"), lambda: ec.grade_lattice(kind, tight=True))
    monkeypatch.setenv("MOONRT_TRAVERSE_TILE", ts)
    rt = ctx(cases["penalties"].dem)
    for name, lat in cases.items():
        model = want(("cost", name), lambda: tm.field(lat.dem, lat.t, lat.src, lat.start, lat.P))
        rt.upload_dem(lat.dem)
        got = gpu_cost(rt, lat.t, lat.src, lat.start, lat.P)
        assert_cost_equal(got, model, f"{name}, tile {ts}")
        s = lat.sites
        reached = np.isfinite(got[0][s["vi"], s["vj"]])
        assert np.array_equal(got[1][s["vi"], s["vj"]][reached], s["k"][reached]) and (got[1][lat.walled()] == 255).all()
        if name.startswith("grade"):
            exact = np.array([v in ("climb", "descend") for v in lat.variant])
            assert exact.sum() >= 4 and (reached[exact] == (not name.endswith("tight"))).all(), name
    rt.close()


@pytest.mark.parametrize("ts", TILES)
def test_corridors_pass_through_tile_corners(native_lib, monkeypatch, ts):
    """Diagonal corridors one node wide: every hand-off from tile to tile is through a corner (the diagonal tile flags, the
    3 x 3 seeding for a source on a tile's last node, the wrapped tile column at +-180), on both fields."""
    c = ec.CORRIDOR_TIMED
    monkeypatch.setenv("MOONRT_TRAVERSE_TILE", ts)
    rt = None
    for name in ec.CORRIDORS:
        dem, t, src, P, on = ec.corridor(name)
        av = ec.corridor_mask(name)
        w_cost = want(("corridor", name, "cost"), lambda: tm.field(dem, t, src, None, P))
        w_mask = want(("corridor", name, "mask"), lambda: ttm.field(dem, t, src, c["ticks"], P, av, c["tpc"], c["tpe"]))
        w_none = want(("corridor", name, "none"), lambda: ttm.field(dem, t, src, c["ticks"], P, None, c["tpc"], c["tpe"]))
        for w in (w_cost, w_mask, w_none):
            check_corridor(name, w, src, on)
        assert not np.array_equal(w_mask[0], w_none[0])         # the table makes the route wait
        if rt is None:
            rt = ctx(dem)
        else:
            rt.upload_dem(dem)
        st, st_t = {}, {}
        assert_cost_equal(gpu_cost(rt, t, src, None, P, st), w_cost, f"{name}, tile {ts}: costs")
        assert_arrival_equal(gpu_arrival(rt, t, src, c["ticks"], P, ec.packed(av), c["n_epochs"], c["tpe"], c["tpc"], st_t), w_mask,
                             f"{name}, tile {ts}: random table")
        assert_arrival_equal(gpu_arrival(rt, t, src, c["ticks"], P, None, 0, c["tpe"], c["tpc"]), w_none, f"{name}, tile {ts}: no table")
        print(f"{name}, tile {ts}: costs {st['launches']} launches, {st['tile_visits']} tile visits; arrivals {st_t['launches']} "
              f"launches, {st_t['tile_visits']} tile visits")
        # the corridor crosses every tile of its diagonal, and a tile's value reaches the next one a launch later at the earliest
        for s in (st, st_t):
            assert s["tile_visits"] >= 64 // int(ts) and s["launches"] >= 32 // int(ts)
    rt.close()


@pytest.mark.parametrize("ts", TILES)
def test_thin_windows_match_the_model(native_lib, monkeypatch, ts):
    """33 x 65 (the last tile one node high and one node wide at every tile edge), the same wrapped, 1 x 40, 40 x 1, 1 x 1."""
    c = ec.THIN_TIMED
    monkeypatch.setenv("MOONRT_TRAVERSE_TILE", ts)
    rt = None
    for name in ec.THIN:
        dem, t, src, c0, ticks, av = ec.thin(name)
        assert name == "1x1" or t.rows % int(ts) == 1 or t.cols % int(ts) == 1
        w_cost = want(("thin", name, "cost"), lambda: tm.field(dem, t, src, c0))
        w_mask = want(("thin", name, "mask"), lambda: ttm.field(dem, t, src, ticks, None, av, c["tpc"], c["tpe"]))
        w_none = want(("thin", name, "none"), lambda: ttm.field(dem, t, src, ticks, None, None, c["tpc"], c["tpe"]))
        if name != "1x1":
            assert np.isfinite(w_cost[0]).mean() > 0.5 and (w_mask[0] != NEVER).mean() > 0.5 and not np.array_equal(w_mask[0], w_none[0])
        if rt is None:
            rt = ctx(dem)
        else:
            rt.upload_dem(dem)
        assert_cost_equal(gpu_cost(rt, t, src, c0), w_cost, f"{name}, tile {ts}: costs")
        assert_arrival_equal(gpu_arrival(rt, t, src, ticks, None, ec.packed(av, seed=3), c["n_epochs"], c["tpe"], c["tpc"]), w_mask,
                             f"{name}, tile {ts}: random table")
        assert_arrival_equal(gpu_arrival(rt, t, src, ticks, None, None, 0, c["tpe"], c["tpc"]), w_none, f"{name}, tile {ts}: no table")
    rt.close()
