"""The depression hierarchy on the GPU: mrtx_bowls / MoonRT.bowls / MoonRT.peaks against the sweep of
tests/bowls_model.py.  Every field of every record and every label is compared with ==, from host and from device tables, with
and without row weights, with and without invert.  Lattices are at most 128 x 128 so that the model runs in well under a second;
the one larger window is compared device against device (identity 1, against mrtx_fill)."""
import ctypes as C
import os

import numpy as np
import pytest

import bowls_cases as bc
import bowls_model as bm
import model_cases as mc
from common import assert_bit_equal
from moonrtx_amd import _lib
from moonrtx_amd import basins as bs
from moonrtx_amd.renderer import DeviceBuffer, MoonRT, MoonRTError
from moonrtx_amd.scene import named_scene
from test_gpu_illumination import make

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt(native_lib):
    """One context for the module, without a DEM, a light or a Moon frame: the stage needs none of them."""
    r = MoonRT(16, 16)
    yield r
    r.close()


def weights_for(rows):
    """distinct per row and near 2^32, so that weight and volume need 64 bits"""
    return (2 ** 32 - 1 - 3 * np.arange(rows)).astype(np.uint32)


def on_device(a):
    buf = DeviceBuffer(max(a.nbytes, 4))
    buf.upload(np.ascontiguousarray(a))
    return buf


def run(rt, case, invert, weights, device, stats=None, labels=True):
    z, conn, wrap, edge, table = case
    kw = dict(edge_outlets=edge, connectivity=conn, wrap=wrap, invert=invert, row_weights=weights, labels=labels, stats=stats)
    if not device:
        return rt.bowls(z, table, **kw)
    zb, tb = on_device(z), on_device(table) if table is not None else None
    try:
        return rt.bowls(zb, tb, shape=z.shape, **kw)
    finally:
        zb.free()
        if tb is not None:
            tb.free()


def assert_tree_equal(got, want, want_labels, what):
    assert got.records.dtype == bs.BOWL_DTYPE and got.records.shape == want.shape, (what, got.records.shape, want.shape)
    for name in bs.BOWL_DTYPE.names:
        bad = np.flatnonzero(got.records[name] != want[name])
        assert bad.size == 0, (what, name, int(bad[0]), got.records[bad[0]], want[bad[0]])
    assert got.labels.dtype == np.int32 and got.labels.shape == want_labels.shape, what
    bad = np.argwhere(got.labels != want_labels)
    assert bad.size == 0, (what, len(bad), bad[0].tolist(), int(got.labels[tuple(bad[0])]), int(want_labels[tuple(bad[0])]))


def check(rt, case, what, inverts=(False, True)):
    """From host tables with row weights and from device tables without, both directions, against the model; returns the
    model's tree of the last direction."""
    z, conn, wrap, edge, table = case
    for invert in inverts:
        for device, weights in ((False, weights_for(z.shape[0])), (True, None)):
            want, want_labels = bm.bowls(z, conn, wrap, edge, table, invert, weights)
            st = {}
            got = run(rt, case, invert, weights, device, st)
            assert_tree_equal(got, want, want_labels, (what, invert, device))
            assert (got.z == z).all() and got.connectivity == conn and got.wrap == bool(wrap) and got.invert == invert
            assert st["launches"] > 0 and st["kernel_ms"] > 0.0 and st["bowls"] == len(want)
            if len(want):
                assert (want["parent"][want["parent"] >= 0] > np.flatnonzero(want["parent"] >= 0)).all()
    return got


# ---- thin and ragged lattices
THIN = {
    "1x1": (1, 1, False), "1x40": (1, 40, False), "40x1": (40, 1, False), "33x65": (33, 65, False), "31x97": (31, 97, False),
    "64x64": (64, 64, False), "65x129": (65, 129, False), "5x3_wrapped": (5, 3, True), "40x64_wrapped": (40, 64, True),
    "37x65_wrapped": (37, 65, True),
}


@pytest.mark.parametrize("name", sorted(THIN))
def test_thin_and_ragged_lattices(rt, name):
    rows, cols, wrap = THIN[name]
    for conn in (4, 8):
        if min(rows, cols) > 1:
            check(rt, bc.random_case(11, rows, cols, conn, wrap, -6, 6), (name, conn, "edges"))
        check(rt, bc.random_case(12, rows, cols, conn, wrap, -6, 6, table_share=0.05, edge=False), (name, conn, "table only"))
        check(rt, bc.random_case(13, rows, cols, conn, wrap, -6, 6, table_share=0.02), (name, conn, "edges and table"))


# ---- long descent paths, long parent chains, many minima
@pytest.mark.parametrize("wrap", (False, True))
def test_a_serpentine_channel_is_one_long_descent_path(rt, wrap):
    for conn in (4, 8):
        got = check(rt, bc.serpentine(96, conn, wrap), ("serpentine", conn, wrap), inverts=(False,))
        assert got.n > 100


def test_a_staircase_of_seventy_pits(rt):
    for conn in (4, 8):
        got = check(rt, bc.staircase(70, conn), ("staircase", conn), inverts=(False,))
        r = got.records
        # seventy pits, their sixty-nine metas, and last the zero-depth leaf of the flat of walls
        assert got.n == 140 and (r["n_children"][70:139] == 2).all() and r["n_leaves"][138] == 70 and r["parent"][138] == -1
        chain, b = 0, 69                                                # the first pit is the shallowest, so the last leaf born
        while r["parent"][b] >= 0:
            b, chain = r["parent"][b], chain + 1
        assert chain == 69 and int(got.level().max()) == 69


def test_a_grid_of_a_thousand_pits_takes_several_rounds(rt):
    case = bc.pit_grid(64, 5)
    st = {}
    got = check(rt, case, "pit grid", inverts=(False,))
    run(rt, case, False, None, True, st)
    assert (got.records["n_children"] == 0).sum() >= 31 * 31             # the pits off the lattice's edge
    assert st["rounds"] >= 3, st                                        # the merge rounds of the sized call


# ---- random heights
@pytest.mark.parametrize("conn,wrap", ((8, False), (4, True)))
@pytest.mark.parametrize("span", ("ties", "some", "full"))
def test_random_heights(rt, span, conn, wrap):
    lo, hi = {"ties": (0, 2), "some": (0, 50), "full": (-2 ** 30, 2 ** 30)}[span]
    case = bc.random_case(21, 96, 128, conn, wrap, lo, hi)
    z = case[0]
    if span == "full":
        z[50, 50], z[90, 17] = 2 ** 30, -2 ** 30                       # the bound itself is accepted
    got = check(rt, case, ("random", span, conn, wrap))
    assert got.n > 100


def test_a_height_beyond_the_bound(rt):
    z, conn, wrap, edge, table = bc.random_case(22, 40, 50, 8, False, -9, 9)
    rec, lab = np.zeros(2000, bs.BOWL_DTYPE), np.zeros((40, 50), np.int32)
    for at, bad in (((0, 0), 2 ** 30 + 1), ((39, 49), -2 ** 30 - 1), ((20, 20), 2 ** 31 - 1), ((7, 3), -2 ** 31)):
        mine = z.copy()
        mine[at] = bad
        st = _lib.MrtxStats()
        st.launches = 0xABCD
        n = C.c_uint64(9)
        assert bc.bowls_call(rt._lib, rt._ctx, bc.block(40, 50), z=mine, bowls=rec, cap=2000, label=lab, n=n, st=st) == -1
        msg = rt._lib.mrtx_last_error(rt._ctx).decode()
        assert f"height {at[0] * 50 + at[1]} must lie in -2^30 .. 2^30 (got {bad})" in msg, msg
        assert st.launches == 0xABCD and n.value == 9 and (lab == 0).all() and (rec.view(np.uint8) == 0).all()
        with pytest.raises(MoonRTError, match="1 heights of the device table lie outside"):
            run(rt, (mine, conn, wrap, edge, table), False, None, True)
    check(rt, (z, conn, wrap, edge, table), "afterwards")


# ---- outlets
def test_outlet_sources(rt):
    rng = np.random.default_rng(31)
    z = rng.integers(-8, 9, (70, 75)).astype(np.int32)
    table = (rng.random(z.shape) < 0.01).astype(np.uint8) * 7          # any nonzero byte is an outlet
    for conn, wrap in ((4, False), (8, True)):
        check(rt, (z, conn, wrap, False, table), ("table only", conn, wrap))
        check(rt, (z, conn, wrap, True, table), ("table and edges", conn, wrap))
        check(rt, (z, conn, wrap, True, None), ("edges", conn, wrap))
        none = check(rt, (z, conn, wrap, False, np.zeros_like(table)), ("no outlet", conn, wrap), inverts=(False,))
        r = none.records
        roots = none.roots()
        assert len(roots) == 1 and r["spill_at"][roots[0]] == -1 and r["spill_level"][roots[0]] == _lib.FILL_NONE
        assert r["volume"][roots[0]] == 0 and r["count"][roots[0]] == z.size and (none.labels >= 0).all()
    # a lattice of outlets only has no bowl
    z = rng.integers(-8, 9, (20, 33)).astype(np.int32)
    got = check(rt, (z, 8, False, True, np.ones(z.shape, np.uint8)), "outlets only")
    assert got.n == 0 and (got.labels == -1).all()


def test_weights_that_wrap_the_volume(rt):
    z = np.full((40, 40), 2 ** 30, np.int32)
    z[1:-1, 1:-1] = -2 ** 30 + 1
    z[20, 20] = -2 ** 30
    w = weights_for(40)
    want, _ = bm.bowls(z, 8, False, True, None, False, w)
    exact = sum(int(w[i]) * 38 * (2 ** 31 - 1) for i in range(1, 39)) + int(w[20])
    assert exact >= 2 ** 64 and int(want[-1]["volume"]) == exact % 2 ** 64
    check(rt, (z, 8, False, True, None), "deep")


# ---- capacity
def test_counting_and_capacity(rt):
    case = bc.random_case(41, 50, 60, 8, False, 0, 9)
    z = case[0]
    want, want_labels = bm.bowls(z, 8)
    total = len(want)
    assert total > 20
    n, rounds, st = C.c_uint64(0), C.c_uint64(99), _lib.MrtxStats()
    assert bc.bowls_call(rt._lib, rt._ctx, bc.block(50, 60), z=z, n=n, rounds=rounds, st=st) == 0
    assert n.value == total and 0 < rounds.value < 20 and st.launches > 0
    # a table that is too small: nothing written, the needed size named, n_bowls set
    rec, lab = np.zeros(total, bs.BOWL_DTYPE), np.zeros((50, 60), np.int32)
    n = C.c_uint64(0)
    assert bc.bowls_call(rt._lib, rt._ctx, bc.block(50, 60), z=z, bowls=rec, cap=total - 1, label=lab, n=n) == -1
    msg = rt._lib.mrtx_last_error(rt._ctx).decode()
    assert f"{total} bowls are needed (bowl_cap = {total - 1})" in msg, msg
    assert n.value == total and (rec.view(np.uint8) == 0).all() and (lab == 0).all()
    # exactly enough, and more than enough
    for cap in (total, total + 7):
        rec = np.zeros(cap, bs.BOWL_DTYPE)
        assert bc.bowls_call(rt._lib, rt._ctx, bc.block(50, 60), z=z, bowls=rec, cap=cap, label=lab, n=n) == 0
        assert n.value == total and (rec[:total] == want).all() and (rec[total:].view(np.uint8) == 0).all()
        assert (lab == want_labels).all()
    # without labels the records are the same
    got = run(rt, case, False, None, False, labels=False)
    assert got.labels is None and (got.records == want).all()
    got = run(rt, case, False, None, True, labels=False)
    assert got.labels is None and (got.records == want).all()


# ---- stage hygiene
def test_every_refusal_has_its_text(rt):
    z, outlet, rec, lab = bc.refusal_tables()
    dev = DeviceBuffer(16384)
    try:
        for text, kw in bc.refusals(z, outlet, rec, lab, dev.ptr):
            bc.assert_refused(rt._lib, rt._ctx, text, kw, (rec, lab))
    finally:
        dev.free()
    with pytest.raises(ValueError):
        rt.bowls(np.zeros((3, 3, 2), np.int32))
    with pytest.raises(ValueError):
        rt.bowls(np.zeros((3, 3), np.float32))
    with pytest.raises(ValueError):
        rt.bowls(np.zeros((3, 3), np.int32), outlets=np.zeros((3, 4), np.uint8))
    with pytest.raises(ValueError):
        rt.bowls(np.zeros((3, 3), np.int32), row_weights=np.ones(4, np.uint32))


def test_leaves_the_render_state_alone(native_lib):
    s = named_scene("S1", 16, 16).with_size(48, 32, spp_per_launch=16)
    dem = mc.crater_dem()
    case = bc.random_case(61, 40, 70, 8, True, -9, 9, table_share=0.01)
    want, want_labels = bm.bowls(*case)

    def go(with_bowls):
        r = make(s, dem, _lib.F_COUNT_STATS)
        st1 = r.render(1)
        if with_bowls:
            for device in (False, True):
                assert_tree_equal(run(r, case, False, None, device), want, want_labels, ("between two renders", device))
        st2 = r.render(1)
        out = r.read_linear(), r.read_hits(), r.samples_done(), st1, st2
        r.close()
        return out
    a, b = go(False), go(True)
    assert_bit_equal(b[0], a[0], "linear radiance")
    assert_bit_equal(b[1], a[1], "hit buffer")
    assert b[2] == a[2] == 32
    for k in ("primary_hits", "shadow_rays", "height_samples", "bounce_rays"):
        assert b[4][k] == a[4][k], k


# ---- the identities, device against device
def synthetic_window(n):
    """(n, n) int32 heights of a rolling terrain with craters, in units of 0.25 m."""
    i, j = np.indices((n, n)).astype(np.float64)
    rng = np.random.default_rng(81)
    h = 300.0 * np.sin(i / 61.0) * np.cos(j / 47.0) + 40.0 * rng.standard_normal((n, n))
    for _ in range(60):
        ci, cj, r = rng.uniform(0, n), rng.uniform(0, n), rng.uniform(4, 40)
        d2 = ((i - ci) ** 2 + (j - cj) ** 2) / (r * r)
        h -= 8.0 * r * np.exp(-d2) - 3.0 * r * np.exp(-(np.sqrt(d2) - 1.0) ** 2 * 8.0)
    return bs.quantise_heights(h, 0.25)


def test_the_fill_of_the_tree_is_the_fill(rt):
    z = synthetic_window(512)
    w = weights_for(512)
    for conn, wrap in ((8, False), (4, True)):
        tree = rt.bowls(z, connectivity=conn, wrap=wrap, row_weights=w, unit_m=0.25)
        m = rt.fill_depressions(z, connectivity=conn, wrap=wrap, unit_m=0.25)
        assert tree.n > 1000 and (tree.fill() == m.fill).all()
        r = tree.records
        roots = tree.roots()
        # the root bowls' volumes sum to the volume of the fill
        depth = m.depth().astype(np.int64)
        exact = sum(int(w[i]) * int(depth[i].sum()) for i in range(512))
        assert sum(int(v) for v in r["volume"][roots]) % 2 ** 64 == exact % 2 ** 64
        # identity 3
        p = r["parent"]
        has = p >= 0
        assert (p[has] > np.flatnonzero(has)).all()
        kids = np.zeros(tree.n, np.uint64)
        np.add.at(kids, p[has], r["count"][has].astype(np.uint64))
        assert (r["own_count"] + kids == r["count"]).all()
        kids[:] = 0
        np.add.at(kids, p[has], r["n_leaves"][has].astype(np.uint64))
        assert (np.where(r["n_children"] == 0, 1, kids) == r["n_leaves"]).all()
        assert int(r["own_count"].sum()) == int((tree.labels >= 0).sum())
        # the selected root bowls as regions of the basin catalogue: each pours at its spill level
        sel = np.zeros(tree.n, bool)
        sel[roots] = True
        sel &= tree.select(min_depth_m=2.0, min_count=4)
        assert sel.sum() > 3
        table, bowl_of = tree.relabel(sel, innermost=False)
        assert (bowl_of == np.flatnonzero(sel)).all()
        basins = rt.basins(table, len(bowl_of), m, row_weights=w)
        assert (basins["pour_level"] == r["spill_level"][bowl_of]).all()
        assert (basins["count"] == r["count"][bowl_of]).all() and (basins["weight"] == r["weight"][bowl_of]).all()
        assert (basins["volume"] == r["volume"][bowl_of]).all()
        peaks = rt.peaks(z, connectivity=conn, wrap=wrap)
        assert peaks.invert and peaks.n > 1000 and (peaks.records["floor_level"] >= peaks.records["spill_level"]).all()


def test_the_bowl_tool(native_lib, tmp_path):
    """tools/bowl_catalogue.py end to end on a window of a small synthetic DEM."""
    import csv
    import subprocess
    import sys
    from moonrtx_amd.renderer import dem_from_ldem, synth_ldem
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import bowl_catalogue as tool
    dem_hw, window = (512, 1024), (100, 200, 48, 70, 2)
    for peaks in (False, True):
        paths = {k: str(tmp_path / f"{k}{int(peaks)}.{'csv' if k == 'csv' else 'npy'}") for k in ("csv", "labels")}
        cmd = [sys.executable, os.path.join(root, "tools", "bowl_catalogue.py"), "--window", *[str(v) for v in window], "--dem-size",
               *[str(v) for v in dem_hw], "--unit-m", "0.25", "--unit-m2", "4", "--min-depth-m", "10", "--csv", paths["csv"],
               "--labels", paths["labels"]] + (["--peaks"] if peaks else [])
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stdout + p.stderr
        # the same heights here
        src = synth_ldem(*dem_hw)
        dem, scale = dem_from_ldem(src, *dem_hw, 1)
        src.free()
        r = MoonRT(16, 16)
        r.bind_dem(dem, *dem_hw)
        radius_m = 1737400.0 * float(scale)
        z = bs.quantise_heights((r.traverse_heights(window).astype(np.float64) - 1.0) * radius_m, 0.25)
        lat, lon, _ = r.traverse_nodes(window)
        r.close()
        dem.free()
        from moonrtx_amd import regions as rg
        w = rg.row_weights(window, dem_hw, radius_m, 4.0)
        want, want_labels = bm.bowls(z, 8, False, True, None, peaks, w)
        tree = bs.BowlTree(want, want_labels, z, 0.25, 8, False, peaks)
        keep = tree.select(min_depth_m=10.0)
        assert 0 < keep.sum() <= tree.n
        with open(paths["csv"]) as f:
            got = list(csv.reader(f))
        rows = [[str(c) for c in row] for row in tool.catalogue_rows(tree, keep, lat, lon, 4.0)]
        assert got[0] == (tool.PEAK_HEADER if peaks else tool.HEADER) and got[1:] == rows
        assert (np.load(paths["labels"]) == tree.relabel(keep)[0]).all()
