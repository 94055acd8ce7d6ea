"""The terrain depressions on the GPU: mrtx_fill / MoonRT.fill_depressions and mrtx_fill_basins /
MoonRT.basins against tests/fill_model.py.  The fill and every field of every basin record are compared with ==, in both
variants (MOONRT_FILL = tiles, sweep), from host and from device tables.

One tile edge is built, TS = 32, so the sizes are those of the issue: 33 x 65 has a last tile one node high and one node
wide, 64 x 64 and 96 x 96 have tile borders at 32 and 64, and the wrapped lattices of 3, 64 and 65 columns have one tile that is
its own neighbour, two tiles that are each other's on both sides, and a last tile one node wide next to the seam.  Launch and
visit counts of the tiled variant may differ from run to run, so no test fixes them."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import fill_cases as fc
import fill_model as fm
import model_cases as mc
import regions_model as rm
from common import assert_bit_equal
from moonrtx_amd import _lib
from moonrtx_amd import basins as bs
from moonrtx_amd.renderer import DeviceBuffer, MoonRT, MoonRTError
from moonrtx_amd.scene import named_scene
from test_gpu_illumination import make

pytestmark = pytest.mark.gpu

VARIANTS = ("tiles", "sweep")


@pytest.fixture(scope="module")
def rt(native_lib):
    """One context for the module, without a DEM, a light or a Moon frame: the stage needs none of them."""
    r = MoonRT(16, 16)
    yield r
    r.close()


@contextlib.contextmanager
def variant(name):
    """MOONRT_FILL = name (None: unset) for the calls inside."""
    old = os.environ.get("MOONRT_FILL")
    try:
        if name is None:
            os.environ.pop("MOONRT_FILL", None)
        else:
            os.environ["MOONRT_FILL"] = name
        yield
    finally:
        if old is None:
            os.environ.pop("MOONRT_FILL", None)
        else:
            os.environ["MOONRT_FILL"] = old


def weights_for(rows):
    """distinct per row and near 2^32, so that weight and volume need 64 bits and volume wraps on a deep basin"""
    return (2 ** 32 - 1 - 3 * np.arange(rows)).astype(np.uint32)


def on_device(a):
    buf = DeviceBuffer(max(a.nbytes, 4))
    buf.upload(np.ascontiguousarray(a))
    return buf


def run_fill(rt, case, device, stats=None):
    z, conn, wrap, edge, table = case
    if not device:
        return rt.fill_depressions(z, table, edge, conn, wrap, stats=stats)
    zb, tb = on_device(z), on_device(table) if table is not None else None
    try:
        return rt.fill_depressions(zb, tb, edge, conn, wrap, shape=z.shape, stats=stats)
    finally:
        zb.free()
        if tb is not None:
            tb.free()


def run_basins(rt, labels, n, z, fill, conn, wrap, weights, device):
    if not device:
        return rt.basins(labels, n, (z, fill), weights, conn, wrap)
    bufs = [on_device(np.ascontiguousarray(a, np.int32)) for a in (labels, z, fill)]
    try:
        return rt.basins(bufs[0], n, (bufs[1], bufs[2]), weights, conn, wrap, shape=labels.shape)
    finally:
        for b in bufs:
            b.free()


def assert_fill_equal(got, want, what):
    assert got.shape == want.shape and got.dtype == np.int32, what
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, len(bad), bad[0].tolist(), int(got[tuple(bad[0])]), int(want[tuple(bad[0])]))


def assert_basins_equal(got, want, what):
    assert got.shape == want.shape and got.dtype == bs.BASIN_DTYPE, (what, got.shape, want.shape)
    for name in bs.BASIN_DTYPE.names:
        bad = np.flatnonzero(got[name] != want[name])
        assert bad.size == 0, (what, name, int(bad[0]), got[bad[0]], want[bad[0]])


def check_fill(rt, case, what):
    """Both variants, from host and from device tables, against the model: so the two variants give the same bytes."""
    z, conn, wrap, edge, table = case
    want = fm.fill(z, conn, wrap, edge, table)
    for v in VARIANTS:
        with variant(v):
            for device in (False, True):
                st = {}
                got = run_fill(rt, case, device, st)
                assert_fill_equal(got.fill, want, (what, v, device))
                assert (got.z == z).all() and got.connectivity == conn and got.wrap == bool(wrap)
                assert st["launches"] > 0 and st["kernel_ms"] > 0.0 and st["visits"] >= 0
    return want


def check_basins(rt, labels, n, z, fill, conn, wrap, what, depression=False):
    """With and without row weights, from host and from device tables, against the model."""
    labels = np.ascontiguousarray(labels, np.int32)
    w = weights_for(labels.shape[0])
    for weights in (w, None):
        want = fm.basins(labels, n, z, fill, conn, wrap, weights)
        for device in (False, True):
            got = run_basins(rt, labels, n, z, fill, conn, wrap, weights, device)
            assert_basins_equal(got, want, (what, weights is not None, device))
            if depression:
                assert (got["level_min"] == got["level_max"]).all() and (got["level_min"] == got["pour_level"]).all(), what
                assert (got["count"] > 0).all() and (got["depth_max"] > 0).all() and (got["pour_at"] >= 0).all(), what


def check(rt, case, what):
    """The fill, then the catalogue of its depressions, labelled by rt.regions at the fill's connectivity and wrap."""
    z, conn, wrap, edge, table = case
    fill = check_fill(rt, case, what)
    if (fill == fm.NONE).any():
        return fill
    m = bs.FillMap(z, fill, None, conn, wrap)
    regions = rt.regions(mask=m.mask(), connectivity=conn, wrap=wrap)
    labels, n = rm.label(m.mask(), conn, wrap)
    assert regions.n == n and (regions.labels == labels).all(), what
    check_basins(rt, regions.labels, regions.n, z, fill, conn, wrap, what, depression=True)
    return fill


# ---- thin and ragged lattices
THIN = {
    "1x1": (1, 1, False), "1x40": (1, 40, False), "40x1": (40, 1, False), "33x65": (33, 65, False), "96x130": (96, 130, False),
    "5x3_wrapped": (5, 3, True), "40x64_wrapped": (40, 64, True), "37x65_wrapped": (37, 65, True),
}


@pytest.mark.parametrize("name", sorted(THIN))
def test_thin_and_ragged_lattices(rt, name):
    rows, cols, wrap = THIN[name]
    for conn in (4, 8):
        check(rt, fc.random_case(11, rows, cols, conn, wrap, -6, 6), (name, conn, "edges"))
        check(rt, fc.random_case(12, rows, cols, conn, wrap, -6, 6, table_share=0.02), (name, conn, "edges and table"))
        check(rt, fc.random_case(13, rows, cols, conn, wrap, -6, 6, table_share=0.05, edge=False), (name, conn, "table only"))


# ---- tile hand-offs
@pytest.mark.parametrize("n", (64, 96))
@pytest.mark.parametrize("transposed", (False, True))
def test_the_level_travels_a_serpentine_channel(rt, n, transposed):
    for conn in (4, 8):
        case = fc.serpentine(n, conn, transposed)
        fill = check(rt, case, ("serpentine", n, conn, transposed))
        z = case[0]
        assert (fill[z < fc.WALL] == 5).all() and (fill[z == fc.WALL] == fc.WALL).all()


@pytest.mark.parametrize("kind,n", (("main", 64), ("anti", 64), ("main", 96), ("anti", 96), ("wrapped", 64)))
def test_diagonal_channels_drain_through_tile_corners_at_eight_only(rt, kind, n):
    case = fc.diagonal(n, 8, kind)
    z, table = case[0], case[4]
    fill = check(rt, case, ("diagonal", kind, n, 8))
    assert (fill[z < fc.WALL] == 5).all()
    fill = check(rt, fc.diagonal(n, 4, kind), ("diagonal", kind, n, 4))
    assert (fill[(z < fc.WALL) & (table == 0)] == fc.WALL).all()


# ---- flats
def test_flats(rt):
    for conn in (4, 8):
        assert (check(rt, fc.flat(70, 96, conn), ("flat", conn)) == 3).all()
        assert (check(rt, fc.flat(40, 64, conn, True), ("flat wrapped", conn)) == 3).all()
        fill = check(rt, fc.flat_basin(96, conn), ("flat basin", conn))
        assert (fill[1:-1, 1:-1] == 7).all()
        check(rt, fc.checkerboard(67, 70, conn), ("checkerboard", conn))
        check(rt, fc.checkerboard(34, 64, conn, True), ("checkerboard wrapped", conn))


# ---- random heights
@pytest.mark.parametrize("conn,wrap", ((8, False), (4, True)))
@pytest.mark.parametrize("span", ("ties", "full"))
def test_random_heights(rt, span, conn, wrap):
    lo, hi = (-5, 5) if span == "ties" else (-2 ** 30, 2 ** 30)
    case = fc.random_case(21, 256, 256, conn, wrap, lo, hi)
    z = case[0]
    z[100, 100], z[200, 17] = 2 ** 30, -2 ** 30                 # the bound itself is accepted
    fill = check_fill(rt, case, ("random", span, conn, wrap))
    if span == "ties" and conn == 8:
        m = bs.FillMap(z, fill, None, conn, wrap)
        regions = rt.regions(mask=m.mask(), connectivity=conn, wrap=wrap)
        assert regions.n > 100
        check_basins(rt, regions.labels, regions.n, z, fill, conn, wrap, ("random", span), depression=True)


def test_a_height_beyond_the_bound(rt):
    z, conn, wrap, edge, table = fc.random_case(22, 40, 50, 8, False, -9, 9)
    fill = np.zeros_like(z)
    for v in VARIANTS:
        with variant(v):
            for at, bad in (((0, 0), 2 ** 30 + 1), ((39, 49), -2 ** 30 - 1), ((20, 20), 2 ** 31 - 1), ((7, 3), -2 ** 31)):
                mine = z.copy()
                mine[at] = bad
                # from host memory: before any launch, at its first occurrence
                st = _lib.MrtxStats()
                st.launches = 0xABCD
                assert fc.fill_call(rt._lib, rt._ctx, fc.block(40, 50), z=mine, fill=fill, st=st) == -1
                msg = rt._lib.mrtx_last_error(rt._ctx).decode()
                assert f"height {at[0] * 50 + at[1]} must lie in -2^30 .. 2^30 (got {bad})" in msg, msg
                assert st.launches == 0xABCD and (fill == 0).all()
                # from a device table: after the launches, counted
                with pytest.raises(MoonRTError, match="1 heights of the device table lie outside"):
                    run_fill(rt, (mine, conn, wrap, edge, table), True)
                with pytest.raises(MoonRTError, match="must lie in -2\\^30"):
                    run_basins(rt, np.zeros_like(z), 1, mine, z, 8, False, None, False)
                with pytest.raises(MoonRTError, match="1 heights of the device table lie outside"):
                    run_basins(rt, np.zeros_like(z), 1, mine, z, 8, False, None, True)
    check(rt, (z, conn, wrap, edge, table), "afterwards")


# ---- outlets
def test_outlet_sources(rt):
    rng = np.random.default_rng(31)
    z = rng.integers(-8, 9, (70, 75)).astype(np.int32)
    table = (rng.random(z.shape) < 0.01).astype(np.uint8) * 7          # any nonzero byte is an outlet
    for conn, wrap in ((4, False), (8, True)):
        check(rt, (z, conn, wrap, False, table), ("table only", conn, wrap))
        check(rt, (z, conn, wrap, True, table), ("table and edges", conn, wrap))
        none = check_fill(rt, (z, conn, wrap, False, np.zeros_like(table)), ("no outlet", conn, wrap))
        assert (none == _lib.FILL_NONE).all()
        # the basins of a fill without outlets: depths up to INT32_MAX, one region over the whole lattice has no pour point
        check_basins(rt, np.zeros_like(z), 1, z - 2 ** 30 + 8, none, conn, wrap, ("no outlet", conn, wrap))
    # an outlet in the deepest node of a pit drains it
    z = np.full((40, 45), 9, np.int32)
    z[10:30, 10:35] = 3
    z[20, 33] = 1
    sink = fc.one_outlet(z.shape, (20, 33))
    assert (check(rt, (z, 8, False, True, sink), "sink") == z).all()
    assert (check(rt, (z, 8, False, True, None), "no sink")[10:30, 10:35] == 9).all()


# ---- basins of any label table
def test_basins_of_a_callers_labels(rt):
    rng = np.random.default_rng(41)
    z = rng.integers(-20, 21, (67, 70)).astype(np.int32)
    for conn, wrap in ((4, True), (8, False)):
        fill = fm.fill(z, conn, wrap)
        mine = np.where(rng.random(z.shape) < 0.7, rng.integers(0, 5, z.shape), -1).astype(np.int32)    # disconnected labels
        mine[mine == 3] = 4                                             # a label that no node carries
        check_basins(rt, mine, 6, z, fill, conn, wrap, ("mine", conn, wrap))
        got = rt.basins(mine, 6, (z, fill), None, conn, wrap)
        for r in (3, 5):
            assert got[r].tolist() == (0, 0, 0, 2 ** 31 - 1, -2 ** 31, 0, -1, -1, 2 ** 31 - 1, 0)
        check_basins(rt, np.zeros_like(z), 1, z, fill, conn, wrap, ("whole", conn, wrap))
        whole = rt.basins(np.zeros_like(z), 1, (z, fill), None, conn, wrap)[0]
        assert whole["pour_at"] == -1 and whole["pour_level"] == 2 ** 31 - 1 and whole["count"] == z.size
        # any fill table: one below the heights gives depth 0
        check_basins(rt, mine, 6, z, z - 3, conn, wrap, ("a fill below the heights", conn, wrap))


def test_volume_wraps_modulo_two_to_the_64(rt):
    z = np.full((40, 40), 2 ** 30, np.int32)
    z[1:-1, 1:-1] = -2 ** 30 + 1
    fill = fm.fill(z, 8)
    labels = np.where(z < 0, 0, -1).astype(np.int32)
    w = weights_for(40)
    want = fm.basins(labels, 1, z, fill, 8, False, w)
    exact = sum(int(w[i]) * 38 * (2 ** 31 - 1) for i in range(1, 39))
    assert exact >= 2 ** 64 and int(want[0]["volume"]) == exact % 2 ** 64 and want[0]["depth_max"] == 2 ** 31 - 1
    check_basins(rt, labels, 1, z, fill, 8, False, "deep")


def test_a_bad_label_table_is_refused_after_the_launch(rt):
    rng = np.random.default_rng(43)
    z = rng.integers(-9, 10, (40, 50)).astype(np.int32)
    fill = fm.fill(z, 8)
    labels, n = rm.label(fill > z, 8)
    out = np.zeros(n, bs.BASIN_DTYPE)
    for bad in (n, n + 1000, 2 ** 31 - 1, -2, -2 ** 31):
        mine = labels.copy()
        mine[17, 23] = bad
        st = _lib.MrtxStats()
        assert fc.basins_call(rt._lib, rt._ctx, 40, 50, 0, 8, labels=mine, n=n, z=z, fill=fill, out=out, st=st) == -1, bad
        assert "1 entries outside -1" in rt._lib.mrtx_last_error(rt._ctx).decode()
        assert st.launches == 3
        with pytest.raises(MoonRTError, match="entries outside -1"):
            run_basins(rt, mine, n, z, fill, 8, False, None, True)
    # no regions: the table is checked, nothing is written
    none = np.full((40, 50), -1, np.int32)
    assert rt.basins(none, 0, (z, fill)).shape == (0,)
    assert run_basins(rt, none, 0, z, fill, 8, False, None, True).shape == (0,)
    one = none.copy()
    one[2, 2] = 0
    with pytest.raises(MoonRTError, match="entries outside -1"):
        rt.basins(one, 0, (z, fill))
    check_basins(rt, labels, n, z, fill, 8, False, "afterwards", depression=True)


# ---- stage hygiene
def test_every_refusal_has_its_text(rt):
    z, outlet, fill, labels, out = fc.refusal_tables()
    dev = DeviceBuffer(8192)
    try:
        with variant(None):
            for text, kw in fc.fill_refusals(z, outlet, fill, dev.ptr):
                fc.assert_refused(rt._lib, rt._ctx, fc.fill_call, text, kw, (fill,))
            for text, kw in fc.basins_refusals(labels, z, fill, out, dev.ptr):
                fc.assert_refused(rt._lib, rt._ctx, fc.basins_call, text, kw, (out,))
        with variant("quick"):
            fc.assert_refused(rt._lib, rt._ctx, fc.fill_call, "MOONRT_FILL must be tiles or sweep \\(got quick\\)",
                              dict(z=z, fill=fill, f=fc.block()), (fill,))
    finally:
        dev.free()
    with pytest.raises(ValueError):
        rt.fill_depressions(np.zeros((3, 3, 2), np.int32))
    with pytest.raises(ValueError):
        rt.fill_depressions(np.zeros((3, 3), np.float32))
    with pytest.raises(ValueError):
        rt.fill_depressions(np.zeros((3, 3), np.int32), outlets=np.zeros((3, 4), np.uint8))
    with pytest.raises(ValueError):
        rt.basins(np.zeros((3, 3), np.int32), 1, (np.zeros((3, 3), np.int32), np.zeros((3, 4), np.int32)))


def test_the_catalogue_convenience(rt):
    z = fc.random_case(51, 60, 64, 8, True, -30, 30)[0]
    m = rt.fill_depressions(z, connectivity=8, wrap=True, unit_m=0.5)
    w = weights_for(60)
    regions, table = m.catalogue(rt, row_weights=w)
    labels, n = rm.label(m.mask(), 8, True)
    assert regions.n == n and n > 0 and regions.wrap and (regions.labels == labels).all()
    assert_basins_equal(table, fm.basins(labels, n, z, fm.fill(z, 8, True), 8, True, w), "catalogue")
    assert (table["weight"] == regions.table["weight"]).all() and (table["count"] == regions.table["count"]).all()
    # deeper than 5 m = 10 units: the floors alone, several to a depression where a sill between them is shallower
    deep, table2 = m.catalogue(rt, min_depth_m=5.0)
    labels2, n2 = rm.label(m.depth() > 10, 8, True)
    assert deep.n == n2 > 0 and (deep.labels == labels2).all()
    assert_basins_equal(table2, fm.basins(labels2, n2, z, m.fill, 8, True), "deep")
    assert (table2["level_min"] == table2["level_max"]).all() and (table2["depth_max"] > 10).all()
    assert int(table2["count"].sum()) < int(table["count"].sum())


def test_leaves_the_render_state_alone(native_lib):
    s = named_scene("S1", 16, 16).with_size(48, 32, spp_per_launch=16)
    dem = mc.crater_dem()
    case = fc.random_case(61, 40, 70, 8, True, -9, 9, table_share=0.01)
    want = fm.fill(*case)

    def go(with_fill):
        r = make(s, dem, _lib.F_COUNT_STATS)
        st1 = r.render(1)
        if with_fill:
            for v in VARIANTS:
                with variant(v):
                    got = run_fill(r, case, v == "sweep")
                    assert_fill_equal(got.fill, want, ("between two renders", v))
            got.catalogue(r, row_weights=weights_for(40))
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


def test_the_depression_tool(native_lib, tmp_path):
    """tools/depression_catalogue.py end to end on a window of a small synthetic DEM."""
    import csv
    import subprocess
    import sys
    from moonrtx_amd import regions as rg
    from moonrtx_amd.renderer import dem_from_ldem, synth_ldem
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import depression_catalogue as tool
    dem_hw, window = (512, 1024), (100, 200, 48, 70, 2)
    rng = np.random.default_rng(71)
    outlets = (rng.random((48, 70)) < 0.002).astype(np.uint8)
    np.save(tmp_path / "outlets.npy", outlets)
    paths = {k: str(tmp_path / f"{k}.{'csv' if k == 'csv' else 'npy'}") for k in ("fill", "depth", "csv", "labels")}
    cmd = [sys.executable, os.path.join(root, "tools", "depression_catalogue.py"), "--window", *[str(v) for v in window], "--dem-size",
           *[str(v) for v in dem_hw], "--unit-m", "0.25", "--unit-m2", "4", "--min-depth-m", "1", "--min-area-km2", "1000", "--outlets",
           str(tmp_path / "outlets.npy"), "--fill", paths["fill"], "--depth", paths["depth"], "--csv", paths["csv"], "--labels",
           paths["labels"]]
    env = dict(os.environ)
    env.pop("MOONRT_FILL", None)
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=env)
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
    fill = fm.fill(z, 8, False, True, outlets)
    depth = np.array(fm.depth(fill, z), np.int32)
    assert (np.load(paths["fill"]) == fill).all() and (np.load(paths["depth"]) == depth).all() and (depth > 4).any()
    labels, n = rm.label(depth * 0.25 > 1.0, 8, False)
    w = rg.row_weights(window, dem_hw, radius_m, 4.0)
    table = fm.basins(labels, n, z, fill, 8, False, w)
    keep = table["weight"].astype(np.float64) * 4.0 >= 1000e6
    assert 0 < keep.sum() <= n
    with open(paths["csv"]) as f:
        got = list(csv.reader(f))
    want = [[str(c) for c in row] for row in tool.catalogue_rows(table[keep], 70, lat, lon, 0.25, 4.0)]
    assert got[0] == tool.HEADER and got[1:] == want
    vol = [float(row[9]) for row in got[1:]]
    assert vol == sorted(vol, reverse=True)
    new = np.where(keep, np.cumsum(keep) - 1, -1)
    assert (np.load(paths["labels"]) == np.where(labels >= 0, new[labels], -1)).all()
