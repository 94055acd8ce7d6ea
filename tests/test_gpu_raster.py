"""The polygon rasterisation on the GPU: mrtx_rasterise / MoonRT.rasterise against
tests/raster_model.py, and round trips through the region outlines.  Every label and every field of every cover record is
compared with ==."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import model_cases as mc
import outline_model as om
import raster_cases as rc
import raster_model as rs
import regions_cases as gc
from common import assert_bit_equal
from moonrtx_amd import _lib
from moonrtx_amd import regions as rg
from moonrtx_amd.renderer import DeviceBuffer, MoonRT, MoonRTError
from moonrtx_amd.scene import named_scene
from test_gpu_illumination import make
from test_gpu_zonal import label_cases

pytestmark = pytest.mark.gpu

VARIANTS = ("bins", "brute")
RULES = ("nonzero", "evenodd")
ORDERS = ("first", "last")


@pytest.fixture(scope="module")
def rt(native_lib):
    """One context for the module, without a DEM, a light or a Moon frame: the stage needs none of them."""
    r = MoonRT(16, 16)
    yield r
    r.close()


@contextlib.contextmanager
def variant(name):
    """MOONRT_RASTER = name (None: unset) for the calls inside."""
    old = os.environ.get("MOONRT_RASTER")
    try:
        if name is None:
            os.environ.pop("MOONRT_RASTER", None)
        else:
            os.environ["MOONRT_RASTER"] = name
        yield
    finally:
        if old is None:
            os.environ.pop("MOONRT_RASTER", None)
        else:
            os.environ["MOONRT_RASTER"] = old


def run(rt, pg, shape, wrap, rule, order, weights, device, stats=None):
    if not device:
        return rt.rasterise(pg, shape, wrap, rule, order, weights, stats=stats)
    rb, vb = DeviceBuffer(max(pg.rings.nbytes, 24)), DeviceBuffer(max(pg.vertices.nbytes, 8))
    try:
        if len(pg):
            rb.upload(pg.rings)
        if pg.vertices.size:
            vb.upload(pg.vertices)
        return rt.rasterise((rb, len(pg), vb, pg.vertices.shape[0], pg.n_polygons, pg.subcell_bits), shape, wrap, rule, order, weights,
                            stats=stats)
    finally:
        rb.free()
        vb.free()


def assert_raster_equal(got, labels, cover, what):
    assert got[0].shape == labels.shape and got[0].dtype == np.int32, what
    bad = np.argwhere(got[0] != labels)
    assert bad.size == 0, (what, "label", bad[0].tolist(), int(got[0][tuple(bad[0])]), int(labels[tuple(bad[0])]))
    assert got[1].shape == cover.shape, (what, got[1].shape, cover.shape)
    for name in rg.COVER_DTYPE.names:
        bad = np.flatnonzero(got[1][name] != cover[name])
        assert bad.size == 0, (what, name, int(bad[0]), got[1][bad[0]], cover[bad[0]])


def check(rt, pg, shape, wrap, what):
    """Both variants, from host and from device tables, under both rules and orders, with and without row weights near 2^32: every
    one against the model, so the two variants give the same bytes; and the count of the crossings."""
    rows, cols = shape
    w = rc.weights_for(rows)
    hits = rs.crossings(pg.rings, pg.vertices, rows, cols, wrap, pg.subcell_bits)
    for rule in RULES:
        for order in ORDERS:
            for weights in (w, None):
                want = rs.raster(pg.rings, pg.vertices, pg.n_polygons, rows, cols, wrap, pg.subcell_bits, RULES.index(rule),
                                 ORDERS.index(order), weights, hits=hits)
                for v in VARIANTS:
                    with variant(v):
                        for device in (False, True):
                            st = {}
                            got = run(rt, pg, shape, wrap, rule, order, weights, device, st)
                            assert_raster_equal(got, want[0], want[1], (what, v, rule, order, device, weights is not None))
                            assert st["crossings"] == want[2] == len(hits) and st["launches"] > 0, (what, v, st)


# ---- the built polygons: oblique and sub-cell geometry, and the layout's edges
def polygons_of(case):
    rings, n, rows, cols, wrap, s = case
    recs, verts = rs.polygons(rings)
    return rg.Polygons(recs, verts, n, s), (rows, cols), wrap


@pytest.mark.parametrize("name", rc.GEOMETRY)
def test_built_polygons_equal_the_model(rt, name):
    pg, shape, wrap = polygons_of(rc.geometry_cases()[name])
    check(rt, pg, shape, wrap, name)


def test_what_the_built_polygons_hold(rt):
    """The cases are what their names say, on the device."""
    cases = rc.geometry_cases()
    pg, shape, wrap = polygons_of(cases["two_triangles"])
    for rule in RULES:
        first, cover = rt.rasterise(pg, shape, wrap, rule, "first")
        last, _ = rt.rasterise(pg, shape, wrap, rule, "last")
        assert (first == last).all() and (first >= 0).all() and cover["count"].tolist() == cover["owned"].tolist() == [28, 36]
    pg, shape, wrap = polygons_of(cases["pentagram"])
    nz, eo = rt.rasterise(pg, shape, wrap, "nonzero")[0], rt.rasterise(pg, shape, wrap, "evenodd")[0]
    assert nz[10, 10] == 0 and eo[10, 10] == -1 and ((eo >= 0) <= (nz >= 0)).all()
    pg, shape, wrap = polygons_of(cases["overlapping"])
    first, cf = rt.rasterise(pg, shape, wrap)
    last, cl = rt.rasterise(pg, shape, wrap, order="last")
    assert first[6, 6] == 0 and last[6, 6] == 2 and cf["count"].tolist() == cl["count"].tolist()
    assert (cf["owned"] < cf["count"]).any() and int(cf["owned"].sum()) == int((first >= 0).sum())
    # the comb's first bin holds far more crossings than one staging chunk, and many_bins more bins than one chunk of the scan
    hits = rs.crossings(*rs.polygons(cases["comb"][0]), 80, 100)
    assert sum(1 for p, j, _, _ in hits if p == 0 and j < 64) == 4800 > 64
    assert cases["many_bins"][1] * -(-cases["many_bins"][3] // 64) > 2048
    hits = rs.crossings(*rs.polygons(cases["clipped_to_row_0"][0][:2]), 6, 16, False, 3)
    assert hits and all(i0 == 0 for _, _, i0, _ in hits)
    hits = rs.crossings(*rs.polygons(cases["edge_longer_than_cols"][0][:1]), 11, 10, True, 2)
    assert max(np.bincount([j for _, j, _, _ in hits])) >= 4


# ---- round trips: rasterising the outlines of a label table gives the table back
def closed_form_cover(labels, n, weights):
    rows, cols = labels.shape
    cover = np.zeros(n, rg.COVER_DTYPE)
    cover["i_min"] = cover["i_max"] = cover["first_at"] = -1
    w = np.ones(rows, np.uint64) if weights is None else weights.astype(np.uint64)
    ii, jj = np.nonzero(labels >= 0)
    lab = labels[ii, jj]
    for p in np.unique(lab).tolist():
        rws = ii[lab == p]
        at = (ii * cols + jj)[lab == p]
        total = sum(int(v) for v in w[rws].tolist())
        cover[p] = (total, total, rws.size, rws.size, int(rws.min()), int(rws.max()), int(at.min()), 0)
    return cover


def round_trip(rt, labels, n, wrap, what):
    """Through the model's rings and through the device's own region_outlines, at both connectivities and in both modes.  The
    model's corner rings at connectivity 4 take every combination of variant, side, rule, order and weights; the others both
    variants and both rules."""
    labels = np.ascontiguousarray(labels, np.int32)
    shape = labels.shape
    w = rc.weights_for(shape[0])
    want = {True: closed_form_cover(labels, n, w), False: closed_form_cover(labels, n, None)}
    for conn in (4, 8):
        for corners in (True, False):
            r, v = om.trace(labels, conn, wrap, om.CORNERS if corners else om.ALL)
            mine = rg.Polygons(rs.rings_of_outlines(r), v, n, 0)
            n_hits = len(rs.crossings(mine.rings, mine.vertices, shape[0], shape[1], wrap, 0))
            theirs = rt.region_outlines(labels, n, conn, wrap, corners).polygons(n)
            full = conn == 4 and corners
            for src, pg in (("model", mine), ("device", theirs)):
                every = full and src == "model"
                for v_ in VARIANTS:
                    with variant(v_):
                        for rule in RULES:
                            for order in (ORDERS if every else ORDERS[:1]):
                                for device in ((False, True) if every else (False,)):
                                    for weights in ((w, None) if every else (w,)):
                                        st = {}
                                        got = run(rt, pg, shape, wrap, rule, order, weights, device, st)
                                        assert_raster_equal(got, labels, want[weights is not None],
                                                            (what, conn, corners, src, v_, rule, order, device, weights is not None))
                                        assert st["crossings"] == n_hits, (what, conn, corners, src, v_, st)


BUILT = [c["name"] for c in gc.CASES]


@pytest.mark.parametrize("name", BUILT)
def test_round_trips_of_the_built_cases(rt, name):
    case = gc.BY_NAME[name]
    labels, n = gc.answer(case, 4)
    round_trip(rt, labels, n, case["wrap"], name)


def own_cases():
    """The cases of tests/test_gpu_outline.py that the issue names, rebuilt by name and shape."""
    out = {}
    out["1x1"] = (np.zeros((1, 1), np.int32), 1, False)
    out["1x3_wrapped_full"] = (np.zeros((1, 3), np.int32), 1, True)
    m = np.full((6, 7), -1, np.int32)
    m[1, 6] = m[2, 0] = 0
    m[4, 0] = m[5, 6] = 0
    out["saddle_on_the_seam"] = (m, 1, True)
    m = np.full((40, 130), -1, np.int32)
    m[15, 63] = m[16, 64] = 0
    m[15, 64] = m[16, 63] = 1
    out["saddle_on_a_tile_corner"] = (m, 2, False)
    m = np.full((7, 70), -1, np.int32)
    m[2:5, :] = 0
    out["band_round_the_seam"] = (m, 1, True)
    g = m.copy()
    g[2:5, 33] = -1
    out["band_with_a_gap"] = (g, 1, True)
    h = m.copy()
    h[3, 10:20] = -1
    h[3, 69] = -1
    out["band_with_holes"] = (h, 1, True)
    out["full_wrapped"] = (np.zeros((33, 65), np.int32), 1, True)
    out["2100_in_a_row"] = (np.zeros((1, 2100), np.int32), 1, True)
    out["16x1025"] = label_cases()["16x1025"]
    return out


OWN = ["1x1", "1x3_wrapped_full", "saddle_on_the_seam", "saddle_on_a_tile_corner", "band_round_the_seam", "band_with_a_gap",
       "band_with_holes", "full_wrapped", "2100_in_a_row", "16x1025"]


@pytest.mark.parametrize("name", OWN)
def test_round_trips_of_the_outline_cases(rt, name):
    labels, n, wrap = own_cases()[name]
    round_trip(rt, labels, n, wrap, name)


# ---- empty tables
def test_no_polygons_and_no_rings_give_an_empty_table(rt):
    none = rg.Polygons(np.zeros(0, rg.RASTER_RING_DTYPE), np.zeros((0, 2), np.int32), 0)
    three = rg.Polygons(np.zeros(0, rg.RASTER_RING_DTYPE), np.zeros((0, 2), np.int32), 3)
    empty = np.zeros(3, rg.COVER_DTYPE)
    empty["i_min"] = empty["i_max"] = empty["first_at"] = -1
    for v in VARIANTS:
        with variant(v):
            for device in (False, True):
                for order in ORDERS:
                    st = {}
                    labels, cover = run(rt, none, (5, 70), True, "nonzero", order, None, device, st)
                    assert (labels == -1).all() and labels.shape == (5, 70) and cover.shape == (0,) and st["crossings"] == 0
                    assert_raster_equal(run(rt, three, (5, 70), False, "evenodd", order, None, device), np.full((5, 70), -1, np.int32), empty,
                                        (v, device, order))


# ---- a scan of more than 256 chunks: the middle launch's threads each take a run of chunk sums
def test_more_polygons_than_one_thread_of_the_scan_takes_a_chunk_of(rt):
    n = 600000                                              # 293 chunks of 2 048: the bins (one strip) and brute's polygons alike
    u = 4
    rings = [(p, [(y * u + 1, x * u), (y * u, (x + 4) * u - 1), ((y + 3) * u, (x + 4) * u), ((y + 3) * u + 1, x * u + 2)])
             for p, y, x in ((0, 0, 0), (1, 1, 2), (2047, 2, 3), (2048, 3, 4), (299999, 4, 1), (524288, 1, 5), (n - 1, 5, 3), (n - 1, 0, 6))]
    recs, verts = rs.polygons(rings)
    pg = rg.Polygons(recs, verts, n, 2)
    w = rc.weights_for(9)
    for order in ORDERS:
        want = rs.raster(recs, verts, n, 9, 11, False, 2, rs.NONZERO, ORDERS.index(order), w)
        assert len(np.unique(want[0])) == 8 and int((want[1]["count"] > 0).sum()) == 7
        for v in VARIANTS:
            with variant(v):
                st = {}
                got = run(rt, pg, (9, 11), False, "nonzero", order, w, False, st)
                assert_raster_equal(got, want[0], want[1], (v, order))
                assert st["crossings"] == want[2]


# ---- the launches
def test_launches_are_equal_for_a_case_and_its_mirror_image(rt):
    cases = rc.geometry_cases()
    seen = {}
    for name in ("overlapping", "width_65", "across_the_seam", "comb", "many_bins"):
        for v in VARIANTS:
            with variant(v):
                counts = []
                for case in (cases[name], rc.mirrored(cases[name])):
                    pg, shape, wrap = polygons_of(case)
                    st = {}
                    rt.rasterise(pg, shape, wrap, stats=st)
                    assert st["launches"] > 0 and st["kernel_ms"] > 0.0
                    counts.append(st["launches"])
                assert counts[0] == counts[1], (name, v, counts)
                seen.setdefault(v, set()).add(counts[0])
    # ... and depend on the variant alone
    assert all(len(s) == 1 for s in seen.values()), seen


# ---- what the call refuses
def raster_call(rt, r, **kw):
    return rc.raster_call(rt._lib, rt._ctx, r, **kw)


def test_every_refusal(rt):
    """Each text, the count and the statistics as they were, no table touched, on the host or on the device (that no refusal
    makes a device call is shown without a device, in tests/test_raster_host.py)."""
    rings, vertices, labels, cover = rc.refusal_tables()
    dev = DeviceBuffer(8192)
    fill = np.full(8192, 0xAB, np.uint8)
    try:
        dev.upload(fill)
        for text, kw in rc.refusal_cases(rings, vertices, labels, cover, dev.ptr):
            with variant(None):
                rc.assert_refused(rt._lib, rt._ctx, text, kw, labels, cover)
        F = dict(rings=rings, vertices=vertices, labels=labels, cover=cover, r=rc.block())
        D = dict(dev_rings=dev.ptr, n_rings=2, dev_vertices=dev.ptr + 64, n_vertices=8, dev_labels=dev.ptr + 512, dev_cover=dev.ptr + 1024,
                 r=rc.block())
        for kw in (F, D):
            with variant("fast"):
                rc.assert_refused(rt._lib, rt._ctx, "MOONRT_RASTER must be bins or brute \\(got fast\\)", kw, labels, cover)
        assert (dev.download(np.uint8, (8192,)) == 0xAB).all()
        with variant("fast"), pytest.raises(MoonRTError, match="MOONRT_RASTER must be bins or brute"):
            rt.rasterise(rg.Polygons(rings, vertices, 1), (8, 9))
        # the context still works, and the tables of the refusals are good ones
        pg = rg.Polygons(rings, vertices, 1)
        check(rt, pg, (8, 9), False, "after the refusals")
    finally:
        dev.free()


def bad_tables():
    """[(what is wrong, rings, vertices, the two counts of the message)] for an 8 x 9 lattice with wrap and one polygon."""
    rings, vertices, _, _ = rc.refusal_tables()
    out = []

    def ring(what, bad_rings=1, bad_coords=0, v=None, **fields):
        r = rings.copy()
        for k, val in fields.items():
            r[k][1] = val
        out.append((what, r, vertices if v is None else v, bad_rings, bad_coords))
    ring("polygon out of range", polygon=1)
    ring("polygon negative", polygon=-1)
    ring("beyond the table", first=5)
    ring("first far beyond the table", first=2 ** 63)
    ring("no vertices", n_vertices=0)
    ring("a wind of 2", wind=2)
    ring("a wind of -2", wind=-2)
    ring("reserved", reserved=7)
    for val in (2 ** 24 + 1, -2 ** 24 - 1, 2 ** 31 - 1, -2 ** 31):
        v = vertices.copy()
        v[6, 1] = val
        ring(f"a coordinate of {val}", 0, 1, v)
    v = vertices.copy()
    v[0] = (2 ** 30, -2 ** 30)
    r = rings.copy()
    r["polygon"][0] = 5
    out.append(("two coordinates and a ring", r, v, 1, 2))
    v = vertices.copy()
    v[4:, 1] = (2 ** 24, 2 ** 24 - 1, 2 ** 24 - 1, 2 ** 24 - 2)     # legal, and so is the closing point where a turn is short
    r = rings.copy()
    r["wind"][1] = 1
    out.append(("closing point", r, v, 0, 0))
    return out


def test_a_bad_table_is_refused_after_the_launch_with_nothing_written(rt):
    for v in VARIANTS:
        with variant(v):
            for what, rings, vertices, bad_rings, bad_coords in bad_tables():
                if what == "closing point":             # good where a turn is 9 units; bad where it is 2^24 + 256 and leaves 2^25
                    blocks = [(rc.block(wrap=1, s=0), None), (rc.block(rows=1, cols=2 ** 16 + 1, wrap=1, s=8), (1, 0))]
                else:
                    blocks = [(rc.block(wrap=1), (bad_rings, bad_coords))]
                for r, counts in blocks:
                    N = r.rows * r.cols
                    labels, cover = np.full(N, 0x5A5A5A5A, np.int32), np.zeros(1, rg.COVER_DTYPE)
                    cover.view(np.uint8)[:] = 0xAB
                    lb, cb = DeviceBuffer(4 * N), DeviceBuffer(40)
                    rb, vb = DeviceBuffer(rings.nbytes), DeviceBuffer(vertices.nbytes)
                    try:
                        lb.upload(labels)
                        cb.upload(cover)
                        rb.upload(rings)
                        vb.upload(vertices)
                        for device in (False, True):
                            crossings, st = C.c_uint64(5), _lib.MrtxStats()
                            if device:
                                code = raster_call(rt, r, dev_rings=rb.ptr, n_rings=2, dev_vertices=vb.ptr, n_vertices=8, dev_labels=lb.ptr,
                                                   dev_cover=cb.ptr, crossings=crossings, st=st)
                            else:
                                code = raster_call(rt, r, rings=rings, vertices=vertices, labels=labels, cover=cover, crossings=crossings, st=st)
                            if counts is None:
                                assert code == 0, (what, v, device, rt._lib.mrtx_last_error(rt._ctx).decode())
                                labels[:] = 0x5A5A5A5A
                                cover.view(np.uint8)[:] = 0xAB
                                lb.upload(labels)
                                cb.upload(cover)
                                continue
                            msg = rt._lib.mrtx_last_error(rt._ctx).decode()
                            assert code == -1, (what, v, device)
                            assert f"holds {counts[0]} bad records and the vertex table {counts[1]} coordinates outside" in msg, (what, msg)
                            assert crossings.value == 5 and st.launches > 0, (what, v, device)
                            assert (labels == 0x5A5A5A5A).all() and (cover.view(np.uint8) == 0xAB).all(), (what, v, device)
                            assert (lb.download(np.int32, (N,)) == 0x5A5A5A5A).all() and (cb.download(np.uint8, (40,)) == 0xAB).all(), (what, v)
                    finally:
                        for b in (lb, cb, rb, vb):
                            b.free()
            with pytest.raises(MoonRTError, match="1 bad records"):
                rt.rasterise(rg.Polygons(bad_tables()[0][1], bad_tables()[0][2], 1), (8, 9), True)
    rings, vertices, _, _ = rc.refusal_tables()
    check(rt, rg.Polygons(rings, vertices, 1), (8, 9), True, "afterwards")


def test_too_many_crossings_are_refused_after_their_count(rt):
    # 130 edges from one end of the coordinates' range to the other, each across 2^25 columns of a window three columns wide
    pts = [(k, (-1) ** k * 2 ** 24) for k in range(130)]
    pg = rg.Polygons.from_rings([(0, pts)])
    total = 128 * 2 ** 25 + 2 * 2 ** 25                    # every edge, the closing one too, spans all 2^25 centres
    labels = np.full((2, 3), 77, np.int32)
    cover = np.zeros(1, rg.COVER_DTYPE)
    for v in VARIANTS:
        with variant(v):
            crossings, st = C.c_uint64(5), _lib.MrtxStats()
            assert raster_call(rt, rc.block(2, 3, 1), rings=pg.rings, vertices=pg.vertices, labels=labels, cover=cover, crossings=crossings,
                               st=st) == -1
            msg = rt._lib.mrtx_last_error(rt._ctx).decode()
            assert f"cross the columns {total} times" in msg, msg
            assert crossings.value == 5 and st.launches > 0 and (labels == 77).all() and (cover.view(np.uint8) == 0).all()


# ---- the render state
def test_leaves_the_render_state_alone(native_lib):
    s = named_scene("S1", 16, 16).with_size(48, 32, spp_per_launch=16)
    dem = mc.crater_dem()
    pg, shape, wrap = polygons_of(rc.geometry_cases()["across_the_seam"])
    w = rc.weights_for(shape[0])
    want = rs.raster(pg.rings, pg.vertices, pg.n_polygons, shape[0], shape[1], wrap, pg.subcell_bits, 0, 0, w)

    def go(with_raster):
        r = make(s, dem, _lib.F_COUNT_STATS)
        st1 = r.render(1)
        if with_raster:
            assert_raster_equal(run(r, pg, shape, wrap, "nonzero", "first", w, False), want[0], want[1], "between two renders")
            with variant("brute"):
                run(r, pg, shape, wrap, "evenodd", "last", None, True)
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


# ---- the tool
def test_the_rasterise_tool(native_lib, tmp_path):
    """tools/region_outlines.py --geojson into tools/rasterise.py on a small saved map: a shadow across the seam with a lit island
    inside.  The labels that come back are the kept labels."""
    import csv
    import subprocess
    import sys
    import regions_model as model
    rows, cols = 40, 96
    lit = np.ones((rows, cols, 2), np.float32)
    lit[10:30, 90:, 1] = 0.0
    lit[10:30, :9, 1] = 0.0
    lit[18:21, 2:5, 1] = 1.0
    lit[33:36, 40:50, 1] = 0.0
    lit[2, 70, 1] = 0.0                                      # one node: dropped by --min-area-km2
    np.save(tmp_path / "stats.npy", lit)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    window = [str(v) for v in (2000, 0, rows, cols, 480, 1)]
    p = subprocess.run([sys.executable, os.path.join(root, "tools", "region_outlines.py"), "--map", str(tmp_path / "stats.npy"),
                        "--channel", "1", "--below", "0.3", "--window", *window, "--min-area-km2", "20000", "--unit-m2", "100",
                        "--geojson", str(tmp_path / "o.geojson")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    labels, n = model.label(lit[:, :, 1] <= 0.3, 4, True)
    w = rg.row_weights((2000, 0, rows, cols, 480, 1), (23040, 46080), 1737400.0, 100.0)
    cat = model.catalogue(labels, n, True, w)
    keep = np.flatnonzero(cat["weight"].astype(np.float64) * 100.0 >= 20000e6)
    assert keep.tolist() == [1, 2]
    kept = np.where(np.isin(labels, keep), np.searchsorted(keep, labels), -1).astype(np.int32)
    for extra in ([], ["--rule", "nonzero", "--order", "last", "--subcell-bits", "0"]):
        p = subprocess.run([sys.executable, os.path.join(root, "tools", "rasterise.py"), "--geojson", str(tmp_path / "o.geojson"),
                            "--window", *window, "--out", str(tmp_path / "labels.npy"), "--csv", str(tmp_path / "cover.csv"),
                            "--unit-m2", "100", *extra], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stdout + p.stderr
        got = np.load(tmp_path / "labels.npy")
        assert got.dtype == np.int32 and got.shape == kept.shape and (got == kept).all()
        with open(tmp_path / "cover.csv") as f:
            table = list(csv.reader(f))
        assert table[0] == ["polygon", "nodes", "area_km2", "owned_nodes", "owned_area_km2", "row_min", "row_max", "first_node"]
        want = closed_form_cover(kept, 2, w)
        assert len(table) == 3
        for k, line in enumerate(table[1:]):
            c = want[k]
            assert line == [str(k), str(c["count"]), repr(float(c["weight"]) * 100.0 / 1e6), str(c["owned"]),
                            repr(float(c["owned_weight"]) * 100.0 / 1e6), str(c["i_min"]), str(c["i_max"]), str(c["first_at"])]
