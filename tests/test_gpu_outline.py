"""The region outlines on the GPU: mrtx_regions_outline / MoonRT.region_outlines against
tests/outline_model.py.  Every field of every ring record and every vertex is compared with ==."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import model_cases as mc
import outline_cases as oc
import outline_model as om
import regions_cases as rc
from common import assert_bit_equal
from moonrtx_amd import _lib
from moonrtx_amd import regions as rg
from moonrtx_amd.renderer import DeviceBuffer, MoonRT, MoonRTError
from moonrtx_amd.scene import named_scene
from test_gpu_illumination import make
from test_gpu_zonal import label_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt(native_lib):
    """One context for the module, without a DEM, a light or a Moon frame: the stage needs none of them."""
    r = MoonRT(16, 16)
    yield r
    r.close()


def weights_for(rows):
    """distinct per row and near 2^32, so that warea needs 64 bits"""
    return (2 ** 32 - 1 - 3 * np.arange(rows)).astype(np.uint32)


def assert_outlines_equal(got, rings, vertices, what):
    assert got.rings.shape == rings.shape, (what, got.rings.shape, rings.shape)
    for name in rg.RING_DTYPE.names:
        bad = np.flatnonzero(got.rings[name] != rings[name])
        assert bad.size == 0, (what, name, int(bad[0]), got.rings[bad[0]], rings[bad[0]])
    assert got.vertices.shape == vertices.shape, (what, got.vertices.shape, vertices.shape)
    bad = np.flatnonzero((got.vertices != vertices).any(axis=1))
    assert bad.size == 0, (what, "vertex", int(bad[0]), got.vertices[bad[0]].tolist(), vertices[bad[0]].tolist())


def run(rt, labels, n, conn, wrap, corners, weights, device, stats=None):
    if not device:
        return rt.region_outlines(labels, n, conn, wrap, corners, weights, stats=stats)
    buf = DeviceBuffer(max(labels.size * 4, 4))
    try:
        buf.upload(np.ascontiguousarray(labels, np.int32))
        return rt.region_outlines(buf, n, conn, wrap, corners, weights, shape=labels.shape, stats=stats)
    finally:
        buf.free()


VARIANTS = ("contract", "jump")


@contextlib.contextmanager
def variant(name):
    """MOONRT_REGIONS_OUTLINE = name (None: unset) for the calls inside."""
    old = os.environ.get("MOONRT_REGIONS_OUTLINE")
    try:
        if name is None:
            os.environ.pop("MOONRT_REGIONS_OUTLINE", None)
        else:
            os.environ["MOONRT_REGIONS_OUTLINE"] = name
        yield
    finally:
        if old is None:
            os.environ.pop("MOONRT_REGIONS_OUTLINE", None)
        else:
            os.environ["MOONRT_REGIONS_OUTLINE"] = old


@pytest.fixture(params=VARIANTS)
def each_variant(request, monkeypatch):
    """The test runs once under each value of the switch."""
    monkeypatch.setenv("MOONRT_REGIONS_OUTLINE", request.param)
    return request.param


def check(rt, labels, n, wrap, what):
    """Both variants, both connectivities and both modes, from a host and from a device table, with and without row weights:
    every one against the model, so the two variants give the same bytes."""
    labels = np.ascontiguousarray(labels, np.int32)
    w = weights_for(labels.shape[0])
    for conn in (4, 8):
        for corners in (True, False):
            rings, vertices = om.trace(labels, conn, wrap, om.CORNERS if corners else om.ALL, w)
            plain = rings.copy()
            plain["warea"] = plain["area"]
            for v in VARIANTS:
                with variant(v):
                    for device in (False, True):
                        for weights, want in ((w, rings), (None, plain)):
                            got = run(rt, labels, n, conn, wrap, corners, weights, device)
                            assert_outlines_equal(got, want, vertices, (what, v, conn, corners, device, weights is not None))


# ---- the built cases of the regions stage
BUILT = [c["name"] for c in rc.CASES]


@pytest.mark.parametrize("name", BUILT)
def test_built_cases_equal_the_model(rt, name):
    case = rc.BY_NAME[name]
    labels = np.ascontiguousarray(rc.answer(case, 4)[0], np.int32)
    n4 = rc.answer(case, 4)[1]
    # the 4-connected labels at both connectivities (at 8 the rings of diagonal neighbours of one label join through saddles;
    # different labels never do), and the 8-connected labels too where they differ
    check(rt, labels, n4, case["wrap"], name)
    labels8, n8 = rc.answer(case, 8)
    if n8 != n4:
        check(rt, np.ascontiguousarray(labels8, np.int32), n8, case["wrap"], name + "/8")


# ---- own small cases
def own_cases():
    out = {}
    out["1x1"] = (np.zeros((1, 1), np.int32), 1, False)
    out["1x3_wrapped_full"] = (np.zeros((1, 3), np.int32), 1, True)
    out["2x2_checkerboard"] = (np.array([[0, -1], [-1, 0]], np.int32), 1, False)
    m = np.full((6, 7), -1, np.int32)
    m[1, 6] = m[2, 0] = 0                                   # a diagonal pair across the seam, and one of the other diagonal
    m[4, 0] = m[5, 6] = 0
    out["saddle_on_the_seam"] = (m, 1, True)
    m = np.full((40, 130), -1, np.int32)
    m[15, 63] = m[16, 64] = 0                               # the corner shared by four 16 x 64 tiles
    m[15, 64] = m[16, 63] = 1
    out["saddle_on_a_tile_corner"] = (m, 2, False)
    m = np.full((40, 200), -1, np.int32)
    m[37:40, 190:200] = 0
    m[38, 195] = -1
    out["head_in_the_last_tile"] = (m, 1, False)
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
    out["all_outside"] = (np.full((33, 65), -1, np.int32), 0, False)
    out["all_outside_n3"] = (np.full((33, 65), -1, np.int32), 3, True)
    out["full"] = (np.zeros((33, 65), np.int32), 1, False)
    out["full_wrapped"] = (np.zeros((33, 65), np.int32), 1, True)
    out["2100_in_a_row"] = (np.zeros((1, 2100), np.int32), 1, True)      # more sides than one chunk of the scans
    for k in ("16x1025", "rings", "seam_ring_hole", "callers_own", "callers_own_wrapped", "two_checkerboards", "3x3_wrapped",
              "17x65_wrapped"):
        out[k] = label_cases()[k]
    return out


OWN = ["1x1", "1x3_wrapped_full", "2x2_checkerboard", "saddle_on_the_seam", "saddle_on_a_tile_corner", "head_in_the_last_tile",
       "band_round_the_seam", "band_with_a_gap", "band_with_holes", "all_outside", "all_outside_n3", "full", "full_wrapped",
       "2100_in_a_row", "16x1025", "rings", "seam_ring_hole", "callers_own", "callers_own_wrapped", "two_checkerboards",
       "3x3_wrapped", "17x65_wrapped"]


@pytest.mark.parametrize("name", OWN)
def test_own_cases_equal_the_model(rt, name):
    labels, n, wrap = own_cases()[name]
    check(rt, labels, n, wrap, name)


def test_what_the_own_cases_hold(rt):
    """The cases are what their names say, by the model."""
    cases = own_cases()
    r, _ = om.trace(cases["rings"][0], 4, False)
    holes = {l: int(((r["label"] == l) & (r["area"] < 0)).sum()) for l in range(3)}
    assert holes == {0: 1, 1: 2, 2: 5}
    r, _ = om.trace(cases["saddle_on_the_seam"][0], 8, True)
    assert r["n_sides"].tolist() == [8, 8] and len(om.trace(cases["saddle_on_the_seam"][0], 4, True)[0]) == 4
    r, _ = om.trace(cases["band_round_the_seam"][0], 4, True)
    assert r["wind"].tolist() == [1, -1]
    r, _ = om.trace(cases["band_with_a_gap"][0], 4, True)
    assert r["wind"].tolist() == [0] and r["area"].tolist() == [3 * 69]
    r, _ = om.trace(cases["band_with_holes"][0], 4, True)
    assert sorted(r["wind"].tolist()) == [-1, 0, 0, 1]
    ol = run(rt, cases["band_with_holes"][0], 1, 4, True, True, None, False)
    assert ol.holes(1).tolist() == [2] and [ol.role(k) for k in ol.of(0)] == ["winding", "winding", "hole", "hole"]
    r, _ = om.trace(cases["head_in_the_last_tile"][0], 4, False)
    assert r["head"].min() >= 4 * (37 * 200 + 190)


# ---- the identities, against the other stages' device output
@pytest.mark.parametrize("name,conn", [("random_0.59_wrapped", 4), ("random_0.59_wrapped", 8), ("seam_ring", 4), ("checker_33x65_wrapped", 8),
                                       ("spiral", 4)])
def test_identities_on_the_device(rt, each_variant, name, conn):
    case = rc.BY_NAME[name]
    mask = rc.case_mask(case)
    w = weights_for(mask.shape[0])
    m = rt.regions(mask=mask, connectivity=conn, wrap=case["wrap"], row_weights=w)
    shp = m.shapes(rt, conn)
    zon = m.zonal(rt, np.ones(mask.shape, np.float32), row_weights=w)[:, 0]
    ol = m.outlines(rt, conn, True, w)
    lab = ol.rings["label"].astype(np.int64)
    assert lab.min() >= 0 and lab.max() < m.n

    def per_label(values):
        out = np.zeros(m.n, object)
        for l, v in zip(lab.tolist(), values.tolist()):
            out[l] += v
        return out
    plain = ol.rings["wind"] == 0
    assert per_label(ol.rings["area"]).tolist() == m.table["count"].tolist() == zon["count"].tolist()
    assert per_label(ol.rings["warea"]).tolist() == m.table["weight"].tolist() == zon["wcount"].tolist()
    assert per_label(ol.rings["n_sides"]).tolist() == (shp["sides_ns"].astype(np.int64) + shp["sides_ew"]).tolist()
    outer = per_label((plain & (ol.rings["area"] > 0)).astype(np.int64))
    holes = per_label((plain & (ol.rings["area"] < 0)).astype(np.int64))
    assert (outer - holes).tolist() == shp["euler"].tolist()
    assert holes.tolist() == ol.holes(m.n).tolist()
    # a connected region has one outer ring, or none when it winds, and its first ring starts at its root
    winds = per_label((~plain).astype(np.int64))
    assert all(o == (0 if wd else 1) for o, wd in zip(outer.tolist(), winds.tolist()))
    first = {}
    for r in range(len(ol)):
        first.setdefault(int(lab[r]), int(ol.rings["head"][r]))
    assert [first[l] for l in range(m.n)] == (4 * (m.table["root_i"].astype(np.int64) * mask.shape[1] + m.table["root_j"])).tolist()


# ---- the cap protocol
def outline_call(rt, o, labels=None, **kw):
    return oc.outline_call(rt._lib, rt._ctx, o, labels, **kw)


block = oc.block


def test_the_cap_protocol(rt, each_variant):
    labels, n, wrap = label_cases()["rings"]
    want_r, want_v = om.trace(labels, 4, wrap, om.CORNERS)
    R, V = len(want_r), len(want_v)
    o = block(*labels.shape, int(wrap))
    nr, nv = C.c_uint64(77), C.c_uint64(77)
    assert outline_call(rt, o, labels, n=n, counts=(nr, nv)) == 0                  # the count call
    assert (nr.value, nv.value) == (R, V)
    for device in (False, True):
        rings, vertices = np.zeros(R + 2, rg.RING_DTYPE), np.zeros((V + 2, 2), np.int32)
        rb, vb = DeviceBuffer(48 * (R + 2)), DeviceBuffer(8 * (V + 2))
        try:
            def call(ring_cap, vertex_cap):
                nr.value = nv.value = 77
                rings.view(np.uint8)[:] = 0xAB
                vertices.view(np.uint8)[:] = 0xAB
                rb.upload(rings)
                vb.upload(vertices)
                if device:
                    rc_ = outline_call(rt, o, labels, n=n, dev_rings=rb.ptr, ring_cap=ring_cap, dev_vertices=vb.ptr, vertex_cap=vertex_cap,
                                       counts=(nr, nv))
                    return rc_, rb.download(rg.RING_DTYPE, (R + 2,)), vb.download(np.int32, (V + 2, 2))
                rc_ = outline_call(rt, o, labels, n=n, rings=rings, ring_cap=ring_cap, vertices=vertices, vertex_cap=vertex_cap,
                                   counts=(nr, nv))
                return rc_, rings.copy(), vertices.copy()
            for caps in ((R, V), (R + 2, V + 2)):                                   # exact caps fill, and so do larger ones
                rc_, gr, gv = call(*caps)
                assert rc_ == 0 and (nr.value, nv.value) == (R, V)
                assert_outlines_equal(rg.Outlines(gr[:R], gv[:V], *labels.shape, wrap), want_r, want_v, ("caps", caps, device))
                assert (gr[R:].view(np.uint8) == 0xAB).all() and (gv[V:].view(np.uint8) == 0xAB).all()
            for caps in ((R - 1, V), (R, V - 1), (0, 0)):                           # a cap one short
                rc_, gr, gv = call(*caps)
                assert rc_ == -1 and (nr.value, nv.value) == (R, V), caps
                msg = rt._lib.mrtx_last_error(rt._ctx).decode()
                assert f"{R} rings and {V} vertices are needed" in msg, msg
                assert (gr.view(np.uint8) == 0xAB).all() and (gv.view(np.uint8) == 0xAB).all(), caps
        finally:
            rb.free()
            vb.free()


def test_every_refusal(rt):
    """Each text, the counts and the statistics as they were, no table touched, on the host or on the device (that no refusal
    makes a device call is shown without a device, in tests/test_outline_host.py)."""
    labels, rings, vertices = oc.refusal_tables()
    dev = DeviceBuffer(8192)
    fill = np.full(8192, 0xAB, np.uint8)
    try:
        dev.upload(fill)
        for text, kw in oc.refusal_cases(labels, rings, vertices, dev.ptr):
            with variant(None):
                oc.assert_refused(rt._lib, rt._ctx, text, kw, rings, vertices)
        F = dict(labels=labels, rings=rings, ring_cap=4, vertices=vertices, vertex_cap=16, o=block())
        D = dict(dev_labels=dev.ptr, dev_rings=dev.ptr + 512, ring_cap=4, dev_vertices=dev.ptr + 1024, vertex_cap=16, o=block())
        for kw in (F, D):
            with variant("fast"):
                oc.assert_refused(rt._lib, rt._ctx, "MOONRT_REGIONS_OUTLINE must be contract or jump \\(got fast\\)", kw, rings, vertices)
        assert (dev.download(np.uint8, (8192,)) == 0xAB).all()
        # the context still works
        lab, n, wrap = label_cases()["17x65_wrapped"]
        check(rt, lab, n, wrap, "after the refusals")
    finally:
        dev.free()


def test_a_bad_label_table_is_refused_after_the_launch(rt, each_variant):
    labels, n, wrap = label_cases()["random_0.59_wrapped"]
    o = block(*labels.shape, int(wrap))
    rings, vertices = np.zeros(labels.size, rg.RING_DTYPE), np.zeros((4 * labels.size, 2), np.int32)
    for bad in (n, n + 1000, 2 ** 31 - 1, -2, -2 ** 31):
        mine = labels.copy()
        mine[17, 23] = bad
        nr, nv = C.c_uint64(5), C.c_uint64(5)
        assert outline_call(rt, o, mine, n=n, counts=(nr, nv)) == -1, bad
        assert "1 entries outside -1" in rt._lib.mrtx_last_error(rt._ctx).decode()
        assert outline_call(rt, o, mine, n=n, rings=rings, ring_cap=len(rings), vertices=vertices, vertex_cap=len(vertices),
                            counts=(nr, nv)) == -1, bad
        assert "1 entries outside -1" in rt._lib.mrtx_last_error(rt._ctx).decode()
        assert (nr.value, nv.value) == (5, 5) and (rings.view(np.uint8) == 0).all() and (vertices == 0).all()
        with pytest.raises(MoonRTError, match="entries outside -1"):
            run(rt, mine, n, 8, wrap, True, None, True)
    # no regions: the table is checked, nothing is written
    none = np.full((5, 5), -1, np.int32)
    got = rt.region_outlines(none, 0)
    assert len(got) == 0 and got.vertices.shape == (0, 2)
    one = none.copy()
    one[2, 2] = 0
    with pytest.raises(MoonRTError, match="entries outside -1"):
        rt.region_outlines(one, 0)
    check(rt, labels, n, wrap, "afterwards")


def test_launches_depend_on_the_number_of_sides_alone(rt, each_variant):
    mask = rc.case_mask(rc.BY_NAME["random_0.59"])
    labels = np.where(mask, 0, -1).astype(np.int32)
    mirror = np.ascontiguousarray(labels[:, ::-1])
    blocks = np.where(mask, (np.arange(mask.shape[1]) // 7 % 3)[None, :], -1).astype(np.int32)
    for corners in (True, False):
        for weights in (None, weights_for(mask.shape[0])):
            seen = []
            for lab in (labels, mirror):
                st = {}
                ol = rt.region_outlines(lab, 3, 4, False, corners, weights, stats=st)
                assert st["launches"] > 0 and st["kernel_ms"] > 0.0
                seen.append((st["launches"], int(ol.rings["n_sides"].astype(np.int64).sum())))
            assert seen[0] == seen[1], seen
    # other labels on the same set have other sides; the count call launches less than the fill call
    o = block(*labels.shape)
    s1, s2 = _lib.MrtxStats(), _lib.MrtxStats()
    assert outline_call(rt, o, blocks, n=3, st=s1) == 0
    rings, vertices = np.zeros(labels.size, rg.RING_DTYPE), np.zeros((4 * labels.size, 2), np.int32)
    assert outline_call(rt, o, blocks, n=3, rings=rings, ring_cap=len(rings), vertices=vertices, vertex_cap=len(vertices), st=s2) == 0
    assert 0 < s1.launches < s2.launches


def test_leaves_the_render_state_alone(native_lib):
    s = named_scene("S1", 16, 16).with_size(48, 32, spp_per_launch=16)
    dem = mc.crater_dem()
    labels, n, wrap = label_cases()["17x65_wrapped"]
    want = om.trace(labels, 8, wrap, om.CORNERS, weights_for(17))

    def go(with_outlines):
        r = make(s, dem, _lib.F_COUNT_STATS)
        st1 = r.render(1)
        if with_outlines:
            assert_outlines_equal(run(r, labels, n, 8, wrap, True, weights_for(17), False), *want, "between two renders")
            run(r, labels, n, 4, wrap, False, None, True)
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


def test_the_outline_tool(native_lib, tmp_path):
    """tools/region_outlines.py end to end on a small saved map: a shadow across the seam with a lit island inside."""
    import csv
    import json
    import os
    import subprocess
    import sys
    import regions_model as model
    import zonal_model as zm
    rows, cols = 40, 96
    lit = np.ones((rows, cols, 2), np.float32)
    lit[10:30, 90:, 1] = 0.0
    lit[10:30, :9, 1] = 0.0
    lit[18:21, 2:5, 1] = 1.0
    lit[33:36, 40:50, 1] = 0.0
    lit[2, 70, 1] = 0.0                                      # one node: dropped by --min-area-km2
    np.save(tmp_path / "stats.npy", lit)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    window = (2000, 0, rows, cols, 480, 1)
    p = subprocess.run([sys.executable, os.path.join(root, "tools", "region_outlines.py"), "--map", str(tmp_path / "stats.npy"),
                        "--channel", "1", "--below", "0.3", "--window", *[str(v) for v in window], "--min-area-km2", "20000",
                        "--unit-m2", "100", "--side-unit-m", "0.5", "--geojson", str(tmp_path / "o.geojson"), "--csv",
                        str(tmp_path / "o.csv")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    labels, n = model.label(lit[:, :, 1] <= 0.3, 4, True)
    w = rg.row_weights(window, (23040, 46080), 1737400.0, 100.0)
    cat = model.catalogue(labels, n, True, w)
    keep = np.flatnonzero(cat["weight"].astype(np.float64) * 100.0 >= 20000e6)
    assert keep.tolist() == [1, 2]
    kept = np.where(np.isin(labels, keep), np.searchsorted(keep, labels), -1).astype(np.int32)
    rings, vertices = om.trace(kept, 4, True, om.CORNERS, w)
    ol = rg.Outlines(rings, vertices, rows, cols, True)
    ll = ol.corner_latlon(window, (23040, 46080))
    ew, ns = rg.side_weights(window, (23040, 46080), 1737400.0, 0.5)
    sh = zm.shape(kept, 2, 4, True, ew, ns)
    with open(tmp_path / "o.geojson") as f:
        fc = json.load(f)
    assert fc["type"] == "FeatureCollection" and [f["properties"]["region"] for f in fc["features"]] == [0, 1]
    for f in fc["features"]:
        k = f["properties"]["region"]
        assert f["properties"] == {"region": k, "area_km2": float(cat["weight"][keep[k]]) * 100.0 / 1e6, "nodes": int(cat["count"][keep[k]]),
                                   "holes": [1, 0][k], "perimeter_km": float(sh["perimeter"][k]) * (0.5 / 1e3)}
        assert f["geometry"]["type"] == "Polygon" and len(f["geometry"]["coordinates"]) == [2, 1][k]
        for q, (r, ring) in enumerate(zip(ol.of(k), f["geometry"]["coordinates"])):
            a, m = int(rings[r]["first"]), int(rings[r]["n_vertices"])
            want = [[float(ll[a + v, 1]), float(ll[a + v, 0])] for v in range(m)]
            assert ring == [want[0]] + want[:0:-1] + [want[0]]
            s2 = sum(u[0] * v[1] - v[0] * u[1] for u, v in zip(ring[:-1], ring[1:]))
            assert s2 > 0 if q == 0 else s2 < 0
    # the shadow across the seam is one ring with continuous longitude
    lon = [pt[0] for pt in fc["features"][0]["geometry"]["coordinates"][0]]
    assert max(lon) - min(lon) < 90.0 and min(lon) < -180.0
    with open(tmp_path / "o.csv") as f:
        got = list(csv.reader(f))
    assert got[0] == ["ring", "region", "role", "y", "x", "lat", "lon"] and len(got) == 1 + len(vertices)
    at = 1
    for r in range(len(ol)):
        for v in ol.ring(r).tolist():
            line = got[at]
            assert line[:5] == [str(r), str(int(rings[r]["label"])), ol.role(r), str(v[0]), str(v[1])]
            assert (float(line[5]), float(line[6])) == (float(ll[at - 1, 0]), float(ll[at - 1, 1]))
            at += 1
