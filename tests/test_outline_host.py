"""The region outlines without a GPU: the model against cases worked by hand, the four identities
against the regions and zonal models, the record's layout, corner coordinates and the tool's GeoJSON."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import outline_model as om
import regions_model as rm
import zonal_model as zm
from moonrtx_amd import _lib
from moonrtx_amd import regions as rg

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))


def lab(rows):
    return np.array(rows, np.int32)


def fields(rings, *names):
    return [tuple(int(r[n]) for n in names) for r in rings]


# ---- the model against cases worked by hand
def test_one_node():
    for conn in (4, 8):
        for mode in (om.ALL, om.CORNERS):
            rings, v = om.trace(lab([[0]]), conn, False, mode)
            assert fields(rings, "area", "warea", "first", "n_sides", "n_vertices", "label", "head", "wind") == [(1, 1, 0, 4, 4, 0, 0, 0)]
            assert v.tolist() == [[0, 0], [0, 1], [1, 1], [1, 0]]         # NW, NE, SE, SW: the region on the right


def test_a_three_by_three_ring():
    m = np.zeros((3, 3), np.int32)
    m[1, 1] = -1
    rings, v = om.trace(m, 4, False, om.CORNERS, row_weight=[10, 20, 40])
    assert fields(rings, "area", "warea", "n_sides", "n_vertices", "head", "wind") == [(9, 210, 12, 4, 0, 0), (-1, -20, 4, 4, 4 * 1 + 2, 0)]
    assert v[:4].tolist() == [[0, 0], [0, 3], [3, 3], [3, 0]]
    # the hole from the south side of (0, 1) on: the region stays on the right, so the hole is walked the other way round
    assert v[4:].tolist() == [[1, 2], [1, 1], [2, 1], [2, 2]]
    rings, v = om.trace(m, 4, False, om.ALL)
    assert fields(rings, "n_vertices", "first") == [(12, 0), (4, 12)] and len(v) == 16


def test_a_two_by_two_checkerboard():
    m = lab([[0, -1], [-1, 0]])
    rings, v = om.trace(m, 4, False, om.CORNERS)
    assert fields(rings, "area", "n_sides", "head") == [(1, 4, 0), (1, 4, 12)]
    rings, v = om.trace(m, 8, False, om.CORNERS)
    assert fields(rings, "area", "n_sides", "n_vertices", "head", "wind") == [(2, 8, 8, 0, 0)]
    # through the saddle at corner (1, 1), met twice
    assert v.tolist() == [[0, 0], [0, 1], [1, 1], [1, 2], [2, 2], [2, 1], [1, 1], [1, 0]]


def test_a_full_row_round_a_wrapped_window():
    rings, v = om.trace(lab([[0, 0, 0]]), 4, True, om.CORNERS)
    assert fields(rings, "area", "n_sides", "n_vertices", "head", "wind") == [(0, 3, 1, 0, 1), (3, 3, 1, 2, -1)]
    assert v.tolist() == [[0, 0], [1, 1]]                                   # no turn: the head's start corner alone
    rings, v = om.trace(lab([[0, 0, 0]]), 4, True, om.ALL)
    assert v.tolist() == [[0, 0], [0, 1], [0, 2], [1, 1], [1, 0], [1, -1]]  # x is unwrapped: it leaves 0 .. cols
    assert int(rings["area"].sum()) == 3


def test_a_region_across_the_seam_has_continuous_x():
    m = np.full((3, 6), -1, np.int32)
    m[1, 5] = m[1, 0] = m[1, 1] = 0
    rings, v = om.trace(m, 4, True, om.CORNERS)
    assert fields(rings, "area", "n_sides", "n_vertices", "head", "wind") == [(3, 8, 4, 4 * 6, 0)]
    # the head, the north side of (1, 0), follows the north side of (1, 5) straight on and is no vertex; the ring turns first
    # at x = 2 and comes back west beyond column 0, to the block's end one column past the seam
    assert v.tolist() == [[1, 2], [2, 2], [2, -1], [1, -1]]
    rings, v = om.trace(m, 4, True, om.ALL)
    assert v[0].tolist() == [1, 0] and (np.abs(np.diff(v[:, 1])) <= 1).all() and v[:, 1].min() == -1 and v[:, 1].max() == 2
    # without wrap the same table is two regions' worth of rings and every x is natural
    rings, v = om.trace(m, 4, False, om.CORNERS)
    assert len(rings) == 2 and v[:, 1].min() == 0 and v[:, 1].max() == 6


# ---- the identities
def identities(labels, n, conn, wrap, weights):
    cat = rm.catalogue(labels, n, wrap, weights)
    shp = zm.shape(labels, n, conn, wrap)
    for mode in (om.ALL, om.CORNERS):
        rings, v = om.trace(labels, conn, wrap, mode, weights)
        assert int(rings["n_vertices"].sum()) == len(v)
        if mode == om.ALL:
            assert (rings["n_vertices"] == rings["n_sides"]).all()
        for l in range(n):
            r = rings[rings["label"] == l]
            assert int(r["area"].sum()) == int(cat[l]["count"])
            assert int(r["warea"].sum()) == int(cat[l]["weight"])
            assert int(r["n_sides"].sum()) == int(shp[l]["sides_ns"]) + int(shp[l]["sides_ew"])
            outer = int(((r["wind"] == 0) & (r["area"] > 0)).sum())
            holes = int(((r["wind"] == 0) & (r["area"] < 0)).sum())
            assert outer - holes == int(shp[l]["euler"])
            assert not ((r["wind"] == 0) & (r["area"] == 0)).any()
        assert set(np.unique(rings["wind"]).tolist()) <= ({-1, 0, 1} if wrap else {0})
        assert (np.diff(rings["head"]) > 0).all()


@pytest.mark.parametrize("seed", range(6))
def test_the_identities_on_random_lattices(seed):
    rng = np.random.default_rng(100 + seed)
    for _ in range(12):
        rows, cols = int(rng.integers(1, 9)), int(rng.integers(3, 11))
        wrap, conn = bool(rng.integers(0, 2)), int(rng.choice([4, 8]))
        mask = rng.random((rows, cols)) < rng.choice([0.3, 0.59, 0.8, 1.0])
        weights = rng.integers(1, 2 ** 32, rows).astype(np.uint32) if rng.integers(0, 2) else None
        labels, n = rm.label(mask, conn, wrap)
        identities(labels, n, conn, wrap, weights)
        mine = np.where(mask, rng.integers(0, 3, (rows, cols)), -1).astype(np.int32)       # arbitrary disconnected labels
        identities(mine, 3, conn, wrap, weights)


# ---- the refusals come before any device call: on a machine without a GPU each still gives its own text
@pytest.fixture
def ctx(native_lib):
    """A context handle; without a GPU mrtx_create stops at its first HIP call but hands the context out."""
    c = C.c_void_p()
    rc = native_lib.mrtx_create(C.byref(_lib.MrtxConfig(0, 16, 16, 0, 1, 0, 0)), C.byref(c))
    assert rc in (0, -2) and c.value
    yield c
    native_lib.mrtx_destroy(c)


def test_every_refusal_comes_before_any_device_call(native_lib, ctx, monkeypatch):
    import outline_cases as oc
    monkeypatch.delenv("MOONRT_REGIONS_OUTLINE", raising=False)
    labels, rings, vertices = oc.refusal_tables()
    base = 1 << 40                      # never dereferenced: a device call with it, or without a device, would not give -1
    for text, kw in oc.refusal_cases(labels, rings, vertices, base):
        oc.assert_refused(native_lib, ctx, text, kw, rings, vertices)
    # an unknown value of the variant switch, by name; the two known ones are not refused for it
    F = dict(labels=labels, rings=rings, ring_cap=4, vertices=vertices, vertex_cap=16, o=oc.block())
    for bad in ("fast", "", "Jump"):
        monkeypatch.setenv("MOONRT_REGIONS_OUTLINE", bad)
        oc.assert_refused(native_lib, ctx, "MOONRT_REGIONS_OUTLINE must be contract or jump", F, rings, vertices)
    for good in ("contract", "jump"):
        monkeypatch.setenv("MOONRT_REGIONS_OUTLINE", good)
        oc.assert_refused(native_lib, ctx, "reserved must be 0", dict(F, o=oc.block(reserved=1)), rings, vertices)


# ---- the record
def test_ring_dtype_mirrors_the_struct():
    assert C.sizeof(_lib.MrtxRing) == 48 and rg.RING_DTYPE.itemsize == 48 and om.RING == rg.RING_DTYPE
    for name, ctype in _lib.MrtxRing._fields_:
        f = getattr(_lib.MrtxRing, name)
        assert rg.RING_DTYPE.fields[name][1] == f.offset and rg.RING_DTYPE.fields[name][0].itemsize == f.size, name
        assert (rg.RING_DTYPE.fields[name][0].kind == "i") == (ctype in (C.c_int64, C.c_int32)), name
    assert C.sizeof(_lib.MrtxOutline) == 24
    assert [n for n, _ in _lib.MrtxOutline._fields_] == ["rows", "cols", "wrap", "connectivity", "mode", "reserved"]
    assert (_lib.OUTLINE_ALL, _lib.OUTLINE_CORNERS) == (om.ALL, om.CORNERS) == (0, 1)


def ring_table():
    """Region 0 with one hole across the seam of a wrapped 6 x 8 window, region 1 a band all the way round."""
    m = np.full((6, 8), -1, np.int32)
    m[0:3, 6:8] = 0
    m[0:3, 0:2] = 0
    m[1, 7] = -1
    m[4, :] = 1
    return m


def test_outlines_accessors():
    m = ring_table()
    rings, v = om.trace(m, 4, True, om.CORNERS)
    ol = rg.Outlines(rings, v, 6, 8, True)
    assert len(ol) == 4 and [ol.role(r) for r in range(4)] == ["outer", "hole", "winding", "winding"]
    assert ol.of(0).tolist() == [0, 1] and ol.of(1).tolist() == [2, 3] and ol.of(7).tolist() == []
    assert ol.holes(2).tolist() == [1, 0] and ol.holes().tolist() == [1, 0]
    assert ol.ring(1).shape == (4, 2) and ol.ring(2).tolist() == [[4, 0]]
    assert ol.ring(0).base is not None and np.shares_memory(ol.ring(0), ol.vertices)
    with pytest.raises(ValueError):
        rg.Outlines(rings, v[:-1], 6, 8, True)


def test_corner_latlon_against_closed_forms():
    H, W = 180, 360
    v = np.array([[0, 0], [1, 1], [3, -2], [2, 9], [0, 5]], np.int32)
    rings = np.zeros(1, rg.RING_DTYPE)
    rings["n_vertices"] = 5
    ol = rg.Outlines(rings, v, 3, 8, True)
    # stride 2 from row 10, column 350: node (i, j) is the centre of texel (10 + 2 i, 350 + 2 j), at latitude 90 - (row + 1 / 2)
    # and longitude -180 + (col + 1 / 2) degrees; a corner lies one texel (half a stride) north-west of its node
    ll = ol.corner_latlon((10, 350, 3, 8, 2, 1), (H, W))
    assert ll.dtype == np.float64 and ll.shape == (5, 2)
    assert ll[:, 0].tolist() == [80.5, 78.5, 74.5, 76.5, 80.5]
    assert ll[:, 1].tolist() == [169.5, 171.5, 165.5, 187.5, 179.5]         # continuous: beyond 180 and not reduced
    # the poles: a window that starts at row 0 with stride 2 has its first corners half a stride beyond the pole, clipped
    ll = ol.corner_latlon((0, 0, 3, 8, 2, 0), (H, W))
    assert ll[0, 0] == 90.0 and ll[1, 0] == 88.5
    ol2 = rg.Outlines(rings[:1], np.array([[3, 0]] * 5, np.int32), 3, 8, False)
    assert ol2.corner_latlon((175, 0, 3, 8, 2, 0), (H, W))[0, 0] == -90.0   # 90 - (175 + 5 + 0.5) = -90.5, clipped
    # the same convention as row_weights: a row's cell reaches from corner y to corner y + 1
    ll = rg.Outlines(rings[:1], np.array([[0, 0], [1, 0], [2, 0], [3, 0], [3, 0]], np.int32), 3, 8, False).corner_latlon((40, 0, 3, 8, 4), (H, W))
    w = rg.row_weights((40, 0, 3, 8, 4), (H, W), 1000.0, 1.0)
    lat = np.radians(ll[:4, 0])
    want = np.rint(1000.0 ** 2 * (4 * 2.0 * np.pi / W) * (np.sin(lat[:-1]) - np.sin(lat[1:])))
    assert np.abs(w.astype(np.float64) - want).max() <= 1.0


# ---- the tool's GeoJSON
def test_the_tools_geojson_on_model_outlines():
    import json
    import region_outlines as tool
    m = ring_table()
    m[4, 3] = -1                                    # the band no longer goes all the way round: region 1 is an outer ring now
    rings, v = om.trace(m, 4, True, om.CORNERS)
    ol = rg.Outlines(rings, v, 6, 8, True)
    assert [ol.role(r) for r in range(len(ol))] == ["outer", "hole", "outer"]
    ll = ol.corner_latlon((20, 100, 6, 8, 2, 1), (180, 360))
    props = {"area_km2": np.array([1.5, 2.5]), "nodes": np.array([11, 7]), "holes": ol.holes(2), "perimeter_km": np.array([3.0, 4.0])}
    fc = json.loads(json.dumps(tool.feature_collection(ol, ll, props)))
    assert fc["type"] == "FeatureCollection" and len(fc["features"]) == 2
    for f, label in zip(fc["features"], (0, 1)):
        assert f["type"] == "Feature" and f["geometry"]["type"] == "Polygon"
        assert f["properties"] == {"region": label, "area_km2": [1.5, 2.5][label], "nodes": [11, 7][label], "holes": [1, 0][label],
                                   "perimeter_km": [3.0, 4.0][label]}
        got = f["geometry"]["coordinates"]
        assert len(got) == 1 + [1, 0][label]
        for k, ring in enumerate(got):
            assert ring[0] == ring[-1] and len(ring) >= 5                   # closed
            s = tool.shoelace(ring)
            assert s > 0 if k == 0 else s < 0                               # RFC 7946: outer counter-clockwise, holes clockwise
            # the same corners as the ring's vertex slice, as (lon, lat), from the head on
            r = ol.of(label)[k]
            a = int(ol.rings[r]["first"])
            want = {(float(ll[a + q, 1]), float(ll[a + q, 0])) for q in range(int(ol.rings[r]["n_vertices"]))}
            assert {tuple(p) for p in ring} == want and tuple(ring[0]) == (float(ll[a, 1]), float(ll[a, 0]))
    # the enclosed area in corner units is the ring's area
    y0 = [[p[0], p[1]] for p in fc["features"][1]["geometry"]["coordinates"][0]]
    assert abs(tool.shoelace(y0) / 2.0 - 7 * 2.0 * 2.0) < 1e-9              # 7 nodes of 2 x 2 degrees
    # a winding region becomes a MultiLineString
    rings, v = om.trace(ring_table(), 4, True, om.CORNERS)
    ol = rg.Outlines(rings, v, 6, 8, True)
    fc = tool.feature_collection(ol, ol.corner_latlon((20, 100, 6, 8, 2, 1), (180, 360)), {"holes": ol.holes(2)})
    f = fc["features"][1]
    assert f["geometry"]["type"] == "MultiLineString" and f["properties"] == {"region": 1, "holes": 0, "winds": True}
    assert len(f["geometry"]["coordinates"]) == 2
    # a caller's label with two outer rings is refused
    two = lab([[0, -1, 0]])
    rings, v = om.trace(two, 4, False, om.CORNERS)
    ol = rg.Outlines(rings, v, 1, 3, False)
    with pytest.raises(ValueError, match="label 0 has 2 outer rings"):
        tool.feature_collection(ol, ol.corner_latlon((20, 100, 1, 3), (180, 360)), {})
    rows = list(tool.vertex_rows(ol, ol.corner_latlon((20, 100, 1, 3), (180, 360))))
    assert len(rows) == 8 and rows[0][:5] == [0, 0, "outer", 0, 0] and rows[4][:5] == [1, 0, "outer", 0, 2]
