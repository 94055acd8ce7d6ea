"""The polygon rasterisation without a GPU: the model against cases worked by hand, the model's round
trip through the outline model, the records' layouts, Polygons and its coordinates, the refusals and the tool's GeoJSON."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

import outline_model as om
import raster_cases as rc
import raster_model as rs
import regions_model as rm
from moonrtx_amd import _lib
from moonrtx_amd import regions as rg

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))


def model(case, rule=rs.NONZERO, order=rs.FIRST, weights=None):
    rings, n, rows, cols, wrap, s = case
    recs, verts = rs.polygons(rings)
    return rs.raster(recs, verts, n, rows, cols, wrap, s, rule, order, weights)


# ---- the model against cases worked by hand
def test_a_unit_square():
    for s in (0, 3, 8):
        u = 2 ** s
        labels, cover, n = model(([(0, [(u, u), (u, 3 * u), (2 * u, 3 * u), (2 * u, u)])], 1, 4, 5, False, s))
        assert labels.tolist() == [[-1] * 5, [-1, 0, 0, -1, -1], [-1] * 5, [-1] * 5]
        assert cover[0].tolist() == (2, 2, 2, 2, 1, 1, 6, 0) and n == 4


def test_a_centre_on_an_edge_counts_as_below_it_and_spans_are_half_open():
    # a square from the centre of node (0, 0) to the centre of node (2, 2): the rows and columns of the first centres are in, those
    # of the last ones are out
    labels, _, _ = model(([(0, [(1, 1), (1, 5), (5, 5), (5, 1)])], 1, 4, 4, False, 1))
    assert labels.tolist() == [[0, 0, -1, -1], [0, 0, -1, -1], [-1] * 4, [-1] * 4]


def test_two_triangles_cover_every_node_once():
    case = rc.geometry_cases()["two_triangles"]
    for rule in (rs.NONZERO, rs.EVENODD):
        first, cover, _ = model(case, rule, rs.FIRST)
        last, _, _ = model(case, rule, rs.LAST)
        assert (first == last).all() and (first >= 0).all()
        assert int(cover["count"].sum()) == 64 and cover["owned"].tolist() == cover["count"].tolist()
    # the diagonal's nodes have their centres on the shared edge: they are the lower-left triangle's
    assert [int(first[k, k]) for k in range(8)] == [1] * 8


def test_the_pentagram_tells_the_rules_apart():
    case = rc.geometry_cases()["pentagram"]
    nz, _, _ = model(case, rs.NONZERO)
    eo, _, _ = model(case, rs.EVENODD)
    assert nz[10, 10] == 0 and eo[10, 10] == -1 and (nz >= 0).sum() > (eo >= 0).sum() > 0
    assert ((eo >= 0) <= (nz >= 0)).all()


def test_rings_without_area_and_polygons_without_rings():
    labels, cover, _ = model(rc.geometry_cases()["zero_area_and_one_vertex"])
    assert set(np.unique(labels).tolist()) == {-1, 3}
    for p in (0, 1, 2):
        assert cover[p].tolist() == (0, 0, 0, 0, -1, -1, -1, 0)
    assert int(cover[3]["count"]) == 64 and int(cover[3]["first_at"]) == 2 * 12 + 2


def test_overlapping_polygons_and_the_two_orders():
    case = rc.geometry_cases()["overlapping"]
    w = rc.weights_for(case[2])
    first, cf, _ = model(case, rs.NONZERO, rs.FIRST, w)
    last, cl, _ = model(case, rs.NONZERO, rs.LAST, w)
    assert cf["count"].tolist() == cl["count"].tolist() and cf["weight"].tolist() == cl["weight"].tolist()
    assert first[6, 6] == 0 and last[6, 6] == 2 and (cf["owned"] <= cf["count"]).all()
    assert int(cf["owned"].sum()) == int((first >= 0).sum()) == int(cl["owned"].sum())
    assert cf["owned"][0] == cf["count"][0] and cl["owned"][3] == cl["count"][3]
    assert int(cf["weight"][0]) == sum(int(w[i]) * 8 for i in range(1, 9))
    # polygon 1's second ring runs the other way inside its first: a hole under both rules
    assert first[9, 9] == 1 and first[6, 7] == 0 and int(cf["count"][1]) == 8 * 10 - 3 * 2


def test_an_edge_longer_than_the_window_hits_a_column_more_than_once():
    case = ([(0, [(0, 0), (0, 25), (2, 25), (2, 0)])], 1, 3, 10, True, 0)
    labels, cover, n = model(case)
    assert n == 50 and labels[:2, :5].tolist() == [[0] * 5] * 2          # winding 3 on columns 0 .. 4, 2 on the others
    assert (labels[:2] == 0).all() and (labels[2] == -1).all()
    eo, _, _ = model(case, rs.EVENODD)
    assert (eo[:2, :5] == 0).all() and (eo[:2, 5:] == -1).all()


# ---- the round trip: rasterising the outlines of a label table gives the table back
def round_trip(labels, n, wrap):
    labels = np.asarray(labels, np.int32)
    rows, cols = labels.shape
    for conn in (4, 8):
        for mode in (om.ALL, om.CORNERS):
            r, v = om.trace(labels, conn, wrap, mode)
            recs = rs.rings_of_outlines(r)
            hits = rs.crossings(recs, v, rows, cols, wrap, 0)
            for rule in (rs.NONZERO, rs.EVENODD):
                got, cover, _ = rs.raster(recs, v, n, rows, cols, wrap, 0, rule, hits=hits)
                assert (got == labels).all(), (conn, mode, rule)
                assert cover["count"].tolist() == cover["owned"].tolist() == np.bincount(labels[labels >= 0], minlength=n).tolist()


@pytest.mark.parametrize("seed", range(6))
def test_the_round_trip_on_random_tables(seed):
    rng = np.random.default_rng(300 + seed)
    for _ in range(10):
        rows, cols = int(rng.integers(1, 9)), int(rng.integers(3, 11))
        wrap, conn = bool(rng.integers(0, 2)), int(rng.choice([4, 8]))
        mask = rng.random((rows, cols)) < rng.choice([0.3, 0.59, 0.8, 1.0])
        labels, n = rm.label(mask, conn, wrap)
        round_trip(labels, n, wrap)
        mine = np.where(mask, rng.integers(0, 3, (rows, cols)), -1).astype(np.int32)       # arbitrary disconnected labels
        round_trip(mine, 3, wrap)


def seam_cases():
    out = {}
    out["1x3_wrapped_full"] = (np.zeros((1, 3), np.int32), 1, True)
    m = np.full((6, 7), -1, np.int32)
    m[1, 6] = m[2, 0] = 0
    m[4, 0] = m[5, 6] = 0
    out["saddle_on_the_seam"] = (m, 1, True)
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
    return out


@pytest.mark.parametrize("name", sorted(seam_cases()))
def test_the_round_trip_on_the_seam(name):
    round_trip(*seam_cases()[name])


# ---- the records
def test_dtypes_mirror_the_structs():
    for struct, dtype, mine, size in ((_lib.MrtxRasterRing, rg.RASTER_RING_DTYPE, rs.RING, 24), (_lib.MrtxPolygonCover, rg.COVER_DTYPE, rs.COVER, 40)):
        assert C.sizeof(struct) == size == dtype.itemsize and mine == dtype
        for name, ctype in struct._fields_:
            f = getattr(struct, name)
            assert dtype.fields[name][1] == f.offset and dtype.fields[name][0].itemsize == f.size, name
            assert (dtype.fields[name][0].kind == "i") == (ctype in (C.c_int64, C.c_int32)), name
    assert C.sizeof(_lib.MrtxRaster) == 28
    assert [n for n, _ in _lib.MrtxRaster._fields_] == ["rows", "cols", "wrap", "subcell_bits", "rule", "order", "reserved"]
    assert (_lib.RASTER_NONZERO, _lib.RASTER_EVENODD) == (rs.NONZERO, rs.EVENODD) == (0, 1)
    assert (_lib.RASTER_FIRST, _lib.RASTER_LAST) == (rs.FIRST, rs.LAST) == (0, 1)
    assert "mrtx_rasterise" in _lib.SIGNATURES and len(_lib.SIGNATURES["mrtx_rasterise"][1]) == 16


# ---- Polygons
def test_polygons_and_outlines_polygons():
    m = np.full((6, 8), -1, np.int32)
    m[0:3, 6:8] = 0
    m[0:3, 0:2] = 0
    m[1, 7] = -1
    m[4, :] = 2
    rings, v = om.trace(m, 4, True, om.CORNERS)
    ol = rg.Outlines(rings, v, 6, 8, True)
    pg = ol.polygons()
    assert isinstance(pg, rg.Polygons) and len(pg) == 4 and pg.n_polygons == 3 and pg.subcell_bits == 0
    assert ol.polygons(7).n_polygons == 7
    assert pg.rings.dtype == rg.RASTER_RING_DTYPE and (pg.vertices == v).all()
    for a, b in (("first", "first"), ("n_vertices", "n_vertices"), ("polygon", "label"), ("wind", "wind")):
        assert pg.rings[a].tolist() == rings[b].tolist()
    assert (pg.rings["reserved"] == 0).all() and pg.rings["wind"].tolist() == [0, 0, 1, -1]
    assert pg.ring(1).tolist() == ol.ring(1).tolist() and np.shares_memory(pg.ring(0), pg.vertices)
    got, _, _ = rs.raster(pg.rings, pg.vertices, 3, 6, 8, True, 0)
    assert (got == m).all()
    with pytest.raises(ValueError, match="do not add up"):
        rg.Polygons(pg.rings, pg.vertices[:-1], 3)
    with pytest.raises(ValueError, match="subcell_bits"):
        rg.Polygons(pg.rings, pg.vertices, 3, 9)
    empty = rg.Outlines(np.zeros(0, rg.RING_DTYPE), np.zeros((0, 2), np.int32), 6, 8).polygons()
    assert len(empty) == 0 and empty.n_polygons == 0
    mine = rg.Polygons.from_rings([(1, [(0, 0), (0, 4), (4, 4)]), (0, [(1, 1)], -1)], subcell_bits=2)
    assert mine.n_polygons == 2 and mine.rings.tolist() == [(0, 3, 1, 0, 0), (3, 1, 0, -1, 0)] and mine.vertices.tolist() == [[0, 0], [0, 4], [4, 4], [1, 1]]


def test_from_latlon_against_closed_forms():
    H, W = 180, 360
    # stride 2 from row 10, column 350 (test_outline_host's window): corner (y, x) lies at latitude 90 - (10 + 2 y - 1 + 1/2) and
    # longitude -180 + (350 + 2 x - 1 + 1/2) degrees
    window = (10, 350, 3, 8, 2, 1)
    ring = [(80.5, 169.5), (78.5, 171.5), (74.5, 165.5), (76.5, 187.5), (80.5, 179.5)]
    pg = rg.Polygons.from_latlon(window, (H, W), [[ring]], 0)
    assert pg.vertices.tolist() == [[0, 0], [1, 1], [3, -2], [2, 9], [0, 5]] and pg.rings.tolist() == [(0, 5, 0, 0, 0)]
    pg4 = rg.Polygons.from_latlon(window, (H, W), [[ring]])
    assert pg4.subcell_bits == 4 and (pg4.vertices == 16 * pg.vertices).all()
    # a quarter of a degree is an eighth of a cell: floor(v 2^s + 1/2) rounds it up at s = 2 and keeps it at s = 3
    assert rg.Polygons.from_latlon(window, (H, W), [[[(80.25, 169.75)]]], 3).vertices.tolist() == [[1, 1]]
    assert rg.Polygons.from_latlon(window, (H, W), [[[(80.25, 169.75)]]], 2).vertices.tolist() == [[1, 1]]
    assert rg.Polygons.from_latlon(window, (H, W), [[[(80.75, 169.25)]]], 2).vertices.tolist() == [[0, 0]]      # -1/8 -> floor(-1/2 + 1/2)
    # longitudes reduced to +-180 are made continuous again, and a repeated closing vertex is dropped
    reduced = [(lat, (lon + 180.0) % 360.0 - 180.0) for lat, lon in ring]
    again = rg.Polygons.from_latlon(window, (H, W), [[reduced + [reduced[0]]]], 0)
    assert again.vertices.tolist() == pg.vertices.tolist() and again.rings.tolist() == pg.rings.tolist()
    # polygons are numbered in their order, rings in theirs; a polygon may have none
    two = rg.Polygons.from_latlon(window, (H, W), [[], [ring, ring[:3]], [ring[1:]]], 0)
    assert two.n_polygons == 3 and two.rings["polygon"].tolist() == [1, 1, 2] and two.rings["first"].tolist() == [0, 5, 8]
    # a ring that comes back a whole turn on winds (8 columns of stride 2 are not the whole circle: only the wind is read here)
    round_ = [(80.5, 0.5), (80.5, 120.5), (80.5, 240.5), (80.5, 360.5)]
    assert rg.Polygons.from_latlon(window, (H, W), [[round_]], 0).rings.tolist() == [(0, 3, 0, 1, 0)]
    assert rg.Polygons.from_latlon(window, (H, W), [[round_[::-1]]], 0).rings["wind"].tolist() == [-1]
    with pytest.raises(ValueError, match="the window does not"):
        rg.Polygons.from_latlon((10, 350, 3, 8, 2, 0), (H, W), [[round_]], 0)
    with pytest.raises(ValueError, match="2\\^24"):
        rg.Polygons.from_latlon((0, 0, 3, 8, 1, 0), (100000, 200000), [[[(0.0, 0.0), (-80.0, 170.0)]]], 8)
    with pytest.raises(ValueError, match="subcell_bits"):
        rg.Polygons.from_latlon(window, (H, W), [[ring]], 9)


def test_corner_latlon_then_from_latlon_is_the_identity():
    rng = np.random.default_rng(5)
    window = (2000, 46000, 40, 96, 480, 1)
    mask = rng.random((40, 96)) < 0.59
    labels, n = rm.label(mask, 4, True)
    rings, v = om.trace(np.asarray(labels, np.int32), 4, True, om.CORNERS)
    ol = rg.Outlines(rings, v, 40, 96, True)
    ll = ol.corner_latlon(window, (23040, 46080))
    polys = [[] for _ in range(n)]
    for r in range(len(ol)):
        a, m = int(rings[r]["first"]), int(rings[r]["n_vertices"])
        polys[int(rings[r]["label"])].append(ll[a:a + m])
    pg = rg.Polygons.from_latlon(window, (23040, 46080), polys, 0)
    order = np.argsort(rings["label"], kind="stable")
    want = np.concatenate([ol.ring(r) for r in order])
    assert (pg.vertices == want).all() and pg.rings["n_vertices"].tolist() == rings["n_vertices"][order].tolist()
    for s in (1, 4, 8):
        assert (rg.Polygons.from_latlon(window, (23040, 46080), polys, s).vertices == want * 2 ** s).all()


# ---- the refusals come before any device call: on a machine without a GPU each still gives its own text
@pytest.fixture
def ctx(native_lib):
    """A context handle; without a GPU mrtx_create stops at its first HIP call but hands the context out."""
    c = C.c_void_p()
    rc_ = native_lib.mrtx_create(C.byref(_lib.MrtxConfig(0, 16, 16, 0, 1, 0, 0)), C.byref(c))
    assert rc_ in (0, -2) and c.value
    yield c
    native_lib.mrtx_destroy(c)


def test_every_refusal_comes_before_any_device_call(native_lib, ctx, monkeypatch):
    monkeypatch.delenv("MOONRT_RASTER", raising=False)
    rings, vertices, labels, cover = rc.refusal_tables()
    base = 1 << 40                      # never dereferenced: a device call with it, or without a device, would not give -1
    for text, kw in rc.refusal_cases(rings, vertices, labels, cover, base):
        rc.assert_refused(native_lib, ctx, text, kw, labels, cover)
    # an unknown value of the variant switch, by name; the two known ones are not refused for it
    F = dict(rings=rings, vertices=vertices, labels=labels, cover=cover, r=rc.block())
    for bad in ("fast", "", "Brute"):
        monkeypatch.setenv("MOONRT_RASTER", bad)
        rc.assert_refused(native_lib, ctx, "MOONRT_RASTER must be bins or brute", F, labels, cover)
    for good in ("bins", "brute"):
        monkeypatch.setenv("MOONRT_RASTER", good)
        rc.assert_refused(native_lib, ctx, "reserved must be 0", dict(F, r=rc.block(reserved=1)), labels, cover)
    assert native_lib.mrtx_rasterise(None, None, None, None, 0, None, None, 0, 0, None, None, None, None, None, None, None) == -1


def test_the_facade_checks_its_arguments():
    from moonrtx_amd.lattice_calls import LatticeCalls
    pg = rg.Polygons.from_rings([(0, [(0, 0), (0, 4), (4, 4)])])
    with pytest.raises(ValueError, match="rule"):
        LatticeCalls.rasterise(None, pg, (4, 4), rule="winding")
    with pytest.raises(ValueError, match="order"):
        LatticeCalls.rasterise(None, pg, (4, 4), order="painter")
    with pytest.raises(ValueError, match="regions.Polygons"):
        LatticeCalls.rasterise(None, (pg.rings, 1, pg.vertices, 3, 1, 0), (4, 4))


# ---- the tool's GeoJSON
def test_the_tools_geojson_parsing_on_model_outlines():
    import rasterise as tool
    import region_outlines as outlines_tool
    window = (20, 100, 6, 8, 2, 1)
    m = np.full((6, 8), -1, np.int32)
    m[0:3, 6:8] = 0
    m[0:3, 0:2] = 0
    m[1, 7] = -1
    m[4, 1:6] = 1
    rings, v = om.trace(m, 4, True, om.CORNERS)
    ol = rg.Outlines(rings, v, 6, 8, True)
    fc = json.loads(json.dumps(outlines_tool.feature_collection(ol, ol.corner_latlon(window, (180, 360)), {})))
    polys, skipped = tool.polygons_of(fc)
    assert skipped == [] and [len(p) for p in polys] == [2, 1] and [len(r) for r in polys[0]] == [5, 5]
    assert polys[0][0][0] == polys[0][0][-1] and isinstance(polys[0][0][0], tuple)
    for s in (0, 4):
        pg = rg.Polygons.from_latlon(window, (180, 360), polys, s)
        assert pg.rings["n_vertices"].tolist() == [4, 4, 4] and pg.rings["polygon"].tolist() == [0, 0, 1]
        for rule in (rs.NONZERO, rs.EVENODD):
            got, cover, _ = rs.raster(pg.rings, pg.vertices, pg.n_polygons, 6, 8, True, s, rule)
            assert (got == m).all() and cover["count"].tolist() == [11, 5]
    # a MultiPolygon's parts are rings of one polygon; a bare geometry is one polygon; other geometries keep their number
    sq = lambda x, y: [[x, y], [x + 1, y], [x + 1, y + 1], [x, y + 1], [x, y]]
    doc = {"type": "FeatureCollection", "features": [
        {"type": "Feature", "properties": {}, "geometry": {"type": "MultiPolygon", "coordinates": [[sq(0, 0), sq(0.25, 0.25)], [sq(5, 5)]]}},
        {"type": "Feature", "properties": {}, "geometry": {"type": "MultiLineString", "coordinates": [sq(1, 1)]}},
        {"type": "Feature", "properties": {}, "geometry": None},
        {"type": "Feature", "properties": {}, "geometry": {"type": "Polygon", "coordinates": [sq(7, 7)]}}]}
    polys, skipped = tool.polygons_of(doc)
    assert skipped == [1, 2] and [len(p) for p in polys] == [3, 0, 0, 1] and polys[3][0][1] == (7.0, 8.0)     # (lat, lon)
    polys, skipped = tool.polygons_of({"type": "Polygon", "coordinates": [sq(2, 3)]})
    assert skipped == [] and polys == [[[(3.0, 2.0), (3.0, 3.0), (4.0, 3.0), (4.0, 2.0), (3.0, 2.0)]]]
    cover = np.zeros(2, rg.COVER_DTYPE)
    cover[1] = (3000000, 1000000, 3, 1, 4, 5, 33, 0)
    assert list(tool.cover_rows(cover, 2.0))[1] == [1, 3, "6.0", 1, "2.0", 4, 5, 33]
