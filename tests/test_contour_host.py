"""The contour lines without a GPU: the model against cases worked by hand, the four identities on
the built and the random lattices, the record's layout, the float64 geometry and the tool's GeoJSON and CSV."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import contour_cases as cc
import contour_model as cm
from moonrtx_amd import _lib
from moonrtx_amd import contours as ct

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

CASES = cc.built_cases()


def traced(name):
    z, levels, wrap = CASES[name]
    lines, vertices = cm.trace(z, levels, wrap)
    return lines, vertices, ct.Contours(lines, vertices, z, levels, wrap)


def fields(lines, *names):
    return [tuple(int(r[n]) for n in names) for r in lines]


# ---- the model against cases worked by hand.  In a 2 x 2 lattice the edges are 0 (N side), 3 (E), 4 (S) and 1 (W).
def test_the_sixteen_patterns_of_one_cell():
    # bit 0 NW, 1 NE, 2 SE, 3 SW above: entry -> exit, the above corners on the right of the way
    want = {0: [], 1: [[0, 1]], 2: [[3, 0]], 3: [[3, 1]], 4: [[4, 3]], 6: [[4, 0]], 7: [[4, 1]], 8: [[1, 4]], 9: [[0, 4]], 11: [[3, 4]],
            12: [[1, 3]], 13: [[0, 3]], 14: [[1, 0]], 15: [],
            5: [[0, 3], [4, 1]],            # NW and SE above, sum 2 >= 4 c - 2 = 2: the centre is above, the below corners are cut off
            10: [[1, 0], [3, 4]]}
    for p, segs in want.items():
        lines, v, cs = traced(f"pattern_{p:02d}")
        assert [cs.line(r).tolist() for r in range(len(cs))] == segs, p
        assert fields(lines, "n_vertices", "level_index", "level", "closed") == [(2, 0, 1, 0)] * len(segs)
        assert [(int(r["head"]), int(r["tail"])) for r in lines] == [(s[0], s[1]) for s in segs]


def test_both_saddles_above_below_and_at_the_tie():
    lines_of = lambda name: [traced(name)[2].line(r).tolist() for r in range(2)]
    # NW and SE above: entries N (0) and S (4).  Centre above: each pairs with the next side clockwise, N -> E, S -> W
    assert lines_of("saddle_nw_se_above") == lines_of("saddle_nw_se_tie") == lines_of("saddle_tie_at_the_bounds") == [[0, 3], [4, 1]]
    # centre below: with the previous side, N -> W, S -> E; one unit under the tie is below
    assert lines_of("saddle_nw_se_below") == lines_of("saddle_nw_se_just_below") == [[0, 1], [4, 3]]
    # NE and SW above: entries E (3) and W (1)
    assert lines_of("saddle_ne_sw_above") == lines_of("saddle_ne_sw_tie") == [[1, 0], [3, 4]]
    assert lines_of("saddle_ne_sw_below") == [[1, 4], [3, 0]]


def test_lattices_without_cells():
    assert len(traced("1x1")[0]) == 0
    # no cell, so no segment: every crossed edge is an open line of its own, one per level that crosses it
    lines, v, _ = traced("1x2")
    assert fields(lines, "first", "n_vertices", "level_index", "level", "head", "tail", "closed") == [(0, 1, 0, 1, 0, 0, 0), (1, 1, 1, 4, 0, 0, 0)]
    lines, v, _ = traced("5x1")
    assert v.tolist() == [1, 1, 3, 3, 5, 5, 7] and (lines["n_vertices"] == 1).all() and not lines["closed"].any()
    lines, v, _ = traced("1x5_wrapped")
    assert v.tolist() == [0, 0, 2, 2, 4, 4, 6, 8]                   # 8: the edge from column 4 back to column 0


def test_a_cone_has_one_closed_line_per_level():
    lines, v, cs = traced("cone")
    assert fields(lines, "first", "n_vertices", "level_index", "level", "head", "tail", "closed") == [(0, 12, 0, 3, 5, 12, 1), (12, 4, 1, 4, 15, 22, 1)]
    # round the summit (node 12) clockwise on the page, the summit on the right: its N, E, S and W edges
    assert cs.line(1).tolist() == [15, 24, 25, 22]
    assert cs.at(0).tolist() == [0] and cs.at(1).tolist() == [1] and cs.at(2).tolist() == []
    # a pit is walked the other way round
    assert traced("pit")[2].line(1).tolist() == [15, 22, 25, 24]


def test_a_ramp_has_open_lines_from_edge_to_edge():
    lines, v, cs = traced("ramp")
    # heights rise eastwards, so the lines run north, from the last row to the first
    assert [cs.line(r).tolist() for r in range(3)] == [[30, 20, 10, 0], [32, 22, 12, 2], [34, 24, 14, 4]]
    assert fields(lines, "level_index", "level", "head", "tail", "closed") == [(0, 5, 30, 0, 0), (1, 15, 32, 2, 0), (2, 25, 34, 4, 0)]
    assert [traced("ramp_down_the_rows")[2].line(r).tolist() for r in range(3)] == [[1, 3, 5, 7], [9, 11, 13, 15], [17, 19, 21, 23]]


def test_levels_on_one_edge_and_levels_that_cross_nothing():
    lines, v, cs = traced("three_levels_on_an_edge")
    assert fields(lines, "level_index", "level", "head", "tail") == [(1, 1, 4, 0), (2, 5, 4, 0), (3, 10, 4, 0)]
    assert v.tolist() == [4, 0] * 3
    assert len(traced("levels_that_cross_nothing")[0]) == 0 and len(traced("all_void")[0]) == 0


def test_lines_open_at_a_void_node():
    lines, v, cs = traced("void_in_the_middle")
    # the 15 and 25 lines end at the cells round node (2, 2) and start again beyond them; 5 and 35 pass by
    assert [cs.line(r).tolist() for r in cs.at(1)] == [[12, 2], [42, 32]]
    assert [cs.line(r).tolist() for r in cs.at(2)] == [[14, 4], [44, 34]]
    assert cs.line(cs.at(0)[0]).tolist() == [40, 30, 20, 10, 0] and cs.line(cs.at(3)[0]).tolist() == [46, 36, 26, 16, 6]
    lines, v, cs = traced("void_row")
    assert [cs.line(r).tolist() for r in range(4)] == [[10, 0], [12, 2], [40, 30], [42, 32]]


def test_the_seam_and_the_pole():
    lines, v, cs = traced("across_the_seam")
    assert fields(lines, "n_vertices", "closed") == [(8, 1)] and cs.wind(0) == 0
    assert v.tolist() == [1, 12, 24, 25, 35, 32, 20, 11]
    lines, v, cs = traced("across_the_seam_unwrapped")
    assert fields(lines, "n_vertices", "head", "tail", "closed") == [(4, 1, 25, 0), (4, 35, 11, 0)]
    lines, v, cs = traced("ring_round_the_pole")
    assert fields(lines, "n_vertices", "head", "tail", "closed") == [(6, 13, 23, 1)] and cs.wind(0) == 1
    assert v.tolist() == [13, 15, 17, 19, 21, 23]                   # eastwards: the higher rows lie on the right
    lines, v, cs = traced("ring_round_the_pole_other_way")
    assert v.tolist() == [13, 23, 21, 19, 17, 15] and cs.wind(0) == -1
    lines, v, cs = traced("ring_round_the_pole_unwrapped")
    assert fields(lines, "n_vertices", "head", "tail", "closed") == [(6, 13, 23, 0)]
    with pytest.raises(ValueError):
        cs.wind(0)


def test_the_long_cases_are_what_their_names_say():
    for name, closed in (("comb_closed", 1), ("comb_open", 0)):
        lines, v, _ = traced(name)
        assert len(lines) == 1 and int(lines[0]["closed"]) == closed and int(lines[0]["n_vertices"]) > 4096
    lines, v, _ = traced("stripes_3x1400")
    assert len(v) > 2 * 2048 and (lines["n_vertices"] == 3).all()
    assert len(CASES["many_levels"][1]) > 4096


# ---- the identities
@pytest.mark.parametrize("name", list(CASES))
def test_the_identities_on_the_built_cases(name):
    z, levels, wrap = CASES[name]
    lines, vertices = cm.trace(z, levels, wrap)
    cm.check_identities(z, levels, wrap, lines, vertices)


@pytest.mark.parametrize("flavour", cc.FLAVOURS)
def test_the_identities_on_random_lattices(flavour):
    cases = cc.random_cases(flavour)
    assert len(cases) >= 200
    n_closed = n_open = 0
    for z, levels, wrap in cases:
        lines, vertices = cm.trace(z, levels, wrap)
        cm.check_identities(z, levels, wrap, lines, vertices)
        n_closed += int(lines["closed"].sum())
        n_open += len(lines) - int(lines["closed"].sum())
    assert n_closed > 20 and n_open > 200


# ---- the refusals come before any device call: on a machine without a GPU each still gives its own text
@pytest.fixture
def ctx(native_lib):
    """A context handle; without a GPU mrtx_create stops at its first HIP call but hands the context out."""
    c = C.c_void_p()
    rc = native_lib.mrtx_create(C.byref(_lib.MrtxConfig(0, 16, 16, 0, 1, 0, 0)), C.byref(c))
    assert rc in (0, -2) and c.value
    yield c
    native_lib.mrtx_destroy(c)


def test_every_refusal_comes_before_any_device_call(native_lib, ctx):
    z, levels, lines, vertices = cc.refusal_tables()
    base = 1 << 40                      # never dereferenced: a device call with it, or without a device, would not give -1
    cases = cc.refusal_cases(z, levels, lines, vertices, base)
    assert len(cases) >= 30
    for text, kw in cases:
        cc.assert_refused(native_lib, ctx, text, kw, lines, vertices)


# ---- the record
def test_line_dtype_mirrors_the_struct():
    assert C.sizeof(_lib.MrtxContourLine) == 32 and _lib.CONTOUR_LINE_DTYPE.itemsize == 32 and cm.LINE == _lib.CONTOUR_LINE_DTYPE
    assert ct.CONTOUR_LINE_DTYPE is _lib.CONTOUR_LINE_DTYPE and C.alignment(_lib.MrtxContourLine) == 8
    for name, ctype in _lib.MrtxContourLine._fields_:
        f = getattr(_lib.MrtxContourLine, name)
        d = _lib.CONTOUR_LINE_DTYPE.fields[name]
        assert d[1] == f.offset and d[0].itemsize == f.size, name
        assert (d[0].kind == "i") == (ctype is C.c_int32), name
    assert [n for n, _ in _lib.MrtxContourLine._fields_] == ["first", "n_vertices", "level_index", "level", "head", "tail", "closed"]
    assert C.sizeof(_lib.MrtxContours) == 20
    assert [n for n, _ in _lib.MrtxContours._fields_] == ["rows", "cols", "wrap", "n_levels", "reserved"]
    assert ct.VOID == cm.VOID == cc.VOID == _lib.FILL_NONE


# ---- the geometry
def test_xy_against_hand_values():
    _, _, cs = traced("ramp")
    # level 5 between 0 and 10: t = (2 x 5 - 1 - 0) / (2 x 10) = 0.45 from the edge's own node, the western one
    assert cs.xy(0).tolist() == [[3.0, 0.45], [2.0, 0.45], [1.0, 0.45], [0.0, 0.45]]
    assert cs.xy(2).tolist() == [[3.0, 2.45], [2.0, 2.45], [1.0, 2.45], [0.0, 2.45]]
    _, _, cs = traced("ramp_down_the_rows")
    assert cs.xy(1).tolist() == [[1.45, 0.0], [1.45, 1.0], [1.45, 2.0], [1.45, 3.0]]
    # from a higher own node down: node 0 at 10, its east neighbour at 0, level 3: t = (6 - 1 - 20) / (2 x -10) = 0.75
    cs = ct.Contours(*cm.trace([[10, 0]], [3], False), np.array([[10, 0]]), [3], False)
    assert cs.xy(0).tolist() == [[0.0, 0.75]]
    # the half unit: level 1 between 0 and 1 lies half way, level 10 between 0 and 10 at 0.95
    _, _, cs = traced("three_levels_on_an_edge")
    assert cs.xy(2)[:, 1].tolist() == [0.95, 0.95] and traced("pattern_02")[2].xy(0).tolist() == [[0.5, 1.0], [0.0, 0.5]]


def test_x_is_unwrapped_across_the_seam():
    _, _, cs = traced("across_the_seam")
    p = cs.xy(0)
    # t = (6 - 1 - 0) / 10 = 0.5 upwards into the block, (6 - 1 - 10) / -10 = 0.5 out of it
    assert p.tolist() == [[0.5, 0.0], [1.0, 0.5], [2.0, 0.5], [2.5, 0.0], [2.5, -1.0], [2.0, -1.5], [1.0, -1.5], [0.5, -1.0]]
    _, _, cs = traced("ring_round_the_pole")
    assert cs.xy(0).tolist() == [[1.45, float(j)] for j in range(6)]
    _, _, cs = traced("ring_round_the_pole_other_way")
    assert cs.xy(0).tolist() == [[1.55, float(j)] for j in (0, -1, -2, -3, -4, -5)]


def test_latlon_against_closed_forms():
    _, _, cs = traced("across_the_seam")
    # stride 2 from row 10, column 350 of a 180 x 360 DEM: node (i, j) is the centre of texel (10 + 2 i, 350 + 2 j), at latitude
    # 90 - (row + 1 / 2) and longitude -180 + (col + 1 / 2) degrees
    ll = cs.latlon(0, (10, 350, 4, 6, 2, 1), (180, 360))
    assert ll.dtype == np.float64 and ll.shape == (8, 2)
    assert ll[:, 0].tolist() == [78.5, 77.5, 75.5, 74.5, 74.5, 75.5, 77.5, 78.5]
    assert ll[:, 1].tolist() == [170.5, 171.5, 171.5, 170.5, 168.5, 167.5, 167.5, 168.5]
    _, _, cs = traced("ring_round_the_pole")
    lon = cs.latlon(0, (0, 354, 4, 6, 1, 1), (180, 360))[:, 1]
    assert lon.tolist() == [174.5, 175.5, 176.5, 177.5, 178.5, 179.5]
    lon = cs.latlon(0, (0, 356, 4, 6, 1, 1), (180, 360))[:, 1]
    assert lon.max() == 181.5                                       # continuous: beyond 180 and not reduced
    with pytest.raises(ValueError):
        cs.latlon(0, (0, 0, 4, 6, 0), (180, 360))


def test_contours_accessors():
    lines, v, cs = traced("void_in_the_middle")
    assert len(cs) == 6 and (cs.rows, cs.cols, cs.wrap) == (5, 5, False)
    assert cs.at(1).tolist() == [0, 3] and cs.at(0).tolist() == [2] and cs.at(9).tolist() == []
    assert np.shares_memory(cs.line(0), cs.vertices)
    with pytest.raises(ValueError):
        ct.Contours(lines, v[:-1], CASES["void_in_the_middle"][0], [5, 15, 25, 35])


def test_levels_for():
    assert ct.levels_for(0, 40, 10).tolist() == [10, 20, 30, 40]            # lo < c <= hi
    assert ct.levels_for(-25, 25, 10).tolist() == [-20, -10, 0, 10, 20]
    assert ct.levels_for(-25, 25, 10, offset=5).tolist() == [-15, -5, 5, 15, 25]
    assert ct.levels_for(3, 3, 1).tolist() == [] and ct.levels_for(3, 4, 7).tolist() == []
    assert ct.levels_for(0, 65536, 1).size == 65536 and ct.levels_for(0, 40, 10).dtype == np.int32
    with pytest.raises(ValueError):
        ct.levels_for(0, 65537, 1)
    with pytest.raises(ValueError):
        ct.levels_for(0, 10, 0)
    # what crosses a lattice is what levels_for lists
    z, _, wrap = CASES["cone"]
    lines, _ = cm.trace(z, ct.levels_for(int(z.min()), int(z.max()), 1), wrap)
    assert sorted(set(lines["level"].tolist())) == list(range(int(z.min()) + 1, int(z.max()) + 1))


# ---- the tool's GeoJSON and CSV
def test_the_tools_geojson_and_csv_on_model_contours():
    import json
    import contour_map as tool
    window = (10, 350, 4, 6, 2, 1)
    _, _, cs = traced("across_the_seam")
    fc = json.loads(json.dumps(tool.feature_collection(cs, window, (180, 360), 0.5)))
    assert fc["type"] == "FeatureCollection" and len(fc["features"]) == 1
    f = fc["features"][0]
    assert f["type"] == "Feature" and f["geometry"]["type"] == "LineString"
    assert f["properties"] == {"line": 0, "level": 1.5, "level_index": 0, "closed": True, "vertices": 8}
    pts = f["geometry"]["coordinates"]
    assert len(pts) == 9 and pts[0] == pts[-1] == [170.5, 78.5] and pts[4] == [168.5, 74.5]       # (lon, lat), closed
    rows = list(tool.vertex_rows(cs, window, (180, 360), 0.5))
    assert len(rows) == 8 and rows[0] == [0, "1.5", 1, 0, 1, "0.5", "0.0", "78.5", "170.5"]
    assert rows[5] == [0, "1.5", 1, 5, 32, "2.0", "-1.5", "75.5", "167.5"] and len(tool.HEADER) == len(rows[0])
    # open lines are not closed, and --min-vertices drops the short ones
    _, _, cs = traced("void_in_the_middle")
    fc = tool.feature_collection(cs, (0, 0, 5, 5), (180, 360), 1.0, min_vertices=3)
    assert [f["properties"]["line"] for f in fc["features"]] == [2, 5]
    assert all(len(f["geometry"]["coordinates"]) == 5 and not f["properties"]["closed"] for f in fc["features"])
    assert len(list(tool.vertex_rows(cs, (0, 0, 5, 5), (180, 360), 1.0, min_vertices=3))) == 10
    # quantising: NaN becomes void, and the level table spans the valid values
    z = tool.quantise(np.array([[0.0, 1.004], [np.nan, -0.126]]), 0.01)
    assert z.tolist() == [[0, 100], [ct.VOID, -13]]
    assert tool.level_table(z, 0.01, interval=0.5).tolist() == [0, 50, 100]
    assert tool.level_table(z, 0.01, levels=[0.5, 0.25, 0.5]).tolist() == [25, 50]
    assert tool.level_table(np.full((2, 2), ct.VOID, np.int32), 0.01, interval=1.0).size == 0
