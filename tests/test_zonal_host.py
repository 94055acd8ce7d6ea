"""The zonal statistics and outlines of labelled regions without a GPU: the independent model
(tests/zonal_model.py) against cases worked by hand, the numpy dtypes against the ctypes structs, the side lengths against
the closed forms of a meridian and a parallel, the refusal of a null context, and the helpers of moonrtx_amd.regions."""
import ctypes as C
import math

import numpy as np
import pytest

import zonal_model as zm
from moonrtx_amd import _lib
from moonrtx_amd import regions as rg

INF = math.inf


def test_the_order_key_is_the_total_order_of_the_bits():
    x = np.array([-INF, -3.5, -1e-45, -0.0, 0.0, 1e-45, 2.0, INF], np.float32)
    k = zm.order_key(x)
    assert (np.diff(k.astype(np.int64)) > 0).all()
    assert k[3] + 1 == k[4]                                  # -0.0 and +0.0 are neighbours, in that order


def test_the_fixed_point_rounds_half_to_even_and_clips():
    q, c = zm.fixed(np.array([0.5, 1.5, 2.5, -0.5, -1.5, 0.25], np.float32), 1.0)
    assert q == [0, 2, 2, 0, -2, 0] and not c.any()
    q, c = zm.fixed(np.array([2.0 ** 31, -2.0 ** 31, 2.0 ** 31 - 128, INF, -INF, 3e38], np.float32), 1.0)
    assert q == [2 ** 31, -2 ** 31, 2 ** 31 - 128, 2 ** 31, -2 ** 31, 2 ** 31] and c.tolist() == [True, True, False, True, True, True]
    q, c = zm.fixed(np.array([1.0], np.float32), 2.0 ** 31)
    assert q == [2 ** 31] and c.all()
    assert [rg.fixed_point(v, 4.0) for v in (0.125, 0.375, -INF, 1e30)] == [0, 2, -2 ** 31, 2 ** 31]


def test_zonal_by_hand_3x3():
    labels = np.array([[0, 0, 1], [0, -1, 1], [2, 2, 1]], np.int32)
    field = np.array([[1.5, np.nan, -0.0], [2.5, 9.0, 0.0], [np.nan, np.nan, -0.0]], np.float32)
    w = np.array([10, 20, 30], np.uint32)
    z = zm.zonal(labels, 4, field, 2.0, w)[:, 0]
    # region 0: nodes 0 (1.5), 1 (NaN), 3 (2.5): q = 3 and 5
    assert tuple(z[0].tolist()) == (30, 10 * 3 + 20 * 5, 8, 2, 1, 0, 1.5, 2.5, 0, 3, 0)
    # region 1: -0.0 at node 2, +0.0 at node 5, -0.0 at node 8: the minimum is the first -0.0, the maximum the +0.0
    assert tuple(z[1].tolist())[:6] == (60, 0, 0, 3, 0, 0)
    assert (z[1]["min_at"], z[1]["max_at"]) == (2, 5) and np.signbit(z[1]["min"]) and not np.signbit(z[1]["max"])
    # region 2: all NaN; region 3: no node
    for r, nan in ((2, 2), (3, 0)):
        assert tuple(z[r].tolist()) == (0, 0, 0, 0, nan, 0, INF, -INF, -1, -1, 0)
    # without weights wcount = count and wsum = sum
    u = zm.zonal(labels, 4, field, 2.0)[:, 0]
    assert (u["wcount"] == u["count"]).all() and (u["wsum"] == u["sum"]).all()
    # a histogram of two bins over [0, 4): -0.0 -> t = 0 -> bin 1; 2.5 -> bin 2; 9 is outside every region
    h = zm.histogram(labels, 4, field, 2, 0.0, 0.5, w)
    assert h.tolist() == [[0, 10, 20, 0], [0, 60, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]]
    h = zm.histogram(labels, 4, field, 1, 1.5, 1.0)
    assert h.tolist() == [[0, 1, 1], [3, 0, 0], [0, 0, 0], [0, 0, 0]]       # 1.5 -> t = 0 in the bin, 2.5 -> t = 1 = n_bins: above


def test_sums_fold_modulo_2_64():
    labels = np.zeros((2, 2), np.int32)
    field = np.full((2, 2), 2.0 ** 29, np.float32)
    w = np.array([2 ** 32 - 1, 2 ** 32 - 1], np.uint32)
    z = zm.zonal(labels, 1, field, 2.0, w)[0, 0]
    exact = 4 * (2 ** 32 - 1) * 2 ** 30
    assert exact >= 2 ** 63 and z["wsum"] == exact - 2 ** 64 and zm.wsum_exact(labels, 0, field, 2.0, w) == exact
    with pytest.raises(OverflowError, match="lower scale"):
        rg.check_wsum(zm.zonal(labels, 1, field, 2.0, w), 2.0)
    rg.check_wsum(zm.zonal(labels, 1, field, 0.5, w), 0.5)            # 2^28 x 2^34: fits


def test_shape_by_hand_4x5():
    # a ring of region 0 round a hole of -1 and region 1, and a diagonal pair of region 2
    labels = np.array([[0, 0, 0, -1, 2],
                       [0, -1, 0, 2, -1],
                       [0, 1, 0, -1, -1],
                       [0, 0, 0, -1, -1]], np.int32)
    for conn in (4, 8):
        s = zm.shape(labels, 3, conn)
        assert (s[0]["perimeter"], s[0]["sides_ns"], s[0]["sides_ew"]) == (20, 8, 12)
        assert (s[0]["q1"], s[0]["q3"], s[0]["qd"], s[0]["euler"]) == (4, 4, 0, 0)
        assert zm.holes(labels, 0, conn) == 1 and zm.euler_vef(labels, 0, conn) == 0
        assert (s[1]["perimeter"], s[1]["q1"], s[1]["q3"], s[1]["qd"], s[1]["euler"]) == (4, 4, 0, 0, 1)
        # two nodes that touch at a corner: two pieces for 4, one for 8
        assert (s[2]["perimeter"], s[2]["q1"], s[2]["q3"], s[2]["qd"]) == (8, 6, 0, 1)
        assert s[2]["euler"] == (2 if conn == 4 else 1) == zm.components(labels, 2, conn) == zm.euler_vef(labels, 2, conn)
    # side lengths: north/south sides by the row line they lie on, east/west sides by their row
    ew, ns = np.array([1, 10, 100, 1000]), np.array([1, 2, 4, 8, 16]) * 10000
    s = zm.shape(labels, 3, 4, False, ew, ns)
    assert s[1]["perimeter"] == 2 * 100 + 40000 + 80000
    assert s[2]["perimeter"] == (2 * 1 + 10000 + 20000) + (2 * 10 + 20000 + 40000)


def test_shape_by_hand_3x3_wrapped():
    full = np.zeros((3, 3), np.int32)
    s = zm.shape(full, 1, 4, True)[0]
    # every column joins the next: only the first and last row lines bound the region, and it winds round the seam
    assert (s["perimeter"], s["sides_ns"], s["sides_ew"], s["q1"], s["q3"], s["qd"], s["euler"]) == (6, 6, 0, 0, 0, 0, 0)
    assert zm.euler_vef(full, 0, 4, True) == 0 == zm.euler_vef(full, 0, 8, True)
    s = zm.shape(full, 1, 4, False)[0]
    assert (s["perimeter"], s["q1"], s["euler"]) == (12, 4, 1)
    col = np.array([[-1, 0, -1]] * 3, np.int32)
    s = zm.shape(col, 1, 8, True)[0]
    assert (s["perimeter"], s["q1"], s["q3"], s["euler"]) == (8, 4, 0, 1)
    seam = np.array([[0, -1, 0]] * 3, np.int32)                 # columns 2 and 0 are neighbours across the seam
    s = zm.shape(seam, 1, 4, True)[0]
    assert (s["perimeter"], s["sides_ew"], s["q1"], s["euler"]) == (10, 6, 4, 1)


def test_the_three_routes_to_the_euler_number_agree_on_random_masks():
    rng = np.random.default_rng(5)
    for k in range(40):
        rows, cols = rng.integers(1, 9, 2)
        labels = (rng.random((rows, cols)) < 0.6).astype(np.int32) - 1
        for conn in (4, 8):
            s = zm.shape(labels, 1, conn)[0]
            assert s["euler"] == zm.components(labels, 0, conn) - zm.holes(labels, 0, conn) == zm.euler_vef(labels, 0, conn), (k, conn)
            if cols >= 3:
                assert zm.shape(labels, 1, conn, True)[0]["euler"] == zm.euler_vef(labels, 0, conn, True), (k, conn)


def test_dtypes_mirror_the_structs():
    for dt, st, size in ((rg.ZONAL_DTYPE, _lib.MrtxZonal, 56), (rg.SHAPE_DTYPE, _lib.MrtxRegionShape, 32),
                         (zm.ZONAL, _lib.MrtxZonal, 56), (zm.SHAPE, _lib.MrtxRegionShape, 32)):
        assert dt.itemsize == C.sizeof(st) == size
        assert [n for n, _ in st._fields_] == list(dt.names)
        for name, ct in st._fields_:
            assert dt.fields[name][1] == getattr(st, name).offset and dt.fields[name][0].itemsize == C.sizeof(ct), name
            assert dt.fields[name][0].kind == {C.c_uint64: "u", C.c_uint32: "u", C.c_int64: "i", C.c_int32: "i", C.c_float: "f"}[ct]
    assert C.sizeof(_lib.MrtxZonalSpec) == 56
    assert [(_n, getattr(_lib.MrtxZonalSpec, _n).offset) for _n, _ in _lib.MrtxZonalSpec._fields_] == [
        ("rows", 0), ("cols", 4), ("wrap", 8), ("n_ch", 12), ("scale", 16), ("hist_ch", 24), ("n_bins", 28), ("hist_lo", 32),
        ("hist_inv_w", 40), ("reserved", 48)]


def test_side_weights_sum_to_the_meridian_and_the_parallels():
    H, W, R = 1800, 3600, 1737400.0
    window = (300, 0, 200, 900, 3)                              # rows 300, 303 .. 897: cells of three DEM rows
    ew, ns = rg.side_weights(window, (H, W), R, 0.01)
    assert ew.dtype == ns.dtype == np.uint32 and ew.shape == (200,) and ns.shape == (201,)
    lat_n = math.pi / 2 - (300 + 0.5 - 1.5) * math.pi / H
    lat_s = math.pi / 2 - (897 + 0.5 + 1.5) * math.pi / H
    # the east sides of one column add up to the meridian arc between the window's edges (each rounded to a centimetre)
    assert abs(int(ew.astype(np.int64).sum()) * 0.01 - R * (lat_n - lat_s)) <= 200 * 0.005
    # every row line is a parallel: R cos(lat) dlon, and all 900 columns of it the window's share of the circle
    dlon = 3 * 2 * math.pi / W
    for k in (0, 1, 57, 200):
        lat = lat_n - k * 3 * math.pi / H
        assert abs(int(ns[k]) * 0.01 - R * math.cos(lat) * dlon) <= 0.005 + 1e-6
    assert abs(int(ns[0]) * 900 * 0.01 - 2 * math.pi * R * math.cos(lat_n) * (2700 / W)) <= 900 * 0.006
    # a side on a pole has no length; a unit too fine does not fit
    with pytest.raises(ValueError, match="rounds to zero"):
        rg.side_weights((0, 0, 10, 10), (H, W), R, 1.0)
    with pytest.raises(ValueError, match="does not fit 32 bits"):
        rg.side_weights(window, (H, W), R, 1e-7)
    with pytest.raises(ValueError):
        rg.side_weights((1700, 0, 200, 10), (H, W), R, 1.0)


def test_null_context_is_refused_without_a_gpu(native_lib):
    z = _lib.MrtxZonalSpec(4, 4, 0, 1, 1.0, 0, 0, 0.0, 1.0, 0)
    labels = np.zeros((4, 4), np.int32)
    field = np.ones((4, 4), np.float32)
    table = np.zeros(1, rg.ZONAL_DTYPE)
    assert native_lib.mrtx_regions_zonal(None, C.byref(z), None, labels.ctypes.data, 1, None, field.ctypes.data, None, None,
                                         table.ctypes.data, None, None, None) == -1
    shape = np.zeros(1, rg.SHAPE_DTYPE)
    assert native_lib.mrtx_regions_shape(None, 4, 4, 0, 4, None, labels.ctypes.data, 1, None, None, None, shape.ctypes.data,
                                         None) == -1
    assert (table.view(np.uint8) == 0).all() and (shape.view(np.uint8) == 0).all()
    assert native_lib.mrtx_last_error(None) == b"null context"
    assert native_lib.mrtx_abi_version() == 7


def test_the_helpers():
    z = np.zeros((2, 2), rg.ZONAL_DTYPE)
    z["count"], z["sum"], z["wcount"], z["wsum"] = [[4, 0], [2, 1]], [[10, 0], [-3, 7]], [[8, 0], [20, 5]], [[40, 0], [-10, 35]]
    assert np.array_equal(rg.zonal_mean(z, 2.0), [[1.25, np.nan], [-0.75, 3.5]], equal_nan=True)
    assert np.array_equal(rg.zonal_area_mean(z, 2.0), [[2.5, np.nan], [-0.25, 3.5]], equal_nan=True)
    s = np.zeros(3, rg.SHAPE_DTYPE)
    s["euler"] = [1, 0, -4]
    h, wind = rg.holes(s)
    assert h.tolist() == [0, 1, 5] and not wind.any()
    t = np.zeros(3, rg.REGION_DTYPE)
    t["count"], t["dj_min"], t["dj_max"] = [5, 70, 0], [-2, -35, 0], [2, 34, 0]
    h, wind = rg.holes(s, t, 70, True)
    assert wind.tolist() == [False, True, False]
    assert not rg.holes(s, t, 70, False)[1].any()
    m = rg.RegionMap(np.zeros((2, 70), np.int32), t, True, None)
    assert m.holes(s)[1].tolist() == [False, True, False]
