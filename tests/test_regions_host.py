"""The regions stage without a GPU: the model against hand-written answers, the built cases doing what
they are built for (asserted from the model alone), the row weights, the RegionMap helpers, the record's layout and the
refusals that need no device."""
import ctypes as C
import math

import numpy as np
import pytest

import regions_cases as rc
import regions_model as model
from moonrtx_amd import _lib
from moonrtx_amd import regions as rg


def lab(rows):
    return np.array([[int(c) if c != "." else -1 for c in r.split()] for r in rows], np.int32)


def msk(rows):
    return np.array([[c != "." for c in r.split()] for r in rows], np.uint8)


# ---- the model against answers written by hand, 5 x 7
HAND = [
    # name, mask, connectivity, wrap, labels
    ("two blocks", [". # # . . . .", ". # . . . # #", ". . . . . # .", ". . . . . . .", ". . . . . . ."], 4, False,
     [". 0 0 . . . .", ". 0 . . . 1 1", ". . . . . 1 .", ". . . . . . .", ". . . . . . ."]),
    ("diagonal at 4", ["# . . . . . .", ". # . . . . .", ". . # . . . .", ". . . . . . .", ". . . . . . ."], 4, False,
     ["0 . . . . . .", ". 1 . . . . .", ". . 2 . . . .", ". . . . . . .", ". . . . . . ."]),
    ("diagonal at 8", ["# . . . . . .", ". # . . . . .", ". . # . . . .", ". . . . . . .", ". . . . . . ."], 8, False,
     ["0 . . . . . .", ". 0 . . . . .", ". . 0 . . . .", ". . . . . . .", ". . . . . . ."]),
    ("the seam joins", ["# . . . . . #", ". . . . . . .", "# . . # . . .", ". . . . . . #", ". . . . . . ."], 4, True,
     ["0 . . . . . 0", ". . . . . . .", "1 . . 2 . . .", ". . . . . . 3", ". . . . . . ."]),
    ("the seam's diagonal", ["# . . . . . .", ". . . . . . #", ". . . . . . .", ". . . . . . .", ". . . . . . ."], 8, True,
     ["0 . . . . . .", ". . . . . . 0", ". . . . . . .", ". . . . . . .", ". . . . . . ."]),
    ("no seam without wrap", ["# . . . . . #", ". . . . . . .", ". . . . . . .", ". . . . . . .", ". . . . . . ."], 8, False,
     ["0 . . . . . 1", ". . . . . . .", ". . . . . . .", ". . . . . . .", ". . . . . . ."]),
    ("a late root", [". . . . . . #", "# . # . # . #", "# # # # # # #", ". . . . . . .", ". . . . . . ."], 4, False,
     [". . . . . . 0", "0 . 0 . 0 . 0", "0 0 0 0 0 0 0", ". . . . . . .", ". . . . . . ."]),
]


@pytest.mark.parametrize("name,mask,conn,wrap,want", HAND, ids=[h[0] for h in HAND])
def test_model_labels_by_hand(name, mask, conn, wrap, want):
    got, n = model.label(msk(mask), conn, wrap)
    assert np.array_equal(got, lab(want)) and n == lab(want).max() + 1


def test_model_catalogue_by_hand():
    # a wrapped region: root (0, 0), nodes (0, 0), (0, 6), (1, 6), (1, 5); dj = 0, -1, -1, -2 at cols = 7 (cols / 2 = 3)
    labels = lab(["0 . . . . . 0", ". . . . . 0 0", ". . 1 . . . .", ". . . . . . .", ". . . . . . ."])
    t = model.catalogue(labels, 2, True, np.array([10, 20, 30, 40, 50]))
    assert t[0].tolist() == (60, 2, -4, 4, 0, 0, 0, 1, -2, 0, 0)
    assert t[1].tolist() == (30, 2, 0, 1, 2, 2, 2, 2, 0, 0, 0)
    # the same table unwrapped: dj = 0, 6, 6, 5
    t = model.catalogue(labels, 2, False)
    assert t[0].tolist() == (4, 2, 17, 4, 0, 0, 0, 1, 0, 6, 0)
    # dj = -cols / 2 at even cols: root column 0, node column 3 of 6
    t = model.catalogue(lab(["0 . . 0 . ."]), 1, True)
    assert (t[0]["dj_min"], t[0]["dj_max"], t[0]["sum_dj"]) == (-3, 0, -3)
    # a number no node carries
    t = model.catalogue(lab(["0 . 2"]), 3)
    assert t[1].tolist() == (0, 0, 0, 0, -1, -1, 0, 0, 0, 0, 0)


def test_model_predicate_rounds_the_interval_to_float32():
    lo32, hi32 = np.float32(rc.LO), np.float32(rc.HI)
    assert float(lo32) < rc.LO and float(hi32) > rc.HI          # a float64 comparison would put both out
    f = np.array([[lo32, hi32, np.nextafter(lo32, np.float32(-np.inf)), np.nextafter(hi32, np.float32(np.inf)), np.nan,
                   np.inf, -np.inf, 0.9]], np.float32)
    assert model.predicate(f, 0, rc.LO, rc.HI).tolist() == [[True, True, False, False, False, False, False, True]]
    assert model.predicate(f, 0, -np.inf, np.inf).tolist() == [[True, True, True, True, False, True, True, True]]


# ---- the cases do what they are built for
def tile_crossings(mask, conn, wrap):
    """Edges of the set whose two ends lie in different tiles."""
    rows, cols = mask.shape
    e = model.edges(mask, conn, wrap)
    ti, tj = (e // cols) // rc.TILE[0], (e % cols) // rc.TILE[1]
    return int(((ti[:, 0] != ti[:, 1]) | (tj[:, 0] != tj[:, 1])).sum())


def test_corridors_cross_many_tile_borders_and_are_one_region():
    for name in ("spiral", "serpentine"):
        c = rc.BY_NAME[name]
        assert tile_crossings(c["mask"], 4, False) >= 20, name
        for conn in (4, 8):
            assert rc.answer(c, conn)[1] == 1, name
    # one node wide: no 2 x 2 block of the spiral is full
    m = rc.BY_NAME["spiral"]["mask"]
    assert not (m[:-1, :-1] & m[1:, :-1] & m[:-1, 1:] & m[1:, 1:]).any() and m.sum() > 96 * 96 // 3


def test_locally_separate_pieces_are_separate_inside_every_tile():
    for name in ("comb", "u_down", "u_up"):
        c = rc.BY_NAME[name]
        m = c["mask"]
        assert rc.answer(c, 4)[1] == 1
        most = 0
        for i0 in range(0, m.shape[0], rc.TILE[0]):
            for j0 in range(0, m.shape[1], rc.TILE[1]):
                most = max(most, model.label(m[i0:i0 + rc.TILE[0], j0:j0 + rc.TILE[1]], 8, False)[1])
        assert most >= 2, name
    # the comb: in each of the teeth's tiles every tooth is a component of its own
    m = rc.BY_NAME["comb"]["mask"]
    for i0 in (0, 16):
        for j0 in range(0, m.shape[1], rc.TILE[1]):
            sub = m[i0:i0 + 16, j0:j0 + rc.TILE[1]]
            assert model.label(sub, 8, False)[1] == int(sub[0].sum()) >= 6
    # u_up: the root is in the bar, above and outside the arms' tiles
    assert rc.table(rc.BY_NAME["u_up"], 4)[0]["root_i"] == 15


def test_diagonals_and_checkerboards():
    for name in ("diag_main", "diag_anti", "diag_wrapped"):
        c = rc.BY_NAME[name]
        assert rc.answer(c, 8)[1] == 1 and rc.answer(c, 4)[1] == 64, name
    for name in ("checker_32x66", "checker_33x65", "checker_32x66_wrapped"):
        c = rc.BY_NAME[name]
        assert rc.answer(c, 4)[1] == int(c["mask"].sum()) and rc.answer(c, 8)[1] == 1, name
    # odd cols, wrapped: columns 64 and 0 have one colour, so the seam pairs singletons up
    c = rc.BY_NAME["checker_33x65_wrapped"]
    assert rc.answer(c, 4)[1] == int(c["mask"].sum()) - 17
    assert rc.answer(rc.BY_NAME["empty"], 4)[1] == 0 and rc.answer(rc.BY_NAME["full"], 4)[1] == 1


def test_seam_cases_hit_both_signs_of_dj():
    ring = rc.table(rc.BY_NAME["seam_ring"], 4)
    assert len(ring) == 1 and (ring[0]["dj_min"], ring[0]["dj_max"]) == (-35, 34) and ring[0]["count"] == 140
    first = rc.table(rc.BY_NAME["seam_root_first"], 4)
    assert len(first) == 1 and (first[0]["root_i"], first[0]["root_j"]) == (5, 0)
    assert (first[0]["dj_min"], first[0]["dj_max"]) == (-5, 4)
    last = rc.table(rc.BY_NAME["seam_root_last"], 4)
    assert len(last) == 1 and (last[0]["root_i"], last[0]["root_j"]) == (2, 69)
    assert (last[0]["dj_min"], last[0]["dj_max"]) == (-3, 6)


def test_field_cases_use_every_palette_value_and_the_rounding():
    f = rc.BY_NAME["field_ch0"]["field"]
    assert np.isnan(f).any() and np.isposinf(f).any() and np.isneginf(f).any()
    for ch in range(4):
        c = rc.BY_NAME[f"field_ch{ch}"]
        x = f[:, :, ch]
        want = rc.case_mask(c).astype(bool)
        with np.errstate(invalid="ignore"):
            in64 = (x.astype(np.float64) >= rc.LO) & (x.astype(np.float64) <= rc.HI)
        assert (want & ~in64).any() and not (in64 & ~want).any()        # float32(LO) and float32(HI): in only as float32
        assert 0 < want.sum() < want.size


# ---- row weights
def test_row_weights_sum_to_the_zone():
    R, H, W = 1737400.0, 1800, 3600
    for row0, rows, stride in ((1500, 300, 1), (0, 100, 3), (1502, 99, 3), (0, 1800, 1)):
        unit = 100.0
        w = rg.row_weights((row0, 0, rows, W // stride, stride, 1), (H, W), R, unit)
        assert w.dtype == np.uint32 and w.shape == (rows,)
        first, last = row0, row0 + (rows - 1) * stride
        a = min(0.5 * math.pi - (first + 0.5 - 0.5 * stride) * math.pi / H, 0.5 * math.pi)
        b = max(0.5 * math.pi - (last + 0.5 + 0.5 * stride) * math.pi / H, -0.5 * math.pi)
        zone = 2.0 * math.pi * R * R * (math.sin(a) - math.sin(b))
        total = float(w.astype(np.float64).sum()) * (W // stride) * unit
        # every weight is off by at most half a unit
        assert abs(total - zone) <= 0.5 * unit * rows * (W // stride) + 1e-9 * zone
        assert abs(total - zone) < 1e-4 * zone
    # rows nearer the pole are smaller
    w = rg.row_weights((1500, 0, 300, 3600, 1, 1), (H, W), R, 100.0)
    assert (np.diff(w.astype(np.int64)) < 0).all()


def test_row_weights_refuse_zero_and_overflow():
    with pytest.raises(ValueError, match="rounds to zero"):
        rg.row_weights((1790, 0, 10, 3600), (1800, 3600), 1737400.0, 1e9)
    with pytest.raises(ValueError, match="32 bits"):
        rg.row_weights((900, 0, 10, 3600), (1800, 3600), 1737400.0, 1e-4)
    with pytest.raises(ValueError):
        rg.row_weights((0, 0, 10, 10), (1800, 3600), 1737400.0, 0.0)


# ---- RegionMap on a map the model made
def model_map(name, conn=4, unit=None):
    c = rc.BY_NAME[name]
    labels, n = rc.answer(c, conn)
    t = rc.table(c, conn, weighted=unit is not None)
    return rg.RegionMap(labels, t.astype(rg.REGION_DTYPE), c["wrap"], unit)


def test_region_dtype_mirrors_the_record():
    assert C.sizeof(_lib.MrtxRegion) == 56 and rg.REGION_DTYPE.itemsize == 56
    assert C.sizeof(_lib.MrtxRegions) == 48
    for name, _ in _lib.MrtxRegion._fields_:
        assert rg.REGION_DTYPE.fields[name][1] == getattr(_lib.MrtxRegion, name).offset, name
    assert rg.REGION_DTYPE.names == tuple(n for n, _ in _lib.MrtxRegion._fields_) == model.RECORD.names


def test_region_map_helpers():
    m = model_map("random_0.59", 4, unit=2.5)
    assert m.n == len(m.table) and m.labels.shape == (200, 136) and m.n > 50
    area = m.area_m2()
    assert area.shape == (m.n,) and np.array_equal(area, m.table["weight"] * 2.5)
    assert np.array_equal(m.area_m2(1.0), m.table["weight"].astype(np.float64))
    big = m.largest(3)
    assert len(big) == 3 and (np.diff(m.table["weight"][big].astype(np.int64)) <= 0).all()
    assert m.table["weight"][big[0]] == m.table["weight"].max()
    f = m.filter(min_count=5)
    keep = m.table["count"] >= 5
    assert f.n == keep.sum() and np.array_equal(f.table, m.table[keep])
    assert ((f.labels >= 0) == np.isin(m.labels, np.flatnonzero(keep))).all() and f.labels.max() == f.n - 1
    # the kept regions keep their nodes and their order
    for new, old in enumerate(np.flatnonzero(keep)[:10]):
        assert np.array_equal(f.labels == new, m.labels == old)
    g = m.filter(min_area=float(np.median(area)))
    assert 0 < g.n < m.n and (g.area_m2() >= np.median(area)).all()
    with pytest.raises(ValueError):
        model_map("random_0.59").area_m2()


def test_centroids_stay_on_the_seam():
    m = model_map("seam_root_first")
    lat = 10.0 - np.arange(20) * 0.5
    lon = -180.0 + (np.arange(70) + 0.5) * (360.0 / 70)
    c = m.centroids(lat, lon)
    # rows 5 .. 8, columns 65 .. 69 and 0 .. 4: the centroid is on the seam, at longitude +-180
    assert c.shape == (1, 2) and abs(c[0, 0] - (10.0 - 6.5 * 0.5)) < 1e-12
    assert abs(abs(c[0, 1]) - 180.0) < 1e-9
    u = model_map("u_down")
    c = u.centroids(np.arange(50.0), np.arange(120.0))
    ii, jj = np.nonzero(rc.BY_NAME["u_down"]["mask"])
    assert abs(c[0, 0] - ii.mean()) < 1e-9 and abs(c[0, 1] - jj.mean()) < 1e-9


# ---- refusals that need no device
def test_null_context_is_refused_without_a_gpu(native_lib):
    r = _lib.MrtxRegions(4, 4, 0, 4, 1, 0, -math.inf, math.inf, 0)
    mask = np.ones((4, 4), np.uint8)
    labels = np.full((4, 4), 7, np.int32)
    n = C.c_uint32(1234)
    assert native_lib.mrtx_regions_label(None, C.byref(r), None, None, None, mask.ctypes.data, None, labels.ctypes.data,
                                         C.byref(n), None) == -1
    assert n.value == 1234 and (labels == 7).all()
    table = np.zeros(1, rg.REGION_DTYPE)
    assert native_lib.mrtx_regions_stats(None, 4, 4, 0, None, labels.ctypes.data, 1, None, None, table.ctypes.data, None) == -1
    assert native_lib.mrtx_last_error(None) == b"null context"
    assert native_lib.mrtx_abi_version() == 7
