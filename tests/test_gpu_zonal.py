"""The zonal statistics and outlines of labelled regions on the MI355X (DESIGN.md sections 3.21 and 4.27): every field of every
record and every histogram column equal to the model's (tests/zonal_model.py), from host and from device tables, with and
without row weights, in the run-reduced and the plain variant, the outlines at both connectivities; labels from the built cases
of the regions stage and from cases made here; every refusal; a bad label table; the launch count; the render state; the tool.
Everything is compared with ==, floats by their bits.

One point of the plan could not be met as written: 65536 nodes of weights near 2^32 - 1 make wcount about 2^48, so the guard
max |q| wcount < 2^63 passes only for |q| <= 2^15.  The heavy case therefore has q just below 2^15 (wsum about 2^62.99, more
than 62 bits, the guard passes), and the case with q near 2^30 is the one in which the guard must raise."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import lattice_cases as lc
import model_cases as mc
import regions_cases as rc
import zonal_model as zm
from common import assert_bit_equal
from moonrtx_amd import _lib
from moonrtx_amd import regions as rg
from moonrtx_amd.renderer import DeviceBuffer, MoonRT, MoonRTError
from moonrtx_amd.scene import named_scene
from test_gpu_illumination import make

pytestmark = pytest.mark.gpu

INF = math.inf
F32 = np.float32


@pytest.fixture(scope="module")
def rt(native_lib):
    """One context for the module, without a DEM, a light or a Moon frame: the stage needs none of them."""
    r = MoonRT(16, 16)
    yield r
    r.close()


# ---- label tables
def rings():
    """Three ring regions on a 30 x 50 lattice: 0 with one hole (an island of region 3), 1 with two (an island of -1 and one of
    region 4), 2 with five one-node holes of -1; region 5 fills the rest of the first rows."""
    lab = np.full((30, 50), -1, np.int32)
    lab[0:2, :] = 5
    lab[3:10, 2:12] = 0
    lab[5:8, 5:9] = 3
    lab[3:12, 15:40] = 1
    lab[5:9, 18:22] = -1
    lab[6:10, 30:36] = 4
    lab[14:28, 3:47] = 2
    for i, j in ((16, 5), (16, 40), (20, 20), (25, 8), (26, 44)):
        lab[i, j] = -1
    return lab


def seam_ring():
    """Rows 2 .. 6 all the way round a wrapped 9 x 12 window with one hole: the region winds round the seam."""
    lab = np.full((9, 12), -1, np.int32)
    lab[2:7, :] = 0
    lab[3:5, 5:7] = -1
    return lab


def blocks(rows, cols, seed, n=5):
    """A caller's table: blocks of 2 x 3 nodes numbered by a hash, some -1."""
    i, j = np.mgrid[0:rows, 0:cols]
    h = ((i // 2) * 2654435761 + (j // 3) * 40503 + seed * 97) % 4294967296
    h = (h ^ (h >> 13)) * 1274126177 % 4294967296
    return ((h >> 7) % (n + 1)).astype(np.int32) - 1


def long_rows():
    """16 x 1025: region 0 fills whole rows, so its runs cross row ends and the ends of the waves' stretches of 1024 nodes;
    regions 1 and 2 are islands inside it and region 3 the last column of some rows."""
    lab = np.zeros((16, 1025), np.int32)
    lab[3:5, 100:164] = 1
    lab[7, 1000:1025] = 2
    lab[8, 0:40] = 2
    lab[10:14, 1024] = 3
    lab[15, 500:600] = -1
    return lab


@functools.lru_cache(maxsize=None)
def label_cases():
    out = {}
    for name in ("spiral", "serpentine", "comb", "diag_main", "diag_anti", "diag_wrapped", "checker_32x66",
                 "checker_32x66_wrapped", "checker_33x65", "checker_33x65_wrapped", "seam_ring", "seam_root_first",
                 "seam_root_last", "random_0.59_wrapped"):
        case = rc.BY_NAME[name]
        labels, n = rc.answer(case, 4)
        out[name] = (np.array(labels, np.int32), int(n), case["wrap"])
    out["1x40"] = (blocks(1, 40, 1), 5, False)
    out["40x1"] = (blocks(40, 1, 2), 5, False)
    out["3x3_wrapped"] = (np.array([[0, -1, 0], [1, 1, 0], [2, 1, -1]], np.int32), 3, True)
    out["17x65"] = (blocks(17, 65, 3), 5, False)
    out["17x65_wrapped"] = (blocks(17, 65, 3), 5, True)
    out["16x1025"] = (long_rows(), 4, False)
    out["rings"] = (rings(), 6, False)
    out["seam_ring_hole"] = (seam_ring(), 1, True)
    mine = np.random.default_rng(9).integers(-1, 6, (37, 70)).astype(np.int32)
    mine[mine == 3] = -1                                    # number 3 has no node; the others are scattered, not connected
    out["callers_own"] = (mine, 6, False)
    out["callers_own_wrapped"] = (mine, 6, True)
    i, j = np.mgrid[0:19, 0:67]
    out["two_checkerboards"] = (((i + j) % 2).astype(np.int32), 2, True)     # every window holds both labels, each on a diagonal
    for v in out.values():
        v[0].setflags(write=False)
    return out


NAMES = ["spiral", "serpentine", "comb", "diag_main", "diag_anti", "diag_wrapped", "checker_32x66", "checker_32x66_wrapped",
         "checker_33x65", "checker_33x65_wrapped", "seam_ring", "seam_root_first", "seam_root_last", "random_0.59_wrapped",
         "1x40", "40x1", "3x3_wrapped", "17x65", "17x65_wrapped", "16x1025", "rings", "seam_ring_hole", "callers_own",
         "callers_own_wrapped", "two_checkerboards"]


# ---- fields
def hash_field(rows, cols, n_ch, seed=0):
    """(rows, cols, n_ch) float32 from an integer hash: coarse values (many equal extremes, in different waves), and NaN, +-inf,
    -0.0, +0.0 and values with |x * 8| >= 2^31 sprinkled in.  Channel 1 is constant: its extremes lie at a region's root."""
    i, j, c = np.mgrid[0:rows, 0:cols, 0:n_ch].astype(np.uint64)
    h = (i * 73856093 + j * 19349663 + c * 83492791 + seed * 2654435761) % 4294967296
    h = ((h ^ (h >> 15)) * 2246822519) % 4294967296
    h = ((h ^ (h >> 13)) * 3266489917) % 4294967296
    h ^= h >> 16
    x = (((h >> 8) % 61).astype(np.float64) * 0.25 - 7.5).astype(F32)
    for mod, val in ((23, np.nan), (29, INF), (31, -INF), (37, -0.0), (41, 0.0), (43, 3.0e8), (47, -2.9e8), (53, 2.0 ** 28),
                     (59, 0.3125), (67, -0.4375)):
        x[h % mod == 0] = F32(val)
    if n_ch > 1:
        x[:, :, 1] = F32(-2.5)
    return np.ascontiguousarray(x)


def weights_for(rows):
    return (1000 + 7 * np.arange(rows)).astype(np.uint32)


SCALE = 8.0
N_CH = {0: 1, 1: 3, 2: 16}


def assert_records_equal(got, want, what):
    assert got.dtype == rg.ZONAL_DTYPE or got.dtype == rg.SHAPE_DTYPE
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for name in got.dtype.names:
        a, b = got[name], want[name]
        if a.dtype.kind == "f":
            a, b = a.view(np.uint32), np.ascontiguousarray(b, F32).view(np.uint32)
        if not np.array_equal(a, b):
            k = tuple(np.argwhere(a != b)[0])
            raise AssertionError(f"{what}: {name} differs, first in record {k}: {got[k]} vs {want[k]}")


def run_zonal(rt, labels, n, field, weights, device, hist=None, wrap=False, scale=SCALE, stats=None):
    if not device:
        return rt.region_statistics(labels, n, field, row_weights=weights, scale=scale, hist=hist, wrap=wrap, stats=stats)
    lab, fld = DeviceBuffer(max(labels.nbytes, 4)), DeviceBuffer(max(field.nbytes, 4))
    try:
        lab.upload(labels)
        fld.upload(field)
        return rt.region_statistics(lab, n, fld, row_weights=weights, scale=scale, hist=hist, wrap=wrap, shape=field.shape,
                                    stats=stats)
    finally:
        lab.free()
        fld.free()


def run_shape(rt, labels, n, conn, wrap, device, ew=None, ns=None, stats=None):
    if not device:
        return rt.region_shapes(labels, n, conn, wrap, ew, ns, stats=stats)
    lab = DeviceBuffer(max(labels.nbytes, 4))
    try:
        lab.upload(labels)
        return rt.region_shapes(lab, n, conn, wrap, ew, ns, shape=labels.shape, stats=stats)
    finally:
        lab.free()


@pytest.mark.parametrize("name", NAMES)
def test_zonal_equals_the_model(rt, monkeypatch, name):
    labels, n, wrap = label_cases()[name]
    rows, cols = labels.shape
    n_ch = N_CH[NAMES.index(name) % 3] if labels.size < 20000 else 3
    field = hash_field(rows, cols, n_ch, NAMES.index(name))
    w = weights_for(rows)
    hist_ch, n_bins, lo, hi = n_ch - 1, 7, -2.0, 5.0
    for weights in (None, w):
        want = zm.zonal(labels, n, field, SCALE, weights)
        want_h = zm.histogram(labels, n, field[:, :, hist_ch], n_bins, lo, n_bins / (hi - lo), weights)
        for variant in ("runs", "plain"):
            monkeypatch.setenv("MOONRT_REGIONS_ZONAL", variant)
            for device in (False, True):
                what = f"{name}, {n_ch} channels, {variant}, {'device' if device else 'host'} tables, " \
                       f"{'row weights' if weights is not None else 'no weights'}"
                got = run_zonal(rt, labels, n, field, weights, device, wrap=wrap)
                assert_records_equal(got, want, what)
                got, h = run_zonal(rt, labels, n, field, weights, device, (hist_ch, n_bins, lo, hi), wrap)
                assert_records_equal(got, want, what + ", with a histogram")
                assert h.dtype == np.uint64 and np.array_equal(h, want_h), what
    # the field has what it is meant to have
    if labels.size >= 2000:
        assert want["n_nan"].sum() > 0 and want["n_clipped"].sum() > 0


@pytest.mark.parametrize("name", NAMES)
def test_shapes_equal_the_model(rt, monkeypatch, name):
    labels, n, wrap = label_cases()[name]
    rows = labels.shape[0]
    ew = (3 + 5 * np.arange(rows)).astype(np.uint32)
    ns = (2 ** 32 - 1 - 11 * np.arange(rows + 1)).astype(np.uint32)         # near 2^32 - 1: the perimeter needs 64 bits
    for conn in (4, 8):
        for sides in (None, (ew, ns)):
            want = zm.shape(labels, n, conn, wrap, *(sides or (None, None)))
            for variant in ("runs", "plain"):
                monkeypatch.setenv("MOONRT_REGIONS_ZONAL", variant)
                for device in (False, True):
                    got = run_shape(rt, labels, n, conn, wrap, device, *(sides or (None, None)))
                    assert_records_equal(got, want, f"{name}, {conn}-connected, {variant}, {'device' if device else 'host'} "
                                                    f"tables, {'side lengths' if sides else 'unit sides'}")


def test_holes_of_rings_and_the_ring_round_the_seam(rt):
    labels, n, _ = label_cases()["rings"]
    for conn in (4, 8):
        s = rt.region_shapes(labels, n, conn)
        h, wind = rg.holes(s)
        assert h[:3].tolist() == [1, 2, 5] and not wind.any()
        for r in range(n):
            assert zm.components(labels, r, conn) == 1
            assert h[r] == zm.holes(labels, r, conn) and s["euler"][r] == zm.euler_vef(labels, r, conn), (conn, r)
    # a region that winds round the seam reads one hole more: its Euler number is V - E + F, not 1 - holes
    labels, n, wrap = label_cases()["seam_ring_hole"]
    for conn in (4, 8):
        s = rt.region_shapes(labels, n, conn, wrap)
        assert s["euler"][0] == zm.euler_vef(labels, 0, conn, True) == -1
        m = rt.regions(mask=(labels >= 0).astype(np.uint8), connectivity=conn, wrap=True)
        assert m.n == 1 and m.holes(m.shapes(rt, conn))[1].tolist() == [True]
    # a caller's label that is not connected reads components minus holes
    labels, n, _ = label_cases()["callers_own"]
    for conn in (4, 8):
        s = rt.region_shapes(labels, n, conn)
        for r in (0, 3, 5):
            assert s["euler"][r] == zm.components(labels, r, conn) - zm.holes(labels, r, conn), (conn, r)
        assert s[3].tolist() == (0, 0, 0, 0, 0, 0, 0)


def special_case():
    """4 x 130: region 0 holds NaN, +-inf, -0.0 and +0.0 (the zeros twice, the later -0.0 and the earlier +0.0 must not win),
    region 1 is all NaN, region 2 holds two equal maxima 200 nodes apart and values that clip."""
    lab = np.zeros((4, 130), np.int32)
    lab[2, :] = 1
    lab[3, :] = 2
    x = np.full((4, 130, 1), 1.0, F32)
    x[0, 3], x[0, 70], x[1, 5], x[1, 100] = 0.0, -0.0, -0.0, 0.0
    x[0, 10], x[1, 90], x[0, 129], x[1, 0] = np.nan, np.nan, INF, -INF
    x[2, :] = np.nan
    x[3, :, 0] = np.linspace(-5, 5, 130).astype(F32)
    x[3, 7], x[3, 120] = 2.0 ** 31, 2.0 ** 31
    x[3, 60], x[3, 61] = -2.0 ** 31, np.nextafter(F32(2.0 ** 31), F32(0))
    return lab, x


def test_special_values(rt, monkeypatch):
    lab, x = special_case()
    for scale in (1.0, 0.5):
        want = zm.zonal(lab, 3, x, scale, weights_for(4))
        assert want[0, 0]["min"] == -INF and want[0, 0]["max"] == INF and want[0, 0]["n_nan"] == 2 and want[0, 0]["n_clipped"] == 2
        assert tuple(want[1, 0].tolist()) == (0, 0, 0, 0, 130, 0, INF, -INF, -1, -1, 0)
        assert (want[2, 0]["max_at"], want[2, 0]["min_at"]) == (3 * 130 + 7, 3 * 130 + 60)
        assert want[2, 0]["n_clipped"] == (3 if scale == 1.0 else 0)
        for variant in ("runs", "plain"):
            monkeypatch.setenv("MOONRT_REGIONS_ZONAL", variant)
            for device in (False, True):
                assert_records_equal(run_zonal(rt, lab, 3, x, weights_for(4), device, scale=scale), want, f"{variant}, scale {scale}")
    # without the infinities the zeros are the extremes of a field of zeros: -0.0 precedes +0.0, the least index of each wins
    z = np.zeros((4, 130, 1), F32)
    z[0, 3], z[0, 70], z[1, 5] = 0.0, -0.0, -0.0
    got = run_zonal(rt, np.zeros((4, 130), np.int32), 1, z, None, False)
    assert (got[0, 0]["min_at"], got[0, 0]["max_at"]) == (70, 0) and np.signbit(got[0, 0]["min"]) and not np.signbit(got[0, 0]["max"])
    assert_records_equal(got, zm.zonal(np.zeros((4, 130), np.int32), 1, z, SCALE), "zeros")


@pytest.mark.parametrize("n_bins", [1, 7, 100, 4096])
def test_histogram_edges(rt, monkeypatch, n_bins):
    """Values at lo, at hi, one ulp either side of both and at an inner bin edge, in three regions.  Rows of 3, 9 and 102
    columns are carried along a wave's stretch (102: by both of a lane's accumulators), rows of 4098 are not."""
    lo, hi = F32(0.7), F32(2.2)                              # float32 values, so that a field value can equal them
    inner = F32(float(lo) + (float(hi) - float(lo)) * (max(n_bins // 2, 1) / n_bins))
    edge = [lo, np.nextafter(lo, F32(-INF)), np.nextafter(lo, F32(INF)), hi, np.nextafter(hi, F32(-INF)), np.nextafter(hi, F32(INF)),
            inner, np.nextafter(inner, F32(-INF)), np.nextafter(inner, F32(INF)), F32(np.nan), F32(INF), F32(-INF), F32(1.0)]
    rows, cols = 5, 70
    idx = (np.arange(rows * cols) * 7) % len(edge)
    x = np.array(edge, F32)[idx].reshape(rows, cols, 1)
    x = np.concatenate([hash_field(rows, cols, 1), x], 2)   # the histogram's channel is the second
    lab = blocks(rows, cols, 4, 3)
    inv_w = n_bins / (float(hi) - float(lo))
    for weights in (None, weights_for(rows)):
        want = zm.histogram(lab, 3, x[:, :, 1], n_bins, float(lo), inv_w, weights)
        assert want[:, 0].sum() > 0 and want[:, -1].sum() > 0 and want[:, 1:-1].sum() > 0
        for variant in ("runs", "plain"):
            monkeypatch.setenv("MOONRT_REGIONS_ZONAL", variant)
            for device in (False, True):
                z, h = run_zonal(rt, lab, 3, x, weights, device, (1, n_bins, float(lo), float(hi)))
                assert np.array_equal(h, want), (n_bins, variant, device)
                assert_records_equal(z, zm.zonal(lab, 3, x, SCALE, weights), "beside the histogram")


def zonal_call(rt, z, **kw):
    return lc.zonal_call(rt._lib, rt._ctx, z, **kw)


def test_heavy_weights_and_the_overflow_guard(rt, monkeypatch):
    """One region of 65536 nodes, weights near 2^32 - 1: wsum needs more than 62 bits and the guard passes; with q near 2^30
    the sum wraps, the record is still the model's modulo 2^64, and the guard raises."""
    case = rc.BY_NAME["full"]
    lab = np.zeros((256, 256), np.int32)
    w = rc.weights_for(case, heavy=True)
    i, j = np.mgrid[0:256, 0:256]
    x = (32768 - ((i * 31 + j * 17) % 16)).astype(F32)[:, :, None]
    want = zm.zonal(lab, 1, x, 1.0, w)
    exact = zm.wsum_exact(lab, 0, x[:, :, 0], 1.0, w)
    assert 2 ** 62 < exact < 2 ** 63 and want[0, 0]["wsum"] == exact and want[0, 0]["wcount"] > 2 ** 47 and want[0, 0]["max"] == 32768
    for variant in ("runs", "plain"):
        monkeypatch.setenv("MOONRT_REGIONS_ZONAL", variant)
        for device in (False, True):
            assert_records_equal(run_zonal(rt, lab, 1, x, w, device, scale=1.0), want, f"heavy weights, {variant}")
    big = (x * F32(2.0 ** 15)).astype(F32)
    want = zm.zonal(lab, 1, big, 1.0, w)
    assert zm.wsum_exact(lab, 0, big[:, :, 0], 1.0, w) >= 2 ** 63
    with pytest.raises(MoonRTError, match="lower scale"):
        run_zonal(rt, lab, 1, big, w, False, scale=1.0)
    got = np.zeros((1, 1), rg.ZONAL_DTYPE)
    z = _lib.MrtxZonalSpec(256, 256, 0, 1, 1.0, 0, 0, 0.0, 1.0, 0)
    assert zonal_call(rt, z, labels=lab, field=big, weights=w, out=got) == 0
    assert_records_equal(got, want, "a sum that wraps")
    assert_records_equal(run_zonal(rt, lab, 1, big, w, True, scale=2.0 ** -15), zm.zonal(lab, 1, big, 2.0 ** -15, w), "a lower scale")


spec = lc.zonal_spec


def test_every_refusal(rt, monkeypatch):
    labels = np.zeros((8, 9), np.int32)
    field = np.ones((8, 9), F32)
    out = np.zeros(4, rg.ZONAL_DTYPE)
    hist = np.zeros(4 * 6, np.uint64)
    dev, dev2 = DeviceBuffer(8192), DeviceBuffer(8192)
    base = dict(labels=labels, field=field, out=out, n=4)
    shape_out = np.zeros(4, rg.SHAPE_DTYPE)
    S = dict(host_labels=labels, host_out=shape_out)

    def shape_call(**kw):
        return lc.shape_call(rt._lib, rt._ctx, **kw)
    try:
        for text, kw in lc.zonal_refusals(labels, field, out, hist, dev.ptr, dev2.ptr):
            lc.refused(rt._lib, rt._ctx, zonal_call(rt, **kw), text)
            assert (out.view(np.uint8) == 0).all() and (hist == 0).all(), text
        for text, kw in lc.shape_refusals(labels, shape_out, dev.ptr):
            lc.refused(rt._lib, rt._ctx, shape_call(**kw), text)
            assert (shape_out.view(np.uint8) == 0).all(), text
        # an unknown value of the switch is refused by name, in both calls
        monkeypatch.setenv("MOONRT_REGIONS_ZONAL", "fast")
        assert zonal_call(rt, spec(), **base) == -1 and "MOONRT_REGIONS_ZONAL" in rt._lib.mrtx_last_error(rt._ctx).decode()
        assert shape_call(**S) == -1 and "MOONRT_REGIONS_ZONAL" in rt._lib.mrtx_last_error(rt._ctx).decode()
        monkeypatch.delenv("MOONRT_REGIONS_ZONAL")
        # the context still works
        lab, n, wrap = label_cases()["17x65_wrapped"]
        f = hash_field(17, 65, 3)
        assert_records_equal(run_zonal(rt, lab, n, f, None, False, wrap=wrap), zm.zonal(lab, n, f, SCALE), "after the refusals")
    finally:
        dev.free()
        dev2.free()


def test_a_bad_label_table_is_refused_after_the_launch(rt):
    labels, n, wrap = label_cases()["random_0.59_wrapped"]
    field = hash_field(*labels.shape, 1)
    out, shp = np.zeros((n, 1), rg.ZONAL_DTYPE), np.zeros(n, rg.SHAPE_DTYPE)
    z = spec(*labels.shape, 1)
    for bad in (n, n + 1000, 2 ** 31 - 1, -2, -2 ** 31):
        mine = labels.copy()
        mine[17, 23] = bad
        assert zonal_call(rt, z, labels=mine, field=field, out=out, n=n) == -1, bad
        assert "1 entries outside -1" in rt._lib.mrtx_last_error(rt._ctx).decode()
        assert rt._lib.mrtx_regions_shape(rt._ctx, *labels.shape, 1, 8, None, mine.ctypes.data, n, None, None, None, shp.ctypes.data,
                                          None) == -1, bad
        assert "1 entries outside -1" in rt._lib.mrtx_last_error(rt._ctx).decode()
        with pytest.raises(MoonRTError, match="entries outside -1"):
            run_shape(rt, mine, n, 4, wrap, True)
    # no regions: the table is checked, nothing is written
    none = np.full((5, 5), -1, np.int32)
    f = np.ones((5, 5), F32)
    got = rt.region_statistics(none, 0, f)
    assert got.shape == (0, 1) and rt.region_shapes(none, 0).shape == (0,)
    got, h = run_zonal(rt, none, 0, f[:, :, None], None, True, (0, 4, 0.0, 1.0))
    assert got.shape == (0, 1) and h.shape == (0, 6)
    one = none.copy()
    one[2, 2] = 0
    with pytest.raises(MoonRTError, match="entries outside -1"):
        rt.region_statistics(one, 0, f)
    with pytest.raises(MoonRTError, match="entries outside -1"):
        rt.region_shapes(one, 0)
    # and the context goes on
    assert_records_equal(run_zonal(rt, labels, n, field, None, False, wrap=wrap), zm.zonal(labels, n, field, SCALE), "afterwards")


def test_launches_do_not_depend_on_the_labels(rt):
    tables = [np.array(rc.answer(rc.BY_NAME["spiral"], 4)[0]), np.full((96, 96), -1, np.int32), np.zeros((96, 96), np.int32),
              blocks(96, 96, 8, 7)]
    field = hash_field(96, 96, 2)
    for hist in (None, (1, 16, -8.0, 8.0)):
        seen = []
        for lab in tables:
            st = {}
            rt.region_statistics(lab, 9, field, hist=hist, stats=st)
            assert st["launches"] > 0 and st["kernel_ms"] > 0.0
            seen.append(st["launches"])
        assert len(set(seen)) == 1, seen
    for conn in (4, 8):
        seen = []
        for lab in tables:
            st = {}
            rt.region_shapes(lab, 9, conn, stats=st)
            seen.append(st["launches"])
        assert len(set(seen)) == 1 and seen[0] > 0, seen


def test_leaves_the_render_state_alone(native_lib):
    s = named_scene("S1", 16, 16).with_size(48, 32, spp_per_launch=16)
    dem = mc.crater_dem()
    labels, n, wrap = label_cases()["17x65_wrapped"]
    field = hash_field(17, 65, 3)

    def go(with_zonal):
        r = make(s, dem, _lib.F_COUNT_STATS)
        st1 = r.render(1)
        if with_zonal:
            got, _ = run_zonal(r, labels, n, field, weights_for(17), False, (0, 7, -2.0, 5.0), wrap)
            assert_records_equal(got, zm.zonal(labels, n, field, SCALE, weights_for(17)), "between two renders")
            run_zonal(r, labels, n, field, None, True, wrap=wrap)
            assert_records_equal(run_shape(r, labels, n, 8, wrap, True), zm.shape(labels, n, 8, wrap), "between two renders")
            run_shape(r, labels, n, 4, wrap, False)
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


def test_the_catalogue_tool_with_statistics_and_shapes(native_lib, tmp_path):
    """tools/region_catalogue.py on a saved map with --stats and --shape: the new columns are the model's, and without the
    options the CSV is what it is with them, less the new columns."""
    import csv
    import os
    import subprocess
    import sys
    import regions_model as model
    rows, cols = 40, 96
    rng = np.random.default_rng(3)
    lit = rng.random((rows, cols, 2)).astype(F32)
    lit[10:30, 90:, 1] = 0.0                                 # a shadow across the seam with a lit island inside
    lit[10:30, :9, 1] = 0.0
    lit[18:21, 2:5, 1] = 1.0
    temp = (40.0 + 200.0 * rng.random((rows, cols, 3))).astype(F32)
    np.save(tmp_path / "stats.npy", lit)
    np.save(tmp_path / "temp.npy", temp)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    window = (2000, 0, rows, cols, 480, 1)
    base = [sys.executable, os.path.join(root, "tools", "region_catalogue.py"), "--map", str(tmp_path / "stats.npy"), "--channel", "1",
            "--below", "0.3", "--window", *[str(v) for v in window], "--min-area-km2", "20000", "--unit-m2", "100"]
    p = subprocess.run(base + ["--out", str(tmp_path / "l0.npy"), "--csv", str(tmp_path / "plain.csv")], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    q = subprocess.run(base + ["--out", str(tmp_path / "l1.npy"), "--csv", str(tmp_path / "full.csv"), "--stats",
                               str(tmp_path / "temp.npy") + ":2", "T", "--stats", str(tmp_path / "stats.npy"), "lit", "--shape",
                               "--side-unit-m", "0.5"], capture_output=True, text=True, timeout=120)
    assert q.returncode == 0, q.stdout + q.stderr
    with open(tmp_path / "plain.csv") as f:
        plain = list(csv.reader(f))
    with open(tmp_path / "full.csv") as f:
        full = list(csv.reader(f))
    k = len(plain[0])
    assert [r[:k] for r in full] == plain and np.array_equal(np.load(tmp_path / "l0.npy"), np.load(tmp_path / "l1.npy"))
    assert full[0][k:] == [f"{n}_{s}" for n in ("T", "lit") for s in ("min", "max", "mean", "area_mean", "min_lat", "min_lon")] + \
        ["perimeter_km", "holes"]
    assert len(full) >= 3
    labels = np.load(tmp_path / "l1.npy")
    n = int(labels.max()) + 1
    w = rg.row_weights(window, (23040, 46080), 1737400.0, 100.0)
    zt = zm.zonal(labels, n, temp[:, :, 2], 1024.0, w)[:, 0]
    ew, ns = rg.side_weights(window, (23040, 46080), 1737400.0, 0.5)
    sh = zm.shape(labels, n, 4, True, ew, ns)
    largest_has_hole = False
    for line in full[1:]:
        rec = dict(zip(full[0], line))
        r = int(rec["region"])
        assert float(rec["T_min"]) == float(zt[r]["min"]) and float(rec["T_max"]) == float(zt[r]["max"])
        assert float(rec["T_mean"]) == int(zt[r]["sum"]) / int(zt[r]["count"]) / 1024.0
        assert float(rec["T_area_mean"]) == float(zt[r]["wsum"]) / float(zt[r]["wcount"]) / 1024.0
        i, j = divmod(int(zt[r]["min_at"]), cols)
        assert float(rec["T_min_lat"]) == 90.0 - (2000 + i * 480 + 0.5) * (180.0 / 23040)
        assert float(rec["T_min_lon"]) == -180.0 + ((j * 480) % 46080 + 0.5) * (360.0 / 46080)
        assert float(rec["perimeter_km"]) == float(sh[r]["perimeter"]) * (0.5 / 1e3)
        assert int(rec["holes"]) == 1 - int(sh[r]["euler"])
        largest_has_hole |= int(rec["holes"]) >= 1
    assert largest_has_hole
    assert model.predicate(lit, 1, -INF, 0.3)[labels >= 0].all()
