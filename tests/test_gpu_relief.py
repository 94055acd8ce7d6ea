"""Terrain relief on the MI355X (DESIGN.md sections 3.14 and 4.15): relief maps bit-equal to the float64 model
(tests/relief_model.py) in every node -- relief, craters, the bowl, strides, the seam, the DEM's first and last rows, every
footprint class, host and device outputs, every tile shape, repeats; the safe share equal to its model; the counter; the render
state left alone; the full-size DEM; and a traverse kept off steep ground by the slope penalty."""
import ctypes as C
import math

import numpy as np
import pytest

import model_cases as mc
import relief_model as rm
import synth_np
from bowl_dem import bowl_dem
from common import assert_bit_equal
from moonrtx_amd import _lib
from moonrtx_amd import traverse as tv
from moonrtx_amd.renderer import DeviceBuffer, MoonRT, MoonRTError, synth_ldem, dem_from_ldem
from moonrtx_amd.scene import named_scene
from test_gpu_illumination import make

pytestmark = pytest.mark.gpu

RM = 1737400.0
INF = float("inf")
TILES = ("0", "16", "32", "64")


def ctx(dem, flags=None):
    rt = MoonRT(16, 16)
    if flags is not None:
        rt.set_params(flags=flags)
    rt.upload_dem(dem)
    return rt


def gpu_relief(rt, t, stats=None):
    """mrtx_relief straight through the ABI, host pointer."""
    out = np.empty((t.rows, t.cols, 4), np.float32)
    st = _lib.MrtxStats()
    rt._check(rt._lib.mrtx_relief(rt._ctx, C.byref(t), None, out.ctypes.data, C.byref(st)), "mrtx_relief")
    if stats is not None:
        stats.update(launches=st.launches, kernel_ms=st.kernel_ms, dem_fetches=st.dem_fetches)
    return out


def assert_table_equal(got, want, what):
    a, b = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    if not np.array_equal(a, b):
        bad = np.argwhere(a != b)
        raise AssertionError(f"{what}: {len(bad)} of {a.size} values differ bitwise, first at {tuple(bad[0])}: "
                             f"{got[tuple(bad[0])]!r} vs {want[tuple(bad[0])]!r}")


def bowl():
    return bowl_dem(360, 720, lat0_deg=-30.0, lon0_deg=40.0, theta_c_deg=6.0, d_over_D=0.2)


def synth():
    return synth_np.dem(180, 360, seed=7, craters=40)


CASES = {
    # name: (dem, window)
    "synth": (synth, rm.make_window(30, 100, 70, 90, ri=2, rj=2)),
    "craters-stride3": (mc.crater_dem, rm.make_window(10, 300, 100, 120, stride=3, ri=3, rj=4)),
    "bowl": (bowl, rm.make_window(200, 400, 80, 80, ri=5, rj=5)),
    "seam": (synth, rm.make_window(40, 340, 50, 45, ri=2, rj=6)),                    # columns 340 .. 384 of 360
    "first-and-last-rows": (synth, rm.make_window(0, 7, 180, 33, ri=6, rj=3)),       # the NaN rows at both ends
    "last-row-stride3": (synth, rm.make_window(2, 350, 60, 40, stride=3, ri=2, rj=1)),
    "ri-not-rj": (mc.crater_dem, rm.make_window(100, 200, 45, 70, ri=9, rj=2)),
    "wide-not-tall": (mc.crater_dem, rm.make_window(100, 700, 40, 50, ri=1, rj=17)),
    "1x1": (synth, rm.make_window(1, 0, 178, 360, ri=1, rj=1)),                      # the whole circle of columns
    "32x32": (mc.crater_dem, rm.make_window(20, 690, 70, 75, ri=32, rj=32)),         # NaN rows on top, over the seam
    "32x32-stride3": (mc.crater_dem, rm.make_window(90, 0, 40, 38, stride=3, ri=32, rj=32)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_relief_matches_the_model_in_every_node(native_lib, name, monkeypatch):
    mk, t = CASES[name]
    dem = mk()
    want = rm.relief(dem, t)
    assert np.isfinite(want).any()
    rt = ctx(dem, _lib.F_COUNT_STATS)
    monkeypatch.delenv("MOONRT_RELIEF_TILE", raising=False)
    st = {}
    got = gpu_relief(rt, t, st)
    print(f"{name}: {t.rows} x {t.cols}, footprint ({t.ri}, {t.rj}), {st['kernel_ms']:.3f} ms")
    assert_table_equal(got, want, name)
    assert st["launches"] == 1 and st["dem_fetches"] == rm.fetches(t, dem.shape[0])
    for tile in TILES:                                      # every tile shape, twice: the same bits
        monkeypatch.setenv("MOONRT_RELIEF_TILE", tile)
        for _ in range(2):
            st = {}
            assert_table_equal(gpu_relief(rt, t, st), want, f"{name}, tile {tile}")
            assert st["dem_fetches"] == rm.fetches(t, dem.shape[0])
    monkeypatch.setenv("MOONRT_RELIEF_TILE", "12")
    with pytest.raises(MoonRTError):
        gpu_relief(rt, t)
    rt.close()


def test_device_output_and_the_windows_dem_checks(native_lib):
    dem = synth()
    t = rm.make_window(30, 100, 77, 133, ri=3, rj=2)
    want = rm.relief(dem, t)
    rt = ctx(dem, 0)                                        # production flags: no counters
    buf = DeviceBuffer(16 * t.rows * t.cols)
    st = _lib.MrtxStats()
    rc = rt._lib.mrtx_relief(rt._ctx, C.byref(t), buf.ptr, None, C.byref(st))
    assert rc == 0, rt._lib.mrtx_last_error(rt._ctx)
    assert_table_equal(buf.download(np.float32, (t.rows, t.cols, 4)), want, "device output")
    assert st.dem_fetches == 0 and st.launches == 1 and st.kernel_ms > 0.0
    buf.free()
    # the checks that need the DEM's shape
    for kw in (dict(row0=175), dict(col0=360), dict(cols=361), dict(stride=60, rows=2, cols=4, rj=3)):
        bad = rm.make_window(**{**dict(row0=20, col0=40, rows=10, cols=10, ri=2, rj=2), **kw})
        with pytest.raises(MoonRTError):
            gpu_relief(rt, bad)
    assert_table_equal(gpu_relief(rt, t), want, "after refusals")
    # a node's bits do not depend on the window it is computed in
    part = gpu_relief(rt, rm.make_window(30 + 11, 100 + 5, 20, 30, ri=3, rj=2))
    assert_table_equal(part, want[11:31, 5:35], "a window inside the window")
    rt.close()


def gpu_share(rt, table, Ri, Rj, wrap, gmax, smax, device=False):
    table = np.ascontiguousarray(table, np.float32)
    rows, cols = table.shape[:2]
    s = _lib.MrtxReliefShare(rows, cols, Ri, Rj, wrap, 0, gmax, smax)
    st = _lib.MrtxStats()
    if device:
        tb, ob = DeviceBuffer(table.nbytes), DeviceBuffer(4 * rows * cols)
        tb.upload(table)
        rc = rt._lib.mrtx_relief_share(rt._ctx, C.byref(s), tb.ptr, None, ob.ptr, None, C.byref(st))
        assert rc == 0, rt._lib.mrtx_last_error(rt._ctx)
        out = ob.download(np.float32, (rows, cols))
        tb.free(); ob.free()
    else:
        out = np.empty((rows, cols), np.float32)
        rt._check(rt._lib.mrtx_relief_share(rt._ctx, C.byref(s), None, table.ctypes.data, None, out.ctypes.data, C.byref(st)),
                  "mrtx_relief_share")
    assert st.launches == 3
    return out


def test_share_equals_its_model(native_lib):
    dem = mc.crater_dem()
    rt = ctx(dem)
    t = rm.make_window(0, 0, 120, 720, ri=3, rj=3)          # the whole circle, NaN rows on top
    table = gpu_relief(rt, t)
    assert np.isnan(table[:3]).all()
    g50, s50 = float(np.nanmedian(table[..., 0])), float(np.nanmedian(table[..., 1]))
    for device in (False, True):
        for Ri, Rj, wrap in ((0, 0, 0), (4, 7, 0), (4, 7, 1), (60, 3, 1), (2, 400, 1), (2, 400, 0), (119, 1024, 0), (1024, 300, 1)):
            got = gpu_share(rt, table, Ri, Rj, wrap, g50, s50, device)
            assert_bit_equal(got, rm.share(table, Ri, Rj, wrap, g50, s50), f"share {Ri} {Rj} {wrap} device={device}")
        everything = gpu_share(rt, table, 5, 5, 1, INF, INF, device)
        assert_bit_equal(everything, rm.share(table, 5, 5, 1, INF, INF), "everything safe")
        assert (everything[20:] == 1.0).all() and (everything[0] < 1.0).all()          # but for the NaN rows
        assert (gpu_share(rt, table, 5, 5, 1, 0.0, 0.0, device) == 0.0).all()          # nothing safe
    # a small odd-shaped map with NaNs sprinkled in, against the brute-force count
    rng = np.random.default_rng(2)
    small = rng.uniform(0.0, 1.0, (23, 301, 4)).astype(np.float32)
    small[rng.random((23, 301)) < 0.1] = np.nan
    for Ri, Rj, wrap in ((1, 2, 1), (3, 200, 1), (30, 1, 0)):
        got = gpu_share(rt, small, Ri, Rj, wrap, 0.5, 0.8)
        assert_bit_equal(got, rm.share(small, Ri, Rj, wrap, 0.5, 0.8), f"small {Ri} {Rj} {wrap}")
    assert_bit_equal(gpu_share(rt, small[:9, :40], 2, 3, 1, 0.5, 0.8), rm.share_brute(small[:9, :40], 2, 3, 1, 0.5, 0.8), "brute")
    # the wrapper
    m = rt.relief((0, 0, 120, 720), footprint_nodes=(3, 3))
    assert_table_equal(m.table, table, "MoonRT.relief")
    assert m.closes_circle
    deg = math.degrees(math.atan(g50))
    got = rt.landing_share(m, deg, s50, ellipse_nodes=(4, 7))
    assert_bit_equal(got, rm.share(table, 4, 7, 1, math.tan(math.radians(deg)), s50), "MoonRT.landing_share")
    rt.close()


def test_share_needs_no_dem(native_lib):
    rt = MoonRT(16, 16)
    table = np.zeros((5, 7, 4), np.float32)
    assert (gpu_share(rt, table, 1, 1, 0, 1.0, 1.0) == 1.0).all()
    rt.close()


def test_leaves_the_render_state_alone(native_lib):
    s = named_scene("S1", 16, 16).with_size(48, 32, spp_per_launch=16)
    dem = mc.crater_dem()

    def run(with_relief):
        rt = make(s, dem, _lib.F_COUNT_STATS)
        st1 = rt.render(1)
        if with_relief:
            m = rt.relief((100, 100, 40, 50), footprint_nodes=(2, 3))
            rt.landing_share(m, 10.0, 50.0, ellipse_nodes=(3, 3))
        st2 = rt.render(1)
        out = rt.read_linear(), rt.read_hits(), rt.samples_done(), st1, st2
        rt.close()
        return out
    a, b = run(False), run(True)
    assert_bit_equal(b[0], a[0], "linear radiance")
    assert_bit_equal(b[1], a[1], "hit buffer")
    assert b[2] == a[2] == 32
    for k in ("primary_hits", "shadow_rays", "height_samples", "bounce_rays"):
        assert b[4][k] == a[4][k], k


def download_rows(buf, r0, n, W):
    """Rows [r0, r0 + n) of a device-resident (H, W) float32 DEM."""
    out = np.empty((n, W), np.float32)
    rc = buf._lib.mrtx_dev_download(buf.device, out.ctypes.data, buf.ptr + r0 * W * 4, out.nbytes)
    assert rc == 0
    return out


def test_full_size(native_lib):
    """The headline DEM (23040 x 46080; its padded row-pair copy passes 4 GiB at row ~11650: 64-bit texel offsets): a window
    beyond that offset and a window over the seam against the model on crops, and a banded footprint in metres near the pole
    against per-band model calls."""
    DEM_H, DEM_W = 23040, 46080
    src = synth_ldem(DEM_H, DEM_W)
    dem, scale = dem_from_ldem(src, DEM_H, DEM_W, 1)
    src.free()
    rt = MoonRT(16, 16)
    rt.bind_dem(dem, DEM_H, DEM_W)
    R = RM * scale
    for name, t in (("beyond 4 GiB", rm.make_window(19000, 30000, 300, 400, ri=4, rj=4, radius_m=R)),
                    ("beyond 4 GiB, 32 x 32, stride 2", rm.make_window(21000, 100, 96, 80, stride=2, ri=32, rj=32, radius_m=R)),
                    ("over the seam", rm.make_window(12000, DEM_W - 150, 200, 300, ri=3, rj=8, radius_m=R)),
                    ("last rows", rm.make_window(DEM_H - 40, 5, 40, 100, ri=5, rj=2, radius_m=R))):
        r0 = max(t.row0 - t.ri * t.stride, 0)
        r1 = min(t.row0 + (t.rows - 1 + t.ri) * t.stride + 1, DEM_H)
        crop = download_rows(dem, r0, r1 - r0, DEM_W)
        st = {}
        got = gpu_relief(rt, t, st)
        print(f"full size, {name}: {st['kernel_ms']:.3f} ms")
        assert_table_equal(got, rm.relief_crop(crop, r0, (DEM_H, DEM_W), t), name)
    # a 300 m footprint on a polar window: rj changes from band to band
    window = (300, 46000, 500, 120, 1)                      # over the seam as well
    m = rt.relief(window, footprint_m=300.0, radius_m=R)
    assert len(m.bands) >= 3 and m.bands[0][2] > m.bands[-1][2]
    r0 = 300 - m.ri
    crop = download_rows(dem, r0, 500 + 2 * m.ri, DEM_W)
    for a, n, rj in m.bands:
        t = rm.make_window(300 + a, 46000, n, 120, ri=m.ri, rj=rj, radius_m=R)
        assert_table_equal(m.table[a:a + n], rm.relief_crop(crop, r0, (DEM_H, DEM_W), t), f"band at row {a}, rj {rj}")
    assert np.isfinite(m.slope_deg).all()
    rt.close()
    dem.free()


def test_slope_penalty_keeps_a_route_off_steep_ground(native_lib):
    dem = bowl()
    rt = ctx(dem)
    window = (200, 400, 80, 80)
    m = rt.relief(window, footprint_nodes=(2, 2))
    limit = 12.0                                             # degrees, at the footprint's scale
    steep = m.grade.astype(np.float64) > tv.max_slope_grade(limit)
    assert 0.02 < steep.mean() < 0.6                        # the bowl's wall is steep, its floor and the plain are not
    # across the bowl: from the plain west of it to the plain east of it, through the rows of its centre
    src, goal = (40, 2), (40, 77)
    assert not steep[src] and not steep[goal]
    plain = rt.traverse(window, nodes=np.array([src]), max_slope_deg=89.0, climb_cost=0.0)
    r0 = tv.route(plain, goal)
    assert steep[r0["i"], r0["j"]].any()                    # the straight way crosses the wall
    P = tv.penalty_from_slope(m, limit)
    assert np.array_equal(np.isinf(P), steep)
    kept = rt.traverse(window, nodes=np.array([src]), penalty=P, max_slope_deg=89.0, climb_cost=0.0)
    r1 = tv.route(kept, goal)
    assert not steep[r1["i"], r1["j"]].any() and (m.slope_deg[r1["i"], r1["j"]] <= limit + 1e-9).all()
    assert r1["length_m"][-1] > r0["length_m"][-1]
    rt.close()
