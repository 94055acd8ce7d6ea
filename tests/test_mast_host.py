"""Mast-height horizons, Earth epochs and joint Sun/Earth windows without a GPU: ephemeris.earth_epochs
against the ephemeris' own sub-Earth point, the float64 model (tests/mast_model.py) at h = 0 and on the smooth sphere, the numpy
reduction of the windows on hand-made sequences, the ABI of the two entry points and their argument checks, and how
MoonRT.horizon / horizon_windows and sunlight.site_windows pass their calls."""
import ctypes as C
import math
import os
import re
from datetime import datetime, timedelta, timezone

import numpy as np
import pytest

import horizon_model as hm
import mast_model as mm
import model_cases as mc
from moonrtx_amd import _lib
from moonrtx_amd import ephemeris as E
from moonrtx_amd import renderer as rmod
from moonrtx_amd import sunlight
from moonrtx_amd.renderer import MoonRT
from moonrtx_amd.scene import MOON_RADIUS, MOON_RADIUS_KM, named_scene

E_INVALID, E_STATE = -1, -3
INF, NAN = float("inf"), float("nan")
OBS = E.Observer(52.2, 21.0, 0.0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def year(step_h, n=None):
    t0 = datetime(2025, 1, 1, tzinfo=timezone.utc)
    return [t0 + timedelta(hours=step_h * k) for k in range(n or int(365 * 24 / step_h))]


def scene():
    return named_scene("S1", 16, 16)


# ---- Earth epochs ------------------------------------------------------------------------------------------------------------
def earth_in_body(row):
    """(lat deg, lon deg, distance in scene units) of a row's light, taken into the body frame with the row's own u, v."""
    ez = row[8:11] / np.linalg.norm(row[8:11])
    v0 = row[11:14] - (row[11:14] @ ez) * ez
    v0 /= np.linalg.norm(v0)
    b = np.stack([np.cross(ez, v0), v0, ez]) @ (row[0:3] - row[5:8])
    r = float(np.linalg.norm(b))
    return math.degrees(math.asin(b[2] / r)), math.degrees(math.atan2(b[0], b[1])), r


def test_earth_epochs_point_at_the_sub_earth_point():
    times = year(73)                                            # 120 dates over the year, at every hour of the day
    ee, se = E.earth_epochs(times, OBS), E.sun_epochs(times, OBS)
    assert ee.shape == se.shape == (len(times), 14) and ee.dtype == np.float64
    assert np.array_equal(ee[:, 5:14], se[:, 5:14])            # the Sun table's Moon frame, exactly
    assert np.all(ee[:, 4] == 0.0)
    both = E.sun_earth_epochs(times, OBS)
    assert np.array_equal(both[0], se) and np.array_equal(both[1], ee)
    for t, row in zip(times, ee):
        e = E.calculate_moon_ephemeris(t, False, OBS)
        lat, lon, r = earth_in_body(row)
        assert abs(lat - e.libr_lat_geo) < 1e-9 and abs(E.wrap_signed_degrees(lon - e.libr_long_geo)) < 1e-9
        d_km = r * MOON_RADIUS_KM / MOON_RADIUS
        assert abs(d_km - E.earth_distance_km(t)) < 1e-6 and 356000.0 < d_km < 407000.0
        alpha = math.asin(row[3] / r)
        assert abs(alpha - math.asin(6378.137 / d_km)) < 1e-12
    with pytest.raises(ValueError):
        E.earth_epochs([datetime(2025, 1, 1)], OBS)


def test_earth_elevation_on_the_smooth_sphere_is_the_pinned_altitude_but_for_the_parallax():
    """The model's Earth-centre elevation at a point of the D = 1 sphere against body_altitude_at_feature of the sub-Earth
    point: they differ by the parallax of the surface point, at most asin(1737.4 / distance) (the Moon's radius seen from the
    Earth's centre); seen from the Moon's centre along the point's vertical there is none.  The bound is the parallax of the
    surface point itself, so the model is evaluated there: scene_epsilon = 0 (the lifted origin stands 1e-5 R higher, which
    adds up to 1e-5 of the bound)."""
    import dataclasses
    times = year(219, 40)
    ee = E.earth_epochs(times, OBS)
    s = dataclasses.replace(scene(), scene_epsilon=0.0)
    dem = np.ones((90, 180), np.float32)
    rng = np.random.default_rng(7)
    lat = np.concatenate([rng.uniform(-89.0, -80.0, 6), rng.uniform(80.0, 89.0, 6), rng.uniform(-60.0, 60.0, 6)])
    lon = np.concatenate([rng.uniform(-180.0, 180.0, 12), rng.uniform(-100.0, 100.0, 6)])
    e_s, _, alpha = hm.sun_position(s, dem, lat, lon, ee)
    for k, t in enumerate(times):
        e = E.calculate_moon_ephemeris(t, False, OBS)
        d_km = E.earth_distance_km(t)
        bound = math.degrees(math.asin(MOON_RADIUS_KM / d_km))
        row = ee[k]
        _, _, r = earth_in_body(row)
        for p in range(lat.size):
            pinned = float(E.body_altitude_at_feature(e.libr_lat_geo, e.libr_long_geo, lat[p], lon[p]))
            assert abs(e_s[p, k] - pinned) <= bound, (k, p, e_s[p, k], pinned, bound)
            # from the Moon's centre: the angle between the point's vertical and the Earth's direction
            la, lo = math.radians(lat[p]), math.radians(lon[p])
            u = np.array([math.cos(la) * math.sin(lo), math.cos(la) * math.cos(lo), math.sin(la)])
            elat, elon, _ = earth_in_body(row)
            b, l = math.radians(elat), math.radians(elon)
            d = np.array([math.cos(b) * math.sin(l), math.cos(b) * math.cos(l), math.sin(b)])
            assert abs(math.degrees(math.asin(float(u @ d))) - pinned) < 1e-6
        assert np.allclose(alpha[:, k], math.degrees(math.asin(6378.137 / d_km)), rtol=0, atol=bound * 0.02)
    assert (np.abs(e_s) < 5.0).any()                            # the Earth near the horizon occurs among the cases


# ---- the raised-horizon model ------------------------------------------------------------------------------------------------
def test_model_at_zero_height_is_the_horizon_model():
    s = scene()
    dem = mc.crater_dem()
    rng = np.random.default_rng(11)
    lat, lon = np.degrees(np.arcsin(rng.uniform(-0.95, 0.95, 6))), rng.uniform(-180.0, 180.0, 6)
    want = hm.horizon(s, dem, lat, lon, 16, 8)
    for h in (0.0, np.zeros(6)):
        got = mm.horizon(s, dem, lat, lon, h, 16, 8)
        for k in ("elev", "lo", "hi", "flagged"):
            assert np.array_equal(got[k], want[k]), k
        assert got["shadow_rays"] == want["shadow_rays"] and got["height_samples"] == want["height_samples"]
    # a raised point beside ground points leaves the ground points' rows as they were
    h = np.array([0.0, 50.0, 0.0, 0.0, 500.0, 0.0])
    got = mm.horizon(s, dem, lat, lon, h, 16, 8)
    assert np.array_equal(got["elev"][h == 0], want["elev"][h == 0])
    assert (got["elev"][h > 0] <= want["elev"][h > 0] + hm.bisection_step_deg(8)).all()


@pytest.mark.parametrize("h_m", [2.0, 10.0, 100.0, 1000.0])
def test_model_dip_on_the_smooth_sphere(h_m):
    """D = 1: the raised origin, at radius r0 = R + eps + hs, lies outside the bounding sphere, which is the surface.  A probe
    at elevation e < 0 passes the centre at distance c = r0 cos(e); it meets the sphere iff c <= R, i.e. e <= -acos(R / r0),
    the geometric dip.  The march starts where the probe enters and its first step lies `step` further on, so it is inside --
    and then below the surface, a hit -- iff the chord 2 sqrt(R^2 - c^2) is at least `step` long: c <= sqrt(R^2 - step^2 / 4).
    A probe whose chord is shorter is clear although it meets the sphere: what one march step can hide.  The probes are
    therefore blocked at e <= -e_hit, e_hit = acos(sqrt(R^2 - step^2 / 4) / r0), and clear at e > -e_hit up to rounding; the
    bisection returns the upper end of a bracket of one step 180 / 2^n_bis around that: -e_hit <= elev <= -e_hit + one
    bisection step, and so -dip - (e_hit - dip) <= elev <= -dip + one bisection step.  1e-9 deg covers float64 rounding
    (the bracket's float64 ends are compared, not the float32 output)."""
    s = scene()
    R, step, n_bis = float(s.radius), s.marching_step, 16
    dem = np.ones((90, 180), np.float32)
    lat, lon = np.array([0.0, 37.0, -71.0, 88.0]), np.array([0.0, 100.0, -140.0, 12.0])
    m = mm.horizon(s, dem, lat, lon, h_m, 8, n_bis)
    P, hs, _ = mm.origins(s, dem, lat, lon, h_m)
    r0 = np.sqrt((P * P).sum(-1))
    assert np.allclose(r0, R + s.scene_epsilon + hs, rtol=0, atol=1e-9) and (hs > 0).all()
    dip = np.degrees(np.arccos(R / r0))[:, None]
    e_hit = np.degrees(np.arccos(math.sqrt(R * R - 0.25 * step * step) / r0))[:, None]
    bis = hm.bisection_step_deg(n_bis)
    elev = (m["hi"] - 0.5) * 180.0                              # the bracket's upper end before its rounding to float32
    assert np.array_equal(elev.astype(np.float32), m["elev"])
    print(f"h = {h_m} m: dip {dip.ravel()[0]:.5f} deg, hidden by one step {float((e_hit - dip).max()):.2e} deg, "
          f"elev + dip in [{float((elev + dip).min()):.2e}, {float((elev + dip).max()):.2e}], bisection step {bis:.2e}")
    assert (e_hit - dip > 0).all() and (e_hit - dip < 0.01 * dip).all()
    assert (elev >= -e_hit - 1e-9).all() and (elev <= -e_hit + bis + 1e-9).all()
    assert (np.abs(elev + dip) <= bis + (e_hit - dip) + 1e-9).all()
    # every probe marches: n_bis shadow rays per (point, azimuth)
    assert m["shadow_rays"] == 4 * 8 * n_bis


def test_model_horizons_fall_with_the_height():
    s = scene()
    dem = mc.crater_dem()
    rng = np.random.default_rng(5)
    lat, lon = np.degrees(np.arcsin(rng.uniform(-0.95, 0.95, 6))), rng.uniform(-180.0, 180.0, 6)
    e0, e2, e100 = (mm.horizon(s, dem, lat, lon, h, 16, 10)["elev"] for h in (0.0, 2.0, 100.0))
    bis = hm.bisection_step_deg(10)
    assert (e100 <= e2 + bis).all() and (e2 <= e0 + bis).all() and (e100 < e0).any()


# ---- the windows' reduction --------------------------------------------------------------------------------------------------
def seq(m, ones=()):
    f = np.zeros(m, np.float32)
    for a, b in ones:
        f[a:b] = 1.0
    return f


def test_windows_reduction_on_hand_made_sequences():
    # a `both` run across the 64-epoch boundary, inside longer ok_a / ok_b runs
    fa, fb = seq(200, [(50, 90)]), seq(200, [(60, 130)])
    w, cnt = mm.windows(fa[None], fb[None], 0.5, 1.0)
    assert w[0].tolist() == [40 / 200, 110.0, 70 / 200, 70.0, 30 / 200, 30.0, 60.0, 110.0] and cnt[0].tolist() == [40, 70, 30]
    # two equally long `both` runs: the earlier one is reported
    fa = seq(150, [(10, 20), (100, 110), (130, 135)])
    w, _ = mm.windows(fa[None], np.ones((1, 150), np.float32), 0.5, 1.0)
    assert w[0, 5] == 10.0 and w[0, 6] == 10.0 and w[0, 7] == 80.0 and w[0, 3] == 0.0 and w[0, 2] == 1.0
    # none
    w, cnt = mm.windows(seq(70, [(0, 30)])[None], seq(70, [(30, 70)])[None], 0.5, 1.0)
    assert w[0, 4] == 0.0 and w[0, 5] == 0.0 and w[0, 6] == -1.0 and w[0, 7] == 70.0 and cnt[0].tolist() == [30, 40, 0]
    # m not a multiple of 64, a run reaching the last epoch
    w, _ = mm.windows(seq(100, [(90, 100)])[None], seq(100, [(0, 100)])[None], 0.5, 1.0)
    assert w[0].tolist() == [0.1, 90.0, 1.0, 0.0, 0.1, 10.0, 90.0, 90.0]
    # m = 1
    for f, want in ((1.0, [1.0, 0.0, 1.0, 0.0, 1.0, 1.0, 0.0, 0.0]), (0.0, [0.0, 1.0, 0.0, 1.0, 0.0, 0.0, -1.0, 1.0])):
        w, _ = mm.windows(np.full((1, 1), f, np.float32), np.full((1, 1), f, np.float32), 0.5, 1.0)
        assert w[0].tolist() == want
    # the thresholds: >=, compared as float32
    f = np.array([[0.5, 0.49999997, 1.0, 0.99999994]], np.float32)
    w, cnt = mm.windows(f, f, 0.5, 1.0)
    assert cnt[0].tolist() == [3, 1, 1] and w[0, 6] == 2.0
    assert mm.first_longest_run([False, True, True, False, True, True]) == (2, 1)
    assert mm.first_longest_run([]) == (0, -1) and hm.longest_run([True] * 5) == 5


# ---- ABI and argument checks -------------------------------------------------------------------------------------------------
def test_the_entry_points_are_declared_exported_and_bound(native_lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "moonrt.h")).read(), flags=re.S)
    for name in ("mrtx_horizon_raised", "mrtx_horizon_windows"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in _lib.SIGNATURES and getattr(native_lib, name) is not None
    assert native_lib.mrtx_abi_version() == 7 == _lib.ABI_VERSION
    assert "#define MRTX_ABI_VERSION 7" in re.sub(r"[ \t]+", " ", open(os.path.join(ROOT, "include", "moonrt.h")).read())


@pytest.fixture
def ctx(native_lib):
    """A context handle; without a GPU mrtx_create stops at its first HIP call but hands the context out."""
    c = C.c_void_p()
    rc = native_lib.mrtx_create(C.byref(_lib.MrtxConfig(0, 16, 16, 0, 1, 0, 0)), C.byref(c))
    assert rc in (0, -2) and c.value
    yield c
    native_lib.mrtx_destroy(c)


def test_horizon_raised_arguments_are_checked_before_any_device_call(native_lib, ctx):
    f = native_lib.mrtx_horizon_raised
    pts = np.array([[10.0, 20.0], [-5.0, 190.0], [-89.5, 0.0]])
    hts = np.array([0.0, 2.0, 1e4])
    out = np.empty((3, 8), np.float32)
    O = out.ctypes.data

    def call(p=pts, h=hts, rm=1737400.0, n=3, n_az=8, nb=6, dev=None, host=O, c=ctx):
        return f(c, None if p is None else p.ctypes.data, None if h is None else h.ctypes.data, rm, n, n_az, nb, dev, host, None)
    assert call(c=None) == E_INVALID
    for kw in (dict(p=None), dict(h=None), dict(host=None), dict(dev=O), dict(n=0), dict(n=-2), dict(n_az=0), dict(n_az=2),
               dict(n_az=12), dict(n_az=8192), dict(nb=0), dict(nb=25), dict(rm=0.0), dict(rm=-1.0), dict(rm=NAN), dict(rm=INF)):
        assert call(**kw) == E_INVALID, kw
    assert native_lib.mrtx_last_error(ctx)
    for bad in (-1.0, -1e-9, NAN, INF, -INF, 1.0001e4, 1e9):
        h = hts.copy()
        h[2] = bad
        assert call(h=h) == E_INVALID, bad
        assert b"height" in native_lib.mrtx_last_error(ctx)
    for bad in ([90.5, 0.0], [NAN, 0.0], [0.0, INF]):
        p = pts.copy()
        p[1] = bad
        assert call(p=p) == E_INVALID, bad
    # good arguments: the missing DEM is next
    for kw in (dict(), dict(h=np.zeros(3)), dict(nb=24, n_az=4096), dict(rm=1.0)):
        assert call(**kw) == E_STATE, kw
    assert b"displacement" in native_lib.mrtx_last_error(ctx)


def test_horizon_windows_arguments_are_checked_before_any_device_call(native_lib, ctx):
    f = native_lib.mrtx_horizon_windows
    pts = np.array([[10.0, 20.0], [-5.0, 190.0]])
    hz = np.zeros((2, 8), np.float32)
    times = year(24, 5)
    ea, eb = E.sun_epochs(times, OBS), E.earth_epochs(times, OBS)
    out = np.empty((2, 8), np.float32)
    O, H = out.ctypes.data, hz.ctypes.data

    def call(p=pts, n=2, n_az=8, dh=None, hh=H, a=ea, b=eb, m=5, ma=0.5, mb=1.0, dev=None, host=O, c=ctx):
        return f(c, None if p is None else p.ctypes.data, n, n_az, dh, hh, None if a is None else a.ctypes.data,
                 None if b is None else b.ctypes.data, m, ma, mb, dev, host, None)
    assert call(c=None) == E_INVALID
    for kw in (dict(p=None), dict(a=None), dict(b=None), dict(n=0), dict(m=0), dict(m=(1 << 24) + 1), dict(n_az=6),
               dict(n_az=2), dict(hh=None), dict(dh=H), dict(host=None), dict(dev=O),
               dict(ma=0.0), dict(ma=-0.1), dict(ma=1.0000001), dict(ma=NAN), dict(ma=INF), dict(ma=1e-60),
               dict(mb=0.0), dict(mb=2.0), dict(mb=NAN), dict(mb=-1.0)):
        assert call(**kw) == E_INVALID, kw
    assert native_lib.mrtx_last_error(ctx)
    bad_hz = hz.copy()
    bad_hz[1, 3] = NAN
    assert call(hh=bad_hz.ctypes.data) == E_INVALID
    bad_ep = eb.copy()
    bad_ep[2, 3] = -1.0
    assert call(b=bad_ep) == E_INVALID and call(a=bad_ep) == E_INVALID
    assert call(host=None, dev=8) == E_INVALID                  # a device output that is not 16-byte aligned
    for kw in (dict(), dict(ma=1e-6, mb=1e-6), dict(ma=1.0, mb=1.0), dict(m=1)):
        assert call(**kw) == E_STATE, kw
    assert b"displacement" in native_lib.mrtx_last_error(ctx)


# ---- the Python layer --------------------------------------------------------------------------------------------------------
class FakeBuffer:
    made = []

    def __init__(self, nbytes, device=0):
        self.nbytes, self.ptr, self.freed = int(nbytes), 1 << 20, False
        FakeBuffer.made.append(self)

    def free(self):
        self.freed = True


class FakeLib:
    def __init__(self):
        self.calls = []

    def mrtx_horizon_points(self, ctx, pts, n, n_az, n_bis, dev, host, st):
        self.calls.append(("points", n, n_az, n_bis, dev is not None))
        st._obj.launches = 1
        return 0

    def mrtx_horizon_raised(self, ctx, pts, hts, radius_m, n, n_az, n_bis, dev, host, st):
        h = np.ctypeslib.as_array(C.cast(hts, C.POINTER(C.c_double)), (n,)).copy()
        self.calls.append(("raised", n, n_az, n_bis, dev is not None, h.tolist(), radius_m))
        st._obj.launches = 1
        return 0

    def mrtx_horizon_windows(self, ctx, pts, n, n_az, dh, hh, ea, eb, m, ma, mb, dev, host, st):
        self.calls.append(("windows", n, n_az, m, ma, mb, dh is not None, hh is not None))
        vals = np.tile(np.array([0.5, 3, 0.25, 4, 0.125, 6, 7, 9], np.float32), (n, 1))
        C.memmove(host, vals.ctypes.data, vals.nbytes)
        st._obj.launches = 1
        return 0

    def mrtx_get_config(self, ctx, cfg):
        return 0


def fake_rt(monkeypatch):
    FakeBuffer.made.clear()
    monkeypatch.setattr(rmod, "DeviceBuffer", FakeBuffer)
    rt = MoonRT.__new__(MoonRT)
    rt._lib = FakeLib()
    rt._ctx = None
    return rt


def test_horizon_takes_heights(monkeypatch):
    rt = fake_rt(monkeypatch)
    la, lo = np.linspace(-5, 5, 5), np.linspace(0, 4, 5)
    rt.horizon(la, lo, n_az=8, n_bis=5)
    rt.horizon(la, lo, n_az=8, n_bis=5, height_m=None)
    assert rt._lib.calls == [("points", 5, 8, 5, False)] * 2
    rt._lib.calls.clear()
    rt.horizon(la, lo, n_az=8, n_bis=5, height_m=10)
    rt.horizon(la, lo, n_az=8, n_bis=5, height_m=np.arange(5.0), radius_m=1.5e6, chunk_bytes=2 * 8 * 4)
    assert rt._lib.calls[0] == ("raised", 5, 8, 5, False, [10.0] * 5, 1737400.0)
    assert [c[1] for c in rt._lib.calls[1:]] == [2, 2, 1] and [c[5] for c in rt._lib.calls[1:]] == [[0.0, 1.0], [2.0, 3.0], [4.0]]
    assert all(c[6] == 1.5e6 for c in rt._lib.calls[1:])
    with pytest.raises(ValueError):
        rt.horizon(la, lo, height_m=np.zeros(4))


def test_horizon_windows_chunks(monkeypatch):
    rt = fake_rt(monkeypatch)
    la, lo = np.linspace(-5, 5, 5), np.linspace(0, 4, 5)
    times = year(24, 3)
    ea, eb = E.sun_epochs(times, OBS), E.earth_epochs(times, OBS)
    hz = np.zeros((5, 8), np.float32)
    st = {}
    got = rt.horizon_windows(la, lo, hz, ea, eb, min_a=0.25, min_b=0.75, stats=st, chunk_bytes=2 * (8 + 8) * 4)
    assert got.shape == (5, 8) and got.dtype == np.float32 and got[4].tolist() == [0.5, 3, 0.25, 4, 0.125, 6, 7, 9]
    assert rt._lib.calls == [("windows", n, 8, 3, 0.25, 0.75, False, True) for n in (2, 2, 1)] and st["launches"] == 3
    assert len(MoonRT.WINDOW_COLUMNS) == 8
    rt._lib.calls.clear()
    rt.horizon_windows(la, lo, FakeBuffer(5 * 8 * 4), ea, eb, n_az=8)
    assert rt._lib.calls == [("windows", 5, 8, 3, 0.5, 1.0, True, False)]
    with pytest.raises(ValueError):
        rt.horizon_windows(la, lo, hz, ea, eb[:2])
    with pytest.raises(ValueError):
        rt.horizon_windows(la, lo, FakeBuffer(5 * 8 * 4), ea, eb)


def test_site_windows_streams_chunks(monkeypatch):
    rt = fake_rt(monkeypatch)
    la, lo = np.linspace(-88, -84, 5), np.linspace(0, 4, 5)
    t0 = datetime(2025, 1, 1, tzinfo=timezone.utc)
    r = sunlight.site_windows(rt, la, lo, t0, 0.25, step_min=30, height_m=10.0, n_az=8, n_bis=5, observer=OBS, chunk=2)
    assert len(r.times) == 12 and r.times[1] - r.times[0] == timedelta(minutes=30)
    kinds = [c[0] for c in rt._lib.calls]
    assert kinds == ["raised", "windows"] * 3 and [c[1] for c in rt._lib.calls] == [2, 2, 2, 2, 1, 1]
    assert all(c[5] == [10.0] * c[1] for c in rt._lib.calls if c[0] == "raised")
    assert all(c[3:] == (12, 0.5, 1.0, True, False) for c in rt._lib.calls if c[0] == "windows")
    assert len(FakeBuffer.made) == 1 and FakeBuffer.made[0].freed and FakeBuffer.made[0].nbytes == 2 * 8 * 4
    # runs in hours, the start as an index into times
    assert r.sun_share.tolist() == [0.5] * 5 and r.longest_no_sun_h.tolist() == [1.5] * 5
    assert r.longest_both_h.tolist() == [3.0] * 5 and r.best_start.tolist() == [7] * 5 and r.best_start.dtype == np.int64
    assert r.longest_outage_h.tolist() == [4.5] * 5 and r.stats["launches"] == 6
    # illumination_statistics: the old call without a height, the raised one with
    rt._lib.calls.clear()
    monkeypatch.setattr(MoonRT, "horizon_sun", lambda self, la, lo, hz, ep, **kw: np.zeros((len(la), 4), np.float32))
    sunlight.illumination_statistics(rt, la, lo, t0, 0.25, step_min=30, n_az=8, n_bis=5, observer=OBS)
    sunlight.illumination_statistics(rt, la, lo, t0, 0.25, step_min=30, n_az=8, n_bis=5, observer=OBS, height_m=2.0,
                                     radius_m=1.7e6)
    assert [c[0] for c in rt._lib.calls] == ["points", "raised"] and rt._lib.calls[1][5:] == ([2.0] * 5, 1.7e6)
