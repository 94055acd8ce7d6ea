"""Terrain horizons and the Sun against them without a GPU (DESIGN.md sections 3.8 and 3.9): argument validation of
mrtx_horizon_points / mrtx_horizon_sun, MoonRT.horizon_azimuths, and the float64 model's known answers."""
import ctypes as C
import math
from datetime import datetime, timezone

import numpy as np
import pytest

import horizon_model as hm
from moonrtx_amd import _lib
from moonrtx_amd import ephemeris as E
from moonrtx_amd.renderer import MoonRT
from moonrtx_amd.scene import named_scene
from test_gpu_illumination import plateau_dem

E_INVALID, E_STATE = -1, -3


@pytest.fixture
def ctx(native_lib):
    """A context handle; without a GPU mrtx_create stops at its first HIP call but hands the context out."""
    c = C.c_void_p()
    rc = native_lib.mrtx_create(C.byref(_lib.MrtxConfig(0, 16, 16, 0, 1, 0, 0)), C.byref(c))
    assert rc in (0, -2) and c.value
    yield c
    native_lib.mrtx_destroy(c)


def good_epochs(m=3):
    s = E.scene_from_ephemeris(E.calculate_moon_ephemeris(datetime(2025, 3, 7, 21, 0, tzinfo=timezone.utc), False,
                                                          E.Observer(52.2, 21.0, 0.0)), 16, 16)
    return np.ascontiguousarray(np.stack([E.epoch_of_scene(s)] * m))


PTS = np.array([[10.0, 20.0], [-5.0, 190.0], [-89.5, 0.0]])


def test_horizon_points_arguments_are_checked_before_any_device_call(native_lib, ctx):
    f = native_lib.mrtx_horizon_points
    out = np.empty((3, 64), np.float32)
    O = out.ctypes.data

    def call(p=PTS, n=3, n_az=64, n_bis=10, dev=None, host=O, c=ctx):
        return f(c, None if p is None else p.ctypes.data, n, n_az, n_bis, dev, host, None)
    assert call(c=None) == E_INVALID
    assert call(p=None) == E_INVALID
    assert call(host=None) == E_INVALID                      # neither output
    assert call(dev=O) == E_INVALID                          # both outputs
    assert native_lib.mrtx_last_error(ctx)
    for n in (0, -1):
        assert call(n=n) == E_INVALID, n
    for n_az in (0, 1, 2, 3, 6, 100, 8192, -64):
        assert call(n_az=n_az) == E_INVALID, n_az
    for n_bis in (0, -1, 25, 100):
        assert call(n_bis=n_bis) == E_INVALID, n_bis
    assert call(n=(1 << 20) + 1, n_az=4096) == E_INVALID     # more than 2^31 outputs (checked before the points are read)
    for bad in ([90.5, 0.0], [-91.0, 0.0], [float("nan"), 0.0], [0.0, float("inf")], [0.0, 2e6]):
        p = PTS.copy()
        p[1] = bad
        assert call(p=p) == E_INVALID, bad
    # every argument good: the missing DEM is next
    for n_az, n_bis in ((4, 1), (64, 10), (4096, 24)):
        assert call(n_az=n_az, n_bis=n_bis) == E_STATE
    assert b"displacement" in native_lib.mrtx_last_error(ctx)


def test_horizon_sun_arguments_are_checked_before_any_device_call(native_lib, ctx):
    f = native_lib.mrtx_horizon_sun
    hz = np.zeros((3, 16), np.float32)
    ep = good_epochs(3)
    out = np.empty((3, 4), np.float32)
    O, H = out.ctypes.data, hz.ctypes.data

    def call(p=PTS, n=3, n_az=16, dh=None, hh=H, e=None, m=3, mode=1, dev=None, host=O, c=ctx):
        e = ep if e is None else e
        return f(c, None if p is None else p.ctypes.data, n, n_az, dh, hh, None if e is False else e.ctypes.data, m, mode, dev,
                 host, None)
    assert call(c=None) == E_INVALID
    assert call(p=None) == E_INVALID
    assert call(e=False) == E_INVALID
    assert call(hh=None) == E_INVALID                       # no horizons
    assert call(dh=H) == E_INVALID                          # both
    assert call(host=None) == E_INVALID
    assert call(dev=O) == E_INVALID
    for kw in (dict(n=0), dict(n=-2), dict(m=0), dict(m=-1), dict(mode=2), dict(mode=-1), dict(n_az=2), dict(n_az=12),
               dict(n_az=8192)):
        assert call(**kw) == E_INVALID, kw
    assert call(mode=0, n=200, m=(1 << 24)) == E_INVALID    # FULL: more than 2^31 outputs (checked before anything is read)
    assert call(m=(1 << 24) + 1) == E_INVALID               # more epochs than the dark run counts exactly
    for bad in (float("nan"), float("inf"), 90.5, -91.0):
        h2 = hz.copy()
        h2[2, 5] = bad
        assert call(hh=h2.ctypes.data) == E_INVALID, bad
    p = PTS.copy()
    p[0] = [0.0, float("nan")]
    assert call(p=p) == E_INVALID
    for i, x in ((0, float("nan")), (3, -1.0), (4, float("inf")), (8, float("nan"))):
        e = ep.copy()
        e[1, i] = x
        assert call(e=e) == E_INVALID, (i, x)
    e = ep.copy()
    e[2, 11:14] = e[2, 8:11]                                # u parallel to v
    assert call(e=e) == E_INVALID
    # good arguments: the missing DEM, in both modes and with either horizon source
    out_full = np.empty((3, 3), np.float32)
    assert call(mode=0, host=out_full.ctypes.data) == E_STATE
    assert call(mode=1) == E_STATE
    assert call(hh=None, dh=H) == E_STATE


def test_horizon_azimuths():
    az = MoonRT.horizon_azimuths(8)
    assert az.dtype == np.float64 and list(az) == [0.0, 45.0, 90.0, 135.0, 180.0, 225.0, 270.0, 315.0]
    big = MoonRT.horizon_azimuths(4096)
    assert big.shape == (4096,) and big[1] == 360.0 / 4096 and big[-1] < 360.0
    # nesting: azimuth 2a at 2 n_az is azimuth a at n_az
    assert np.array_equal(MoonRT.horizon_azimuths(512)[::2], MoonRT.horizon_azimuths(256))
    for bad in (0, 2, 3, 6, 8192):
        with pytest.raises(ValueError):
            MoonRT.horizon_azimuths(bad)


def test_model_on_a_smooth_sphere():
    """D constant: n = U, so every probe above the horizontal escapes and every probe below it is refused by n . d > 0; the
    first probe lies on the horizontal and goes either way: the output is 0 or 180 * 2^-n_bis everywhere."""
    s = named_scene("S1", 16, 16)
    dem = np.ones((90, 180), np.float32)
    lat = np.array([0.0, 35.0, -60.0, 85.0])
    lon = np.array([0.0, 100.0, -150.0, 30.0])
    for n_bis in (1, 6, 12):
        m = hm.horizon(s, dem, lat, lon, 16, n_bis)
        assert set(np.unique(m["elev"]).tolist()) <= {0.0, np.float32(hm.bisection_step_deg(n_bis))}, n_bis
        # the two brackets that can come out: [1/2, 1/2 + 2^-n] or [1/2 - 2^-n, 1/2]
        assert np.all(m["hi"] - m["lo"] == 2.0 ** -n_bis)


def test_model_behind_a_plateau():
    """A 10 km plateau west of lon 0 on the equator: looking west (azimuth 270) from a point 1 deg east of its edge, the
    horizon is the plateau's top edge at lon 0 seen from the lifted origin; other directions see the open sphere."""
    s = named_scene("S1", 16, 16)
    h, w, H_km = 720, 1440, 10.0
    dem = plateau_dem(h, w, -20.0, 0.0, 30.0, H_km)
    R = s.radius
    D0 = float(dem.min())
    n_bis = 14
    lon0 = 1.0
    m = hm.horizon(s, dem, [0.0], [lon0], 16, n_bis)
    o, _, _, _, _ = hm.frame(s, dem, [0.0], [lon0])
    edge = np.array([0.0, R, 0.0])                          # (lat 0, lon 0) at the top radius
    want = hm.elevation_of(o[0], edge)
    # tolerance: one texel of the bilinear edge ramp and one march step, seen from the point's distance to the edge, and one
    # bisection step
    dist = float(np.linalg.norm(edge - o[0]))
    tol = math.degrees((R * math.radians(360.0 / w) + s.marching_step) / dist) + hm.bisection_step_deg(n_bis)
    west = m["elev"][0, 12]                                 # azimuth 12 / 16 turn = 270 deg
    assert 5.0 < want < 40.0
    assert abs(west - want) <= tol, (west, want, tol)
    # east, north and south: no relief within the march's reach
    for a in (0, 4, 8):
        assert abs(m["elev"][0, a]) <= hm.bisection_step_deg(n_bis), (a, m["elev"][0, a])
    assert R * D0 < R


def test_disc_fraction():
    f = hm.disc_fraction
    assert f(0.0, 0.0, 1.0) == pytest.approx(0.5, abs=1e-15)                 # x = 0: half the disc
    assert f(-1.0, 0.0, 1.0) == 1.0 and f(-5.0, 0.0, 1.0) == 1.0            # x <= -1: all of it
    assert f(1.0, 0.0, 1.0) == 0.0 and f(3.0, 0.0, 1.0) == 0.0              # x >= 1: none
    x = np.linspace(-0.99, 0.99, 41)
    assert np.allclose(f(x, 0.0, 1.0) + f(-x, 0.0, 1.0), 1.0, atol=1e-14)  # symmetry
    assert np.all(np.diff(f(x, 0.0, 1.0)) < 0)                              # the higher the horizon, the less disc
    assert f(0.2, 0.3, 0.0) == 1.0 and f(0.3, 0.2, 0.0) == 0.0 and f(0.2, 0.2, 0.0) == 0.0   # a point light
    # the segment area of a unit circle cut at distance x from its centre
    xv = 0.3
    seg = math.acos(xv) - xv * math.sqrt(1 - xv * xv)
    assert f(xv, 0.0, 1.0) == pytest.approx(seg / math.pi, rel=1e-14)


def test_run_length_reduction():
    lr = hm.longest_run
    assert lr([]) == 0 and lr([False] * 5) == 0 and lr([True] * 7) == 7
    assert lr([1, 1, 0, 1, 1, 1, 0, 1]) == 3
    assert lr([0, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1]) == 5          # the run at the end
    assert lr([1, 1, 1, 1, 0, 1, 1]) == 4                       # the run at the start
    f = np.array([[0.0, 0.0, 0.5, 1.0, 0.0, 0.0, 0.0, 0.2],
                  [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0],
                  [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]])
    s = hm.summarize(f)
    assert s[0].tolist() == [pytest.approx(1.7 / 8), 3 / 8, 1 / 8, 3]
    assert s[1].tolist() == [1.0, 1.0, 1.0, 0]
    assert s[2].tolist() == [0.0, 0.0, 0.0, 8]
    # across the 64-epoch chunks the kernel walks: a run spanning chunk boundaries counts whole
    g = np.ones((1, 200))
    g[0, 50:150] = 0.0
    assert hm.summarize(g)[0, 3] == 100
