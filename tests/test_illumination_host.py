"""The Sun illumination stage without a GPU: argument validation of the two C-ABI entry points, the
Sun-sample table, the grid-node convention, the float64 model's smooth-sphere known answers, and the Sun direction of an
ephemeris scene in the moon frame."""
import ctypes as C
import math
from datetime import datetime, timedelta, timezone

import numpy as np
import pytest

import illum_model as im
from moonrtx_amd import _lib
from moonrtx_amd import ephemeris as E
from moonrtx_amd.renderer import MoonRT
from moonrtx_amd.scene import named_scene

E_INVALID, E_STATE = -1, -3


@pytest.fixture
def ctx(native_lib):
    """A context handle.  Without a GPU mrtx_create stops at its first HIP call but hands the context out (the caller must
    destroy it): enough for checks that come before any HIP call."""
    c = C.c_void_p()
    rc = native_lib.mrtx_create(C.byref(_lib.MrtxConfig(0, 16, 16, 0, 1, 0, 0)), C.byref(c))
    assert rc in (0, -2) and c.value
    yield c
    native_lib.mrtx_destroy(c)


def grid(**kw):
    g = dict(lat_north=90.0, lat_south=-90.0, lon_west=-180.0, lon_east=180.0, h=18, w=36, row_begin=0, row_end=18, n_sun=16,
             reserved=0)
    g.update(kw)
    return _lib.MrtxIllumGrid(**g)


def test_grid_arguments_are_checked_before_any_device_call(native_lib, ctx):
    out = np.empty((18, 36, 4), np.float32)
    call = lambda g, dev=None, host=out.ctypes.data: native_lib.mrtx_illum_grid(ctx, C.byref(g), dev, host, None)
    assert native_lib.mrtx_illum_grid(None, C.byref(grid()), None, out.ctypes.data, None) == E_INVALID
    assert native_lib.mrtx_illum_grid(ctx, None, None, out.ctypes.data, None) == E_INVALID
    bad = [grid(h=0), grid(w=0), grid(h=-3, row_end=0),                                   # empty
           grid(lat_north=-10.0, lat_south=10.0), grid(lat_north=5.0, lat_south=5.0),     # inverted / degenerate
           grid(lon_west=30.0, lon_east=-30.0), grid(lat_north=91.0), grid(lat_south=-90.5),
           grid(lat_north=float("nan")), grid(lon_east=float("inf")),
           grid(row_begin=-1), grid(row_end=19), grid(row_begin=5, row_end=5), grid(row_begin=9, row_end=4)]   # bad bands
    bad += [grid(n_sun=n) for n in (0, -4, 3, 12, 48, 128)]
    for g in bad:
        assert call(g) == E_INVALID, (g.h, g.w, g.row_begin, g.row_end, g.n_sun, g.lat_north, g.lat_south)
        assert native_lib.mrtx_last_error(ctx)
    assert call(grid(), host=None) == E_INVALID                       # nowhere to write
    # well-formed, but the context has no DEM (nor moon frame or light): a state error, still before any device call
    assert call(grid()) == E_STATE
    assert b"displacement" in native_lib.mrtx_last_error(ctx)
    for n in (1, 2, 4, 8, 32, 64):
        assert call(grid(n_sun=n, row_begin=3, row_end=4)) == E_STATE
    # longitudes may run past +-180
    assert call(grid(lon_west=100.0, lon_east=260.0)) == E_STATE


def test_point_arguments_are_checked_before_any_device_call(native_lib, ctx):
    pts = np.array([[10.0, 20.0], [-5.0, 190.0]])
    out = np.empty((2, 4), np.float32)
    f = native_lib.mrtx_illum_points
    assert f(None, pts.ctypes.data, 2, 16, out.ctypes.data, None) == E_INVALID
    assert f(ctx, pts.ctypes.data, 0, 16, out.ctypes.data, None) == E_INVALID
    assert f(ctx, pts.ctypes.data, -1, 16, out.ctypes.data, None) == E_INVALID
    assert f(ctx, None, 2, 16, out.ctypes.data, None) == E_INVALID
    assert f(ctx, pts.ctypes.data, 2, 16, None, None) == E_INVALID
    for n in (0, 5, 65, 256):
        assert f(ctx, pts.ctypes.data, 2, n, out.ctypes.data, None) == E_INVALID
    for bad in ([[90.5, 0.0]], [[float("nan"), 0.0]], [[0.0, float("inf")]]):
        b = np.array(bad)
        assert f(ctx, b.ctypes.data, 1, 16, out.ctypes.data, None) == E_INVALID
    assert f(ctx, pts.ctypes.data, 2, 16, out.ctypes.data, None) == E_STATE


def test_sun_sample_table(native_lib):
    assert MoonRT.sun_samples(1).tolist() == [[0.0, 0.0]]                 # the Sun's centre
    for n in (2, 4, 8, 16, 32, 64):
        t = MoonRT.sun_samples(n)
        assert t.dtype == np.float32 and t.shape == (n, 2)
        i = np.arange(n)
        assert np.array_equal(t[:, 0], ((i + 0.5) / n).astype(np.float32))   # stratified in u2 (exact in float32)
        phi = i * 0.6180339887498949
        assert np.array_equal(t[:, 1], (phi - np.floor(phi)).astype(np.float32))
        assert (t >= 0).all() and (t < 1).all() and len(set(t[:, 1].tolist())) == n
        # the golden-ratio sequence is well spread in u3: every one of n equal bins holds at most two samples
        assert np.bincount((t[:, 1] * n).astype(int), minlength=n).max() <= 2
    for n in (0, 3, 128):
        with pytest.raises(ValueError):
            MoonRT.sun_samples(n)


def test_whole_moon_grid_of_the_dem_shape_lands_on_texel_centres():
    """Node (i, j) of a (h, w) whole-Moon map is the centre of cell (i, j); with the DEM's shape its texel coordinates
    (row = lat (-h / pi) + h/2 - 1/2, col = lon (w / 2 pi) + w/2 - 1/2) are (i, j)."""
    for h, w in ((180, 360), (2048, 4096), (23040, 46080)):
        la, lo = MoonRT.grid_nodes((90.0, -90.0), (-180.0, 180.0), (h, w))
        row = np.radians(la) * (-h / math.pi) + (h / 2 - 0.5)
        col = np.radians(lo) * (w / (2 * math.pi)) + (w / 2 - 0.5)
        assert np.abs(row - np.arange(h)).max() < 1e-7 * h and np.abs(col - np.arange(w)).max() < 1e-7 * w
    la, lo = MoonRT.grid_nodes((80.0, 70.0), (-30.0, 370.0), (4, 8))
    assert la.tolist() == [78.75, 76.25, 73.75, 71.25] and lo[0] == -5.0 and lo[-1] == 345.0


def _sphere_scene():
    s = named_scene("S1", 16, 16)
    s.marching_step = 0.05          # a coarse march: the model's shadow rays are cheap, and on the sphere nothing can block
    return s


def test_model_smooth_sphere_known_answers():
    """D = 1: nothing can occlude, so V = (cos > 0) for every sample; mu is the cosine of the angle to the subsolar point up to
    the light's parallax (R / distance ~ 5e-4 rad); the subsolar point sees the whole Sun and carries 2 L (1 - cos th_max)."""
    s = _sphere_scene()
    dem = np.ones((90, 180), np.float32)
    la0, lo0 = im.subsolar_latlon(s)
    lat = np.array([la0, -la0, 0.0, 30.0, la0])
    lon = np.array([lo0, lo0 + 180.0, lo0 + 89.0, lo0 - 60.0, lo0 + 90.0])
    for n in (1, 16):
        m = im.illuminate(s, dem, lat, lon, MoonRT.sun_samples(n).astype(np.float64))
        assert np.array_equal(m["V"], m["cos_pos"]) and np.array_equal(m["D"], np.ones(5))
        alt = [E.sun_altitude_at(la0, lo0, a, b) for a, b in zip(lat, lon)]
        assert np.abs(m["mu"] - np.sin(np.radians(alt))).max() < 1e-3
        assert m["lit"][0] == 1.0 and m["lit"][1] == 0.0 and m["irr"][1] == 0.0
        Lb, _ = im.sun_dir_moon_frame(s)
        sin2 = (s.light_radius / (np.linalg.norm(Lb) - s.radius - s.scene_epsilon)) ** 2    # seen from the lifted point
        # every direction of the cone is within th_max (~5e-3 rad) of the normal: cos >= 1 - 1.3e-5
        assert m["irr"][0] == pytest.approx(2 * s.light_radiance * sin2 / (1 + math.sqrt(1 - sin2)), rel=2e-5)
    # on the terminator (90 deg from the subsolar point) the Sun's disk is partly up
    m = im.illuminate(s, dem, [la0 - 90.0 if la0 > 0 else la0 + 90.0], [lo0], MoonRT.sun_samples(64).astype(np.float64))
    assert 0.0 < m["lit"][0] < 1.0


def test_scene_sun_direction_matches_the_ephemeris_subsolar_point():
    """The light of a scene built by ephemeris.scene_from_ephemeris, seen from the Moon centre in the moon frame, lies at the
    date's (subsolar_lat, subsolar_lon) -- so the maps' lat / lon are the reference's selenographic coordinates.  Measured
    over 120 dates of 2024-2025 (both view modes): at most 7.7e-4 deg.  The two sides are independent derivations -- the
    light is placed from the phase and bright-limb angles (moon_renderer.py:676-727), the subsolar point comes from the
    solar and lunar series through the body rotation -- so the bound is their series' agreement: 2e-3 deg."""
    E.init(E.Observer(-33.9, 18.4, 10))
    worst = 0.0
    for k in range(24):
        t = datetime(2024, 1, 1, tzinfo=timezone.utc) + timedelta(days=9.37 * k, hours=5 * k)
        e = E.calculate_moon_ephemeris(t, bool(k & 1))
        la, lo = im.subsolar_latlon(E.scene_from_ephemeris(e, 64, 64))
        worst = max(worst, 90.0 - E.sun_altitude_at(e.subsolar_lat, e.subsolar_lon, la, lo))
        assert abs(la - e.subsolar_lat) < 2e-3 and abs((lo - e.subsolar_lon + 180.0) % 360.0 - 180.0) < 2e-3
    assert worst < 2e-3
