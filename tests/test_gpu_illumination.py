"""The Sun illumination stage on the MI355X (DESIGN.md sections 3.6 and 4.8): smooth-sphere and shadow-length known answers,
the float64 model (tests/illum_model.py) on cratered relief, bit-identical invariances, no side effect on the render state,
the full-size DEM and the TkOptiX facade."""
import math
from datetime import datetime, timezone

import numpy as np
import pytest

import illum_model as im
import model_cases as mc
import synth_np
from common import assert_bit_equal
from moonrtx_amd import _lib
from moonrtx_amd import ephemeris as E
from moonrtx_amd.renderer import MoonRT, synth_ldem, dem_from_ldem
from moonrtx_amd.scene import named_scene

pytestmark = pytest.mark.gpu


def mu_tol(shape, lat_deg):
    """How far the spec's float32 normal may lie from the float64 model's, per node: the normal comes from central differences
    of D one texel either side (hit_vertex), so one ulp of D (2^-24) tilts it by 2^-24 h / 2 pi (latitude) or
    2^-24 w / (4 pi cos lat) radians (longitude: the gradient is divided by rho = R cos lat); eight such ulps (two bilinear
    evaluations of four rounded terms), plus 1e-5 for the rest of the chain.  On the 360 x 720 crater DEM: 3.7e-5 at the
    equator, 1.7e-3 0.94 deg from the pole (measured there: 1.4e-4); 1.9e-3 at 23040 rows, lat 20 (measured: 7.6e-4)."""
    c = np.maximum(np.cos(np.radians(np.asarray(lat_deg, float))), 1e-3)
    return 1e-5 + 8 * 2.0 ** -24 * np.maximum(shape[0] / (2 * math.pi), shape[1] / (4 * math.pi * c))


def make(scene, dem, flags=0):
    rt = MoonRT(scene.width, scene.height)
    rt.upload_dem(dem)
    rt.apply_scene(scene)
    rt.set_params(flags=flags)
    return rt


def sun_angular_radius(scene):
    Lb, _ = im.sun_dir_moon_frame(scene)
    return math.degrees(math.asin(scene.light_radius / np.linalg.norm(Lb)))


def ephemeris_scene():
    E.init(E.Observer(-33.9, 18.4, 10))
    e = E.calculate_moon_ephemeris(datetime(2025, 3, 7, 21, 0, tzinfo=timezone.utc), False)
    return e, E.scene_from_ephemeris(e, 32, 32)


@pytest.mark.parametrize("n_sun", [1, 16])
def test_smooth_sphere(native_lib, n_sun):
    """D = 1: nothing occludes.  lit = the share of samples with cos > 0 (the model's; nodes with a sample in the cosine band
    excepted), mu = the model's to 1e-5, D = 1; and the terminator lies where the reference's sun_altitude_at (restated in
    ephemeris.py, pinned by tests/golden/host_astro.json), fed the date's subsolar point, crosses 0 +- the Sun's radius."""
    e, s = ephemeris_scene()
    dem = np.ones((90, 180), np.float32)
    shape = (45, 90)
    rt = make(s, dem)
    got = rt.illumination_map(shape=shape, n_sun=n_sun).reshape(-1, 4)
    la, lo = MoonRT.grid_nodes(shape=shape)
    LA, LO = np.meshgrid(la, lo, indexing="ij")
    m = im.illuminate(s, dem, LA.ravel(), LO.ravel(), MoonRT.sun_samples(n_sun).astype(np.float64))
    ok = ~m["flagged"].any(1)
    assert ok.mean() > 0.9
    assert np.array_equal(got[ok, 0], m["lit"][ok].astype(np.float32))
    assert np.abs(got[:, 2] - m["mu"]).max() < 1e-5          # D = 1: no gradient, the normal is the radial unit vector
    assert (got[:, 3] == 1.0).all()
    alt = np.array([E.sun_altitude_at(e.subsolar_lat, e.subsolar_lon, a, b) for a, b in zip(LA.ravel(), LO.ravel())])
    # margin: the light's parallax from the surface (R / distance, 0.03 deg) + the Sun direction's agreement with the
    # ephemeris (2e-3 deg, test_illumination_host) + the normal's float32 error
    r_sun = sun_angular_radius(s) if n_sun > 1 else 0.0
    margin = r_sun + 0.05
    day, night = alt > margin, alt < -margin
    assert day.sum() > 1000 and night.sum() > 1000
    assert (got[day, 0] == 1.0).all() and (got[night, 0] == 0.0).all()
    assert (got[night, 1] == 0.0).all() and (got[day, 1] > 0).all()
    rt.close()


def plateau_dem(h, w, lon_lo, lon_hi, lat_abs, height_km):
    lat = 90.0 - (np.arange(h) + 0.5) * 180.0 / h
    lon = -180.0 + (np.arange(w) + 0.5) * 360.0 / w
    on = (np.abs(lat)[:, None] <= lat_abs) & (lon[None, :] >= lon_lo) & (lon[None, :] < lon_hi)
    e = np.where(on, 1.0 + height_km / 1737.4, 1.0).astype(np.float32)
    return e / e.max()


def test_shadow_length_of_a_plateau(native_lib):
    """A flat sphere with one wide plateau (20 deg, 10 km) and a point-light Sun 8 deg above the plateau's east edge, on the
    equator (n_sun = 1).  Along the equator east of the edge the shadow ends where float64 sphere geometry puts it: the ray
    toward the light from the tip just clears the edge at the plateau's top radius.  Tolerance: one texel (the bilinear edge
    is a one-texel ramp) + one march step (the march can only see the plateau at its steps)."""
    h, w, H_km = 1440, 2880, 10.0
    dem = plateau_dem(h, w, -20.0, 0.0, 30.0, H_km)
    s = named_scene("S1", 16, 16)
    R = s.radius
    s.u, s.v = (0.0, 0.0, 1.0), (0.0, -1.0, 0.0)                     # moon frame (a, b, c) = (x, -y, z)
    d = float(np.linalg.norm(s.light_pos))
    phs = math.radians(-90.0 + 8.0)                                  # Sun 8 deg up at lon 0, in the west
    s.light_pos = (math.sin(phs) * d, -math.cos(phs) * d, 0.0)
    rt = make(s, dem)
    lon = np.linspace(0.0, 7.0, 1401)                                # the base's terminator is 8 deg east of the edge
    got = rt.illumination_at(np.zeros_like(lon), lon, n_sun=1)
    D0 = float(dem.min())
    L = np.array([math.sin(phs) * d, math.cos(phs) * d])

    def blocked(phi):        # the ray from the lifted base point toward the light meets the top circle r = R west of lon 0?
        q = (R * D0 + s.scene_epsilon) * np.array([math.sin(phi), math.cos(phi)])
        l = (L - q) / np.linalg.norm(L - q)
        b = q @ l
        t = -b + math.sqrt(b * b - (q @ q - R * R))                  # where it rises above the plateau top
        x = q + t * l
        return math.atan2(x[0], x[1]) <= 0.0

    a, b = math.radians(0.2), math.radians(7.0)
    assert blocked(a) and not blocked(b)
    for _ in range(80):
        mid = 0.5 * (a + b)
        a, b = (mid, b) if blocked(mid) else (a, mid)
    tip = math.degrees(a)
    tol = 360.0 / w + math.degrees(s.marching_step / R)
    dark = got[:, 0] == 0.0
    assert 1.0 < tip < 5.0
    assert dark[(lon > 180.0 / w) & (lon < tip - tol)].all()
    assert not dark[lon > tip + tol].any()
    edge = lon[~dark & (lon > 180.0 / w)].min()
    print(f"shadow tip: kernel {edge:.4f} deg, float64 geometry {tip:.4f} deg, tolerance {tol:.4f}")
    rt.close()


def relief_cases():
    """S1 over the crater DEM (tests/synth_np.py; gentle slopes: shadows only at the lowest Sun) and the egg-crate relief
    (steep: long shadows), each with a window on the evening terminator and one on the north polar cap (the subsolar point
    is at +18 deg: a low Sun all around the pole)."""
    s = named_scene("S1", 16, 16)
    la0, lo0 = im.subsolar_latlon(s)
    cap = ((90.0, 75.0), (lo0 - 90.0, lo0 + 90.0), (8, 32))
    return s, [("craters", mc.crater_dem(), ((20.0, -20.0), (lo0 + 86.0, lo0 + 94.0), (16, 24))), ("craters", mc.crater_dem(), cap),
               ("egg-crate", mc.corrugated_dem(), ((20.0, -20.0), (lo0 + 70.0, lo0 + 90.0), (16, 24))),
               ("egg-crate", mc.corrugated_dem(), cap)]


def test_relief_matches_the_model(native_lib):
    """n_sun = 16: nodes without a flagged sample have the model's lit exactly (their samples' visibility counted) and its
    irr closely; flagged samples stay under 0.5 %; with F_COUNT_STATS shadow_rays is the model's count."""
    s, cases = relief_cases()
    samples = MoonRT.sun_samples(16).astype(np.float64)
    blocked = 0
    for name, dem, (lat, lon, shape) in cases:
        rt = make(s, dem, flags=_lib.F_COUNT_STATS)
        st = {}
        got = rt.illumination_map(lat, lon, shape, n_sun=16, stats=st).reshape(-1, 4)
        rt.close()
        la, lo = MoonRT.grid_nodes(lat, lon, shape)
        LA, LO = np.meshgrid(la, lo, indexing="ij")
        m = im.illuminate(s, dem, LA.ravel(), LO.ravel(), samples)
        fl = m["flagged"]
        ok = ~fl.any(1)
        blocked += int((m["cos_pos"] & ~m["V"]).sum())
        full = m["irr"].max() / max(m["mu"].max(), 1e-30)            # ~ irr at normal incidence (the whole disk up)
        dirr = np.abs(got[ok, 1] - m["irr"][ok])
        print(f"{name} {lat}: flagged samples {fl.mean():.3%}, nodes with one {1 - ok.mean():.1%}, shadowed samples "
              f"{(m['cos_pos'] & ~m['V']).sum()}; |irr - model| max {dirr.max():.2e} = {dirr.max() / full:.2e} of full Sun; "
              f"|mu - model| max {np.abs(got[:, 2] - m['mu']).max():.2e}; relative irr where irr > 0.2 full Sun "
              f"{(dirr / np.maximum(m['irr'][ok], 1e-30))[m['irr'][ok] > 0.2 * full].max(initial=0):.1e}")
        assert fl.mean() < 0.005
        assert np.array_equal(got[ok, 0], m["lit"][ok].astype(np.float32))
        tol = mu_tol(dem.shape, LA.ravel())
        assert (dirr < tol[ok] * full).all()                # irr = full Sun x cos: the normal's error, nothing else
        assert (np.abs(got[:, 2] - m["mu"]) < tol).all()
        assert np.abs(got[:, 3] - m["D"]).max() < 1e-6
        assert st["shadow_rays"] == m["shadow_rays"]
    assert blocked > 1000        # shadows: the comparison is not vacuous


def test_bit_identical_invariances(native_lib):
    s, cases = relief_cases()
    _, dem, (lat, lon, shape) = cases[2]
    n = 16

    def mapped(flags, **kw):
        rt = make(s, dem, flags)
        try:
            return rt.illumination_map(lat, lon, shape, n_sun=n, **kw)
        finally:
            rt.close()
    base = mapped(0)
    assert_bit_equal(mapped(_lib.F_NO_SKIP), base, "F_NO_SKIP")
    assert_bit_equal(mapped(_lib.F_COUNT_STATS), base, "counting kernel")
    assert_bit_equal(mapped(_lib.F_FORCE_WIDE), base, "F_FORCE_WIDE")
    assert_bit_equal(mapped(_lib.F_FORCE_WIDE | _lib.F_COUNT_STATS | _lib.F_NO_SKIP), base, "wide, counting, no skip")
    rt = make(s, dem)
    bands = [rt.illumination_map(lat, lon, shape, n_sun=n, rows=r) for r in ((0, 5), (5, 6), (6, shape[0]))]
    assert_bit_equal(np.concatenate(bands), base, "three bands vs one call")
    assert_bit_equal(rt.illumination_map(lat, lon, shape, n_sun=n, band_bytes=1), base, "row-by-row through a device buffer")
    la, lo = MoonRT.grid_nodes(lat, lon, shape)
    LA, LO = np.meshgrid(la, lo, indexing="ij")
    assert_bit_equal(rt.illumination_at(LA.ravel(), LO.ravel(), n_sun=n), base.reshape(-1, 4), "points at the nodes vs grid")
    rt.set_camera((40.0, -290.0, 30.0), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0), 2.0)
    rt.set_params(seed=987, spp_per_launch=4, path_seg_min=1, path_seg_max=1)
    rt.set_capsules(np.array([[10.5, 0, 0, 0.05, 0, 10.5, 0, 0, 1, 0, 0, 0]], np.float32))
    assert_bit_equal(rt.illumination_map(lat, lon, shape, n_sun=n), base, "camera, seed, spp, segments, capsules changed")
    # a longitude window past +180 is the same map shifted by 360
    assert_bit_equal(rt.illumination_map(lat, (lon[0] + 360.0, lon[1] + 360.0), shape, n_sun=n)[..., 2:],
                     base[..., 2:], "mu and D 360 deg on")
    rt.close()


def test_no_side_effects_on_the_render_state(native_lib):
    s, cases = relief_cases()
    _, dem, (lat, lon, shape) = cases[2]
    s = s.with_size(48, 32, spp_per_launch=16)

    def run(with_map):
        rt = make(s, dem, _lib.F_COUNT_STATS)
        st1 = rt.render(1)
        if with_map:
            rt.illumination_map(lat, lon, shape, n_sun=16)
            rt.illumination_at([10.0], [20.0], n_sun=4)
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


def test_full_size_whole_moon_map(native_lib):
    """The headline DEM (23040 x 46080, synthesised on the device): a whole-Moon 2048 x 4096 map at n_sun = 16 is finite with
    lit in [0, 1], and a 64-node crop on the terminator matches the model on the DEM rows around it."""
    DEM_H, DEM_W = 23040, 46080
    src = synth_ldem(DEM_H, DEM_W)
    dem, _ = dem_from_ldem(src, DEM_H, DEM_W, 1)
    src.free()
    s = named_scene("S1", 16, 16)
    rt = MoonRT(16, 16)
    rt.bind_dem(dem, DEM_H, DEM_W)
    rt.apply_scene(s)
    rt.set_params(flags=0)
    st = {}
    full = rt.illumination_map(shape=(2048, 4096), n_sun=16, stats=st)
    print(f"whole Moon 2048 x 4096, n_sun 16: {st['kernel_ms']:.2f} ms in {st['launches']} launch(es)")
    assert np.isfinite(full).all() and full[..., 0].min() >= 0.0 and full[..., 0].max() <= 1.0
    assert 0.3 < (full[..., 0] > 0).mean() < 0.7
    la0, lo0 = im.subsolar_latlon(s)
    lat, lon, shape = (20.5, 19.5), (lo0 + 88.0, lo0 + 92.0), (8, 8)
    got = rt.illumination_map(lat, lon, shape, n_sun=16).reshape(-1, 4)
    la, lo = MoonRT.grid_nodes(lat, lon, shape)
    r0 = int((90.0 - 24.0) / 180.0 * DEM_H)
    r1 = int((90.0 - 16.0) / 180.0 * DEM_H)
    band = np.empty((r1 - r0, DEM_W), np.float32)
    assert _lib.load().mrtx_dev_download(0, band.ctypes.data, dem.ptr + r0 * DEM_W * 4, band.nbytes) == 0

    class Rows:      # the DEM rows the crop's shadow rays can reach, indexed like the whole array
        shape = (DEM_H, DEM_W)

        def __getitem__(self, rc):
            r, c = rc
            assert (r >= r0).all() and (r < r1).all(), "a shadow ray left the downloaded rows"
            return band[r - r0, c]
    LA, LO = np.meshgrid(la, lo, indexing="ij")
    m = im.illuminate(s, Rows(), LA.ravel(), LO.ravel(), MoonRT.sun_samples(16).astype(np.float64))
    ok = ~m["flagged"].any(1)
    assert ok.mean() > 0.8
    assert np.array_equal(got[ok, 0], m["lit"][ok].astype(np.float32))
    dmu = np.abs(got[:, 2] - m["mu"]).max()
    tol = mu_tol((DEM_H, DEM_W), LA.ravel())
    print(f"full-size crop: |mu - model| max {dmu:.2e} (bound {tol.min():.2e}), flagged nodes {1 - ok.mean():.1%}")
    assert (np.abs(got[:, 2] - m["mu"]) < tol).all()
    rt.close()
    dem.free()


def test_facade_illumination_at_equals_moonrt(native_lib):
    from test_facade_cpu import drive_like_init_renderer
    from moonrtx_amd.tkoptix import TkOptiX
    dem = synth_np.dem(180, 360, seed=5, craters=30)
    rt = TkOptiX(width=32, height=32)
    drive_like_init_renderer(rt, dem, synth_np.colour_map(90, 180))
    s = named_scene("S1", 32, 32)
    with rt._padlock:
        rt.update_camera("cam1", eye=list(s.eye))
        rt.update_data("moon", u=s.u, v=s.v)
        rt.update_light("sun", pos=list(s.light_pos), radius=s.light_radius)
    la0, lo0 = im.subsolar_latlon(s)
    lat = np.linspace(-60.0, 60.0, 37)
    lon = lo0 + np.linspace(60.0, 100.0, 37)
    got = rt.illumination_at(lat, lon, n_sun=16)
    ref = make(s, dem)
    want = ref.illumination_at(lat, lon, n_sun=16)
    assert_bit_equal(got, want, "TkOptiX.illumination_at vs MoonRT.illumination_at")
    assert (got[:, 0] == 1).any() and (got[:, 0] == 0).any()
    ref.close()
    rt.close()
