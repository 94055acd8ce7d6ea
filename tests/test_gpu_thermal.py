"""Regolith surface temperatures on the MI355X (DESIGN.md sections 3.10 and 4.11): the absorbed flux against the horizon and
illumination stages, FULL and SUMMARY against the float64 model fed the device's own flux, SUMMARY against FULL, bit-exact
invariances, the geothermal floor of a point that never sees the Sun, the context state and every refusal."""
from datetime import datetime, timedelta, timezone

import numpy as np
import pytest

import model_cases as mc
import thermal_model as tm
from common import assert_bit_equal
from moonrtx_amd import _lib, sunlight
from moonrtx_amd import ephemeris as E
from moonrtx_amd.renderer import DeviceBuffer, MoonRT
from moonrtx_amd.scene import named_scene
from test_gpu_illumination import make
from test_thermal_host import T_GEO, thermal_refusals

pytestmark = pytest.mark.gpu

OBS = E.Observer(52.2, 21.0, 0.0)
BLOCK = 709                       # one lunation of hourly epochs
# FULL and SUMMARY against the float64 model: the kernel's column is float64 and its rates float32 (relative error ~1e-7 per
# step, damped by the column within a few steps), its surface solve float32 (stopped at |dT| < 1e-3 K, quadratically
# convergent) and its outputs float32 (half an ulp: 1.5e-5 K at 400 K); a few 1e-3 K at most.  0.05 K leaves room.
T_TOL = 0.05


def scene():
    return named_scene("S1", 16, 16)


def points(seed, n):
    rng = np.random.default_rng(seed)
    return np.degrees(np.arcsin(rng.uniform(-0.95, 0.95, n))), rng.uniform(-180.0, 180.0, n)


def epochs(m):
    t0 = datetime(2025, 3, 1, tzinfo=timezone.utc)
    times = [t0 + timedelta(hours=k) for k in range(m)]
    return E.sun_epochs(times, OBS), E.sun_flux(times)


def small_model():
    """One lunation of spin-up with one reset: the defaults' rules at a test's size."""
    return MoonRT.thermal_grid(3600.0, 1, 1)


@pytest.fixture(scope="module")
def case():
    dem = mc.crater_dem()
    lat, lon = points(7, 40)
    ep, fl = epochs(2 * BLOCK)
    rt = make(scene(), dem, 0)
    hz = rt.horizon(lat, lon, n_az=64, n_bis=12)
    st = {}
    md = small_model()
    flux = rt.surface_temperature(lat, lon, hz, ep, fl, md, mode="flux")
    full = rt.surface_temperature(lat, lon, hz, ep, fl, md, mode="full", stats=st)
    summ = rt.surface_temperature(lat, lon, hz, ep, fl, md, mode="summary", stats=st)
    f = rt.horizon_sun(lat, lon, hz, ep)
    mu = rt.illumination_series(lat, lon, ep, n_sun=1)[..., 2]
    rt.close()
    return dict(dem=dem, lat=lat, lon=lon, ep=ep, fl=fl, hz=hz, flux=flux, full=full, summ=summ, f=f, mu=mu, st=st, md=md)


def test_flux_is_the_disc_fraction_times_the_cosine(native_lib, case):
    """FLUX is exactly 0 where horizon_sun's f is 0 or the series' mu <= 0; elsewhere (1 - A) S f mu rebuilt in float64
    from those outputs within 4e-6 relative + 1e-4 W m^-2 (about 32 float32 ulps: acosf, the albedo polynomial and four
    rounded products)."""
    flux, f, mu, fl = case["flux"], case["f"], case["mu"], case["fl"]
    assert flux.shape == f.shape == (40, 2 * BLOCK)
    dark = (f == 0.0) | (mu <= 0.0)
    assert np.all(flux[dark] == 0.0)
    want = tm.absorbed(f.astype(np.float64), mu.astype(np.float64), fl[None, :].astype(np.float32).astype(np.float64))
    lit = ~dark
    assert lit.mean() > 0.2 and ((f > 0) & (f < 1)).any()
    err = np.abs(flux[lit] - want[lit])
    assert np.all(err <= 4e-6 * want[lit] + 1e-4), err.max()
    assert np.all(flux[lit] > 0.0)


def test_full_and_summary_match_the_model(native_lib, case):
    md = case["md"]
    r = tm.run(case["flux"].astype(np.float64), md.spacing_s, md.n_sub, md.n_spin, md.block, md.n_reset)
    assert r["caps"] == 0 and r["coef_max"] <= 1.0 and case["st"]["newton_cap_hits"] == 0
    full, summ = case["full"], case["summ"]
    assert full.shape == (40, BLOCK) and np.isfinite(full).all()
    d = np.abs(full - r["full"])
    print(f"FULL against the model: max {d.max():.2e} K, mean {d.mean():.2e} K; range {full.min():.1f}-{full.max():.1f} K")
    assert d.max() < T_TOL
    assert np.abs(summ - r["summary"]).max() < T_TOL
    assert full.max() > 300.0 and full.min() < 120.0


def test_summary_is_the_reduction_of_full(native_lib, case):
    full, summ = case["full"], case["summ"]
    assert_bit_equal(summ[:, 0], full.max(1), "maximum")
    assert_bit_equal(summ[:, 1], full.min(1), "minimum")
    assert np.allclose(summ[:, 2], full.astype(np.float64).mean(1), rtol=1e-6, atol=0.0)


def test_invariances_and_horizon_sources(native_lib, case):
    """A point's outputs do not depend on the other points of the call, their order or number; host and device horizons,
    the production build and F_FORCE_WIDE give the same bits."""
    lat, lon, hz, ep, fl, md = case["lat"], case["lon"], case["hz"], case["ep"], case["fl"], case["md"]
    perm = np.random.default_rng(3).permutation(40)[:17]
    for flags in (0, _lib.F_FORCE_WIDE, _lib.F_COUNT_STATS):
        rt = make(scene(), case["dem"], flags)
        for mode in ("full", "summary", "flux"):
            want = case[{"full": "full", "summary": "summ", "flux": "flux"}[mode]]
            assert_bit_equal(rt.surface_temperature(lat[perm], lon[perm], hz[perm], ep, fl, md, mode=mode), want[perm],
                             f"{mode}, permuted subset, flags {flags}")
        buf = DeviceBuffer(hz.nbytes)
        buf.upload(hz)
        assert_bit_equal(rt.surface_temperature(lat, lon, buf, ep, fl, md, mode="summary", n_az=64), case["summ"],
                         f"device horizons, flags {flags}")
        buf.free()
        rt.close()


def test_never_lit_point_stays_at_the_geothermal_floor(native_lib):
    """A point whose horizon hides the Sun all year (the floor of a deep pit: 90 deg all round) absorbs nothing and stays
    within 0.05 K of (Q / eps sigma)^(1/4) = 24.04 K through the default spin-up and a lunation."""
    rt = make(scene(), mc.crater_dem(), 0)
    lat, lon = np.array([-89.0, 10.0]), np.array([30.0, -40.0])
    md = MoonRT.thermal_grid()
    ep, fl = epochs(md.n_spin + BLOCK)
    hz = np.full((2, 16), 90.0, np.float32)
    st = {}
    s = rt.surface_temperature(lat, lon, hz, ep, fl, md, stats=st)
    assert np.all(rt.surface_temperature(lat, lon, hz, ep, fl, md, mode="flux") == 0.0)
    rt.close()
    assert np.abs(s[:, :3] - T_GEO).max() < 0.05, s
    assert st["newton_cap_hits"] == 0


def test_surface_temperatures_end_to_end(native_lib):
    """sunlight.surface_temperatures with the device's horizons in a buffer equals the same run through thermal= (host
    horizons), bit for bit, and gives temperatures in the model's range."""
    rt = make(scene(), mc.crater_dem(), 0)
    lat, lon = points(5, 9)
    t0 = datetime(2025, 3, 1, tzinfo=timezone.utc)
    a = sunlight.surface_temperatures(rt, lat, lon, t0, 2.0, spinup_lunations=1, n_az=32, n_bis=8, observer=OBS, chunk=4)
    b = sunlight.surface_temperatures(rt, lat, lon, t0, 2.0, spinup_lunations=1, n_az=32, n_bis=8, observer=OBS, chunk=4,
                                      thermal=rt.surface_temperature)
    rt.close()
    for x, y, name in zip(a[:4], b[:4], ("t_max", "t_min", "t_mean", "t_bottom_mean")):
        assert_bit_equal(x, y, name)
    assert len(a.times) == 48 and a.times[0] == t0 and a.stats["launches"] == 6
    assert np.all((a.t_min >= 20.0) & (a.t_max <= 450.0) & (a.t_min <= a.t_mean) & (a.t_mean <= a.t_max))


def test_leaves_the_context_state_alone_and_refuses(native_lib):
    s = scene().with_size(48, 32, spp_per_launch=16)
    dem = mc.crater_dem()
    lat, lon = np.array([10.0, -20.0, 33.0]), np.array([20.0, 95.0, -80.0])
    ep, fl = epochs(2 * BLOCK)

    def run(with_thermal):
        rt = make(s, dem, _lib.F_COUNT_STATS)
        st1 = rt.render(1)
        v0 = rt.config()
        if with_thermal:
            hz = rt.horizon(lat, lon, n_az=32, n_bis=8)
            for mode in ("full", "summary", "flux"):
                rt.surface_temperature(lat, lon, hz, ep, fl, small_model(), mode=mode)
        pt = rt.illumination_at(lat, lon, n_sun=16)
        st2 = rt.render(1)
        out = rt.read_linear(), rt.read_hits(), rt.samples_done(), st1, st2, pt, v0 == rt.config()
        rt.close()
        return out
    a, b = run(False), run(True)
    assert_bit_equal(b[0], a[0], "linear radiance")
    assert_bit_equal(b[1], a[1], "hit buffer")
    assert_bit_equal(b[5], a[5], "illumination_at after the thermal stage")
    assert b[2] == a[2] == 32 and b[6]
    for k in ("primary_hits", "shadow_rays", "height_samples", "bounce_rays"):
        assert b[4][k] == a[4][k], k
    rt = make(s, dem, 0)
    thermal_refusals(native_lib, rt._ctx, 0)
    rt.close()
