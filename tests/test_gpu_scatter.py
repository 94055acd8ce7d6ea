"""Terrain-scattered sunlight and infrared on the MI355X (DESIGN.md sections 3.11 and 4.12): view hits against the float64
model and bit-exact invariances, the analytic bowl's view factor, nothing in view changing nothing, EXITANCE against FULL and
FLUX, the gather against numpy, the extra flux against the column model, the physics of a polar bowl, the context state and
the refusals."""
import math
from datetime import datetime, timedelta, timezone

import numpy as np
import pytest

import bowl_dem as bd
import model_cases as mc
import scatter_model as sm
import thermal_model as tm
from common import assert_bit_equal
from moonrtx_amd import _lib, sunlight, thermal
from moonrtx_amd import ephemeris as E
from moonrtx_amd.renderer import MoonRT
from moonrtx_amd.scene import named_scene
from oracle import numpy_paths
from test_gpu_illumination import make
from test_scatter_host import scatter_refusals
from test_thermal_host import T_GEO

pytestmark = pytest.mark.gpu

OBS = E.Observer(52.2, 21.0, 0.0)
BLOCK = 709
T_TOL = 0.05                      # the column against the float64 model (tests/test_gpu_thermal.py)
# the analytic bowl: d/D = 0.2, rim at 6 deg from the centre on a 720 x 1440 DEM (48 texels across the rim)
D_OVER_D, THETA_C, K_BOWL = 0.2, 6.0, 1024
F_BOWL = bd.bowl_view_factor(D_OVER_D)
# Tolerance of the measured share: three binomial standard deviations of K independent rays (the stratified directions do
# better than that), plus the DEM's bilinear facets: the rim, seen from the floor at about D, sits within a quarter texel
# of height of the exact bowl (slope 44 deg at the rim), 0.25 x 0.0436 / 2.09 rad, which moves f by less than 0.01.
BOWL_TOL = 3.0 * math.sqrt(F_BOWL * (1.0 - F_BOWL) / K_BOWL) + 0.01


def scene():
    return named_scene("S1", 16, 16)


def points(seed, n):
    rng = np.random.default_rng(seed)
    return np.degrees(np.arcsin(rng.uniform(-0.95, 0.95, n))), rng.uniform(-180.0, 180.0, n)


def epochs_from(t0, m):
    times = [t0 + timedelta(hours=k) for k in range(m)]
    return E.sun_epochs(times, OBS), E.sun_flux(times)


@pytest.mark.parametrize("which", ["crater", "corrugated", "bowl"])
def test_view_hits_match_the_float64_model(native_lib, which):
    """crater_dem's craters are too shallow for a point to see much of them (a view factor of about 4 (d/D)^2): there the
    check is that every unflagged ray escapes on both sides; corrugated_dem and the bowl give hits."""
    if which == "bowl":
        dem = bd.bowl_dem(720, 1440, 0.0, 0.0, THETA_C, D_OVER_D)
        lat, lon = bd.bowl_points(0.0, 0.0, THETA_C, [0.3, 0.6, 0.85, 1.2])
    else:
        dem = mc.crater_dem() if which == "crater" else mc.corrugated_dem()
        lat, lon = points(11, 24)
    k = 64
    rt = make(scene(), dem, _lib.F_COUNT_STATS)
    st = {}
    hits, share = rt.view_hits(lat, lon, k=k, stats=st)
    rt.close()
    m = sm.view_hits(scene(), dem, lat, lon, k)
    ok = ~m["flagged"]
    got = ~np.isnan(hits[..., 0])
    assert np.array_equal(np.isnan(hits[..., 0]), np.isnan(hits[..., 1]))
    assert ok.mean() > 0.9 and (~got).any() and (got.any() or which == "crater")
    assert np.array_equal(got[ok], m["hit"][ok]), int((got[ok] != m["hit"][ok]).sum())
    assert np.array_equal(share, (got.sum(1) / k).astype(np.float32))
    # hit positions: one final bisection bracket along the ray, float32 positions, the latlon polynomial (1.3e-7 rad)
    both = ok & got & m["hit"]
    ang = sm.angle_between(hits[..., 0][both], hits[..., 1][both], m["lat"][both], m["lon"][both]) if both.any() else np.zeros(1)
    tol = (numpy_paths.bracket(scene()) + 4e-5) / (0.9 * scene().radius) + 1e-6
    print(f"{which}: {int(both.sum())} hits, {(~ok).sum()} flagged rays, max angle {ang.max():.2e} rad (tol {tol:.2e})")
    assert ang.max() < tol
    assert st["bounce_rays"] == lat.size * k and st["height_samples"] > 0 and st["launches"] == 1


def test_view_hits_are_bit_exact_under_order_subsets_builds_and_wide(native_lib):
    dem = mc.crater_dem()
    lat, lon = points(12, 40)
    runs = {}
    for flags in (0, _lib.F_COUNT_STATS, _lib.F_FORCE_WIDE, _lib.F_COUNT_STATS | _lib.F_FORCE_WIDE):
        rt = make(scene(), dem, flags)
        runs[flags] = rt.view_hits(lat, lon, k=32)
        if flags == 0:
            perm = np.random.default_rng(3).permutation(lat.size)
            hp, sp = rt.view_hits(lat[perm], lon[perm], k=32)
            hs, ss = rt.view_hits(lat[5:9], lon[5:9], k=32)
        rt.close()
    h0, s0 = runs[0]
    for flags, (h, s) in runs.items():
        assert_bit_equal(h, h0, f"hits, flags {flags}")
        assert_bit_equal(s, s0, f"share, flags {flags}")
    assert_bit_equal(hp, h0[perm], "hits, permuted points")
    assert_bit_equal(sp, s0[perm], "share, permuted points")
    assert_bit_equal(hs, h0[5:9], "hits, a subset")
    # K = 2K' takes the same direction j only where the tables agree; the share is a count over K
    assert np.all((s0 * 32) == np.round(s0 * 32))


def test_bowl_interior_sees_the_analytic_view_factor(native_lib):
    """Buhl et al. 1968: every interior point of a spherical bowl sees the bowl with f = 4 (d/D)^2 / (1 + 4 (d/D)^2)."""
    dem = bd.bowl_dem(720, 1440, 0.0, 0.0, THETA_C, D_OVER_D)
    lat, lon = bd.bowl_points(0.0, 0.0, THETA_C, [0.3, 0.6, 0.85])
    rt = make(scene(), dem, 0)
    _, share = rt.view_hits(lat, lon, k=K_BOWL)
    rt.close()
    err = np.abs(share.astype(np.float64) - F_BOWL)
    print(f"bowl d/D = {D_OVER_D}: f = {F_BOWL:.4f}, measured {share.min():.4f} - {share.max():.4f}, "
          f"max error {err.max():.4f} (tol {BOWL_TOL:.4f})")
    assert err.max() < BOWL_TOL


def test_nothing_in_view_changes_nothing(native_lib):
    """On the smooth sphere every view ray escapes, so Q_sec is exactly 0 and surface_temperatures(scatter=K) equals
    scatter=0 bit for bit; the EXT column with an all-zero extra table equals mrtx_thermal bit for bit on crater_dem."""
    smooth = np.ones((180, 360), np.float32)
    lat, lon = np.array([-85.0, -60.0, 0.0, 45.0]), np.array([0.0, 30.0, 60.0, -120.0])
    rt = make(scene(), smooth, 0)
    hits, share = rt.view_hits(lat, lon, k=64)
    assert np.isnan(hits).all() and np.all(share == 0.0)
    t0 = datetime(2025, 1, 1, tzinfo=timezone.utc)
    a = sunlight.surface_temperatures(rt, lat, lon, t0, 2.0, spinup_lunations=1, n_az=32, n_bis=10, observer=OBS)
    b = sunlight.surface_temperatures(rt, lat, lon, t0, 2.0, spinup_lunations=1, n_az=32, n_bis=10, observer=OBS,
                                      scatter=64, q_sec_mean=True)
    rt.close()
    for x, y in zip(a[:4], b[:4]):
        assert_bit_equal(y, x, "scatter=K against scatter=0 on the smooth sphere")
    assert b.stats["scatter_hits"] == 0 and np.all(b.stats["q_sec_mean"] == 0.0)

    dem = mc.crater_dem()
    lat, lon = points(7, 24)
    ep, fl = epochs_from(datetime(2025, 3, 1, tzinfo=timezone.utc), 2 * BLOCK)
    md = MoonRT.thermal_grid(3600.0, 1, 1)
    rt = make(scene(), dem, 0)
    hz = rt.horizon(lat, lon, n_az=64, n_bis=12)
    zero = np.zeros((lat.size, ep.shape[0]), np.float32)
    for mode in ("full", "summary", "flux"):
        want = rt.surface_temperature(lat, lon, hz, ep, fl, md, mode=mode)
        assert_bit_equal(rt.surface_temperature_scatter(lat, lon, hz, ep, fl, md, mode=mode, extra_flux=zero), want, mode)
        assert_bit_equal(rt.surface_temperature_scatter(lat, lon, hz, ep, fl, md, mode=mode), want, mode + ", no table")
    rt.close()


@pytest.fixture(scope="module")
def crater_case():
    dem = mc.crater_dem()
    lat, lon = points(7, 24)
    ep, fl = epochs_from(datetime(2025, 3, 1, tzinfo=timezone.utc), 2 * BLOCK)
    md = MoonRT.thermal_grid(3600.0, 1, 1)
    rt = make(scene(), dem, 0)
    hz = rt.horizon(lat, lon, n_az=64, n_bis=12)
    full = rt.surface_temperature(lat, lon, hz, ep, fl, md, mode="full")
    flux = rt.surface_temperature(lat, lon, hz, ep, fl, md, mode="flux")
    ex = rt.surface_temperature_scatter(lat, lon, hz, ep, fl, md, mode="exitance")
    rng = np.random.default_rng(5)
    extra = rng.uniform(0.0, 20.0, (lat.size, ep.shape[0])).astype(np.float32)
    xflux = rt.surface_temperature_scatter(lat, lon, hz, ep, fl, md, mode="flux", extra_flux=extra)
    xfull = rt.surface_temperature_scatter(lat, lon, hz, ep, fl, md, mode="full", extra_flux=extra)
    mu = rt.illumination_series(lat, lon, ep, n_sun=1)[..., 2]
    rt.close()
    return dict(full=full, flux=flux, ex=ex, extra=extra, xflux=xflux, xfull=xfull, md=md, mu=mu)


def test_exitance_is_what_full_and_flux_report(native_lib, crater_case):
    c = crater_case
    n_spin = int(c["md"].n_spin)
    ex, full, flux = c["ex"], c["full"], c["flux"][:, n_spin:]
    assert ex.shape == full.shape + (2,)
    # M_ir = eps sigma T^4 of FULL's temperatures (float32: four rounded products)
    t = full.astype(np.float64)
    want = np.float32(thermal.EMISSIVITY * thermal.SIGMA) * t ** 4
    assert np.all(np.abs(ex[..., 1] - want) <= 4e-7 * want)
    # M_vis (1 - A) / A is FLUX's Q_abs: both exactly 0 in the dark, else equal to float32 rounding
    dark = flux == 0.0
    assert np.all(ex[..., 0][dark] == 0.0) and np.all(ex[..., 0][~dark] > 0.0) and (~dark).mean() > 0.2
    # with A(theta) rebuilt in float64 from the illumination series' mu (acosf and the albedo polynomial in float32 on the
    # device: a few 1e-7 of A, amplified by 1 / (1 - A) <= 7)
    mu = c["mu"][:, n_spin:][~dark].astype(np.float64)
    A = thermal.albedo(np.degrees(np.arccos(np.clip(mu, -1.0, 1.0))))
    mv = ex[..., 0][~dark].astype(np.float64)
    q = flux[~dark].astype(np.float64)
    err = np.abs(mv * (1.0 - A) / A - q)
    print(f"EXITANCE: M_vis (1 - A) / A against Q_abs: max relative {(err / q).max():.2e}; A {A.min():.3f} - {A.max():.3f}")
    assert np.all(err <= 2e-5 * q + 1e-4)


def test_gather_is_the_ordered_numpy_reduction(native_lib):
    rng = np.random.default_rng(9)
    n, k, n_hits, m = 37, 64, 500, 203
    index = np.where(rng.random((n, k)) < 0.4, rng.integers(0, n_hits, (n, k)), -1).astype(np.int32)
    index[3] = -1
    ex = (rng.random((n_hits, m, 2)) * np.array([300.0, 100.0])).astype(np.float32)
    a_h = thermal.albedo_hemispherical()
    want = sm.gather(index, ex, a_h, thermal.EMISSIVITY)
    rt = make(scene(), np.ones((90, 180), np.float32), 0)
    got = rt.scatter_flux(index, ex, a_h, thermal.EMISSIVITY)
    rt.close()
    assert_bit_equal(got, want, "Q_sec")
    assert np.all(got[3] == 0.0)


def test_gather_without_hits_is_zero(native_lib):
    # every ray sees sky, so the hit list is empty: a (0, m, 2) host exitance is a valid table and Q_sec is 0
    rt = make(scene(), np.ones((90, 180), np.float32), 0)
    got = rt.scatter_flux(np.full((5, 16), -1, np.int32), np.zeros((0, 7, 2), np.float32), thermal.albedo_hemispherical(),
                          thermal.EMISSIVITY)
    rt.close()
    assert got.shape == (5, 7) and np.all(got == 0.0)


def test_extra_flux_drives_the_column_as_the_model_says(native_lib, crater_case):
    c = crater_case
    md = c["md"]
    # FLUX with the table is Q_abs + Q_sec, each sum rounded once
    assert_bit_equal(c["xflux"], (c["flux"] + c["extra"]).astype(np.float32), "FLUX with the extra table")
    r = tm.run(c["xflux"].astype(np.float64), md.spacing_s, md.n_sub, md.n_spin, md.block, md.n_reset)
    d = np.abs(c["xfull"] - r["full"])
    print(f"FULL with extra flux against the model: max {d.max():.2e} K")
    assert r["caps"] == 0 and d.max() < T_TOL
    assert np.all(c["xfull"] >= c["full"] - 1e-3)


@pytest.fixture(scope="module")
def polar_bowl():
    """A d/D = 0.2 bowl 3 deg in radius centred 85 deg south: its floor never sees the Sun, its pole-facing wall does."""
    lat0, th = -85.0, 3.0
    dem = bd.bowl_dem(720, 1440, lat0, 0.0, th, D_OVER_D)
    lat, lon = bd.bowl_points(lat0, 0.0, th, [0.25, 0.5, 0.8], n_az=8)
    rt = make(scene(), dem, 0)
    t0 = datetime(2025, 1, 1, tzinfo=timezone.utc)
    kw = dict(spinup_lunations=1, n_az=64, n_bis=12, observer=OBS)
    base = sunlight.surface_temperatures(rt, lat, lon, t0, 15.0, **kw)
    scat = sunlight.surface_temperatures(rt, lat, lon, t0, 15.0, scatter=K_BOWL, q_sec_mean=True, **kw)
    hz = rt.horizon(lat, lon, n_az=64, n_bis=12)
    md = MoonRT.thermal_grid(3600.0, 1, 1)
    times = [t0 + timedelta(hours=k - int(md.n_spin)) for k in range(int(md.n_spin) + 360)]
    direct = rt.surface_temperature(lat, lon, hz, E.sun_epochs(times, OBS), E.sun_flux(times), md, mode="flux")
    rt.close()
    return dict(lat=lat, lon=lon, base=base, scat=scat, direct=direct)


def test_scattered_flux_warms_a_polar_bowl(native_lib, polar_bowl):
    b, s = polar_bowl["base"], polar_bowl["scat"]
    for name in ("t_max", "t_min", "t_mean"):
        assert np.all(getattr(s, name) >= getattr(b, name) - 1e-3), name
    dark = np.all(polar_bowl["direct"] == 0.0, axis=1)
    lit = ~dark
    assert dark[0] and lit.any(), "the floor is never lit; some of the wall is"
    rise = s.t_mean[dark] - b.t_mean[dark]
    print(f"never-lit points: {int(dark.sum())}; floor mean {b.t_mean[0]:.2f} K -> {s.t_mean[0]:.2f} K "
          f"(min {s.t_min[0]:.2f} K), rise over the dark points {rise.min():.2f} - {rise.max():.2f} K; "
          f"view factors {s.stats['view_factor'].min():.3f} - {s.stats['view_factor'].max():.3f}; hits {s.stats['scatter_hits']}")
    assert b.t_max[0] < T_GEO + 0.5
    assert s.t_max[0] > T_GEO + 5.0 and s.t_mean[0] > T_GEO + 2.0
    # a spherical bowl's interior receives the same irradiance from the bowl at every point: Q_sec of the never-lit points is
    # uniform within the tolerance of the view factor, relative to it
    q = s.stats["q_sec_mean"][dark]
    rel = BOWL_TOL / F_BOWL
    print(f"Q_sec over the never-lit points: {q.min():.3f} - {q.max():.3f} W m^-2 (relative spread allowed {rel:.2f})")
    assert q.min() > 0.0 and (q.max() - q.min()) <= rel * q.mean()
    assert set(s.stats["stage_s"]) >= {"view_hits", "horizons", "hit_horizons", "hit_columns", "gather", "columns"}


def test_leaves_the_context_state_alone_and_refuses(native_lib):
    s = scene().with_size(48, 32, spp_per_launch=16)
    dem = mc.crater_dem()
    lat, lon = np.array([10.0, -20.0, 33.0]), np.array([20.0, 95.0, -80.0])
    ep, fl = epochs_from(datetime(2025, 3, 1, tzinfo=timezone.utc), 2 * BLOCK)
    md = MoonRT.thermal_grid(3600.0, 1, 1)

    def run(with_scatter):
        rt = make(s, dem, _lib.F_COUNT_STATS)
        st1 = rt.render(1)
        v0 = rt.config()
        if with_scatter:
            hits, _ = rt.view_hits(lat, lon, k=16)
            hz = rt.horizon(lat, lon, n_az=32, n_bis=8)
            for mode in ("full", "summary", "flux", "exitance"):
                rt.surface_temperature_scatter(lat, lon, hz, ep, fl, md, mode=mode, extra_flux=np.ones((3, 2 * BLOCK)))
            rt.scatter_flux(np.zeros((3, 16), np.int32), np.ones((1, 8, 2), np.float32), 0.2, 0.95)
        pt = rt.illumination_at(lat, lon, n_sun=16)
        st2 = rt.render(1)
        out = rt.read_linear(), rt.read_hits(), rt.samples_done(), st1, st2, pt, v0 == rt.config()
        rt.close()
        return out
    a, b = run(False), run(True)
    assert_bit_equal(b[0], a[0], "linear radiance")
    assert_bit_equal(b[1], a[1], "hit buffer")
    assert_bit_equal(b[5], a[5], "illumination_at after the scatter stages")
    assert b[2] == a[2] == 32 and b[6]
    for k in ("primary_hits", "shadow_rays", "height_samples", "bounce_rays"):
        assert b[4][k] == a[4][k], k
    rt = make(s, dem, 0)
    scatter_refusals(native_lib, rt._ctx, 0)
    with pytest.raises(Exception, match="outside the hit list"):
        rt.scatter_flux(np.ones((1, 16), np.int32), np.ones((1, 8, 2), np.float32), 0.2, 0.95)
    with pytest.raises(Exception, match="K must be"):
        rt.view_hits(lat, lon, k=24)
    rt.close()
