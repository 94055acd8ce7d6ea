"""Terrain horizons and the Sun against them on the MI355X (DESIGN.md sections 3.8, 3.9 and 4.10): the float64 model
(tests/horizon_model.py) on relief and the smooth sphere, the bit-exact properties of 3.8, the counters, consistency with the
direct illumination series over a lunation, SUMMARY against FULL, the render state left alone, and the full-size DEM."""
from datetime import datetime, timedelta, timezone

import numpy as np
import pytest

import horizon_model as hm
import model_cases as mc
from common import assert_bit_equal
from moonrtx_amd import _lib
from moonrtx_amd import ephemeris as E
from moonrtx_amd.renderer import DeviceBuffer, MoonRT, synth_ldem, dem_from_ldem
from moonrtx_amd.scene import named_scene
from moonrtx_amd.sunlight import illumination_statistics
from test_gpu_illumination import make, plateau_dem

pytestmark = pytest.mark.gpu

OBS = E.Observer(52.2, 21.0, 0.0)
FLAG_SETS = (0, _lib.F_COUNT_STATS, _lib.F_FORCE_WIDE, _lib.F_COUNT_STATS | _lib.F_FORCE_WIDE)
# unflagged (point, azimuth) shares of the model at 24 points x 32 azimuths x 10 probes, measured on the CPU from the model
# alone: craters 0.953, egg-crate 0.552 (the last probes graze the relief that makes the horizon, so steep relief flags more);
# the floors leave room below those
FLOORS = {"craters": 0.90, "egg-crate": 0.45}


def scene():
    return named_scene("S1", 16, 16)


def points(seed, n):
    rng = np.random.default_rng(seed)
    return np.degrees(np.arcsin(rng.uniform(-0.95, 0.95, n))), rng.uniform(-180.0, 180.0, n)


def lunation(step_h=4):
    t0 = datetime(2025, 3, 1, tzinfo=timezone.utc)
    return E.sun_epochs([t0 + timedelta(hours=step_h * k) for k in range(int(29.6 * 24 / step_h))], OBS)


@pytest.mark.parametrize("name", ["craters", "egg-crate"])
def test_relief_matches_the_model(native_lib, name):
    """Every unflagged (point, azimuth) is the model's bisection result bit for bit; the unflagged share is above FLOORS."""
    dem = mc.crater_dem() if name == "craters" else mc.corrugated_dem()
    s = scene()
    lat, lon = points(11, 24)
    m = hm.horizon(s, dem, lat, lon, 32, 10)
    rt = make(s, dem, 0)
    got = rt.horizon(lat, lon, n_az=32, n_bis=10)
    rt.close()
    ok = ~m["flagged"]
    bad = np.argwhere(ok & (got != m["elev"]))
    assert ok.mean() > FLOORS[name], ok.mean()
    assert bad.size == 0, f"{len(bad)} unflagged entries differ, e.g. {[(tuple(b), got[tuple(b)], m['elev'][tuple(b)]) for b in bad[:5]]}"
    print(f"{name}: unflagged {ok.mean():.3f}, differing among the flagged {(got != m['elev'])[~ok].mean():.3f}")


def test_smooth_sphere(native_lib):
    """D = 1: the output is 0 or 180 * 2^-n_bis at every point and azimuth (the first probe lies on the horizontal)."""
    dem = np.ones((90, 180), np.float32)
    lat, lon = points(3, 40)
    rt = make(scene(), dem, 0)
    for n_bis in (1, 7, 14):
        got = rt.horizon(lat, lon, n_az=64, n_bis=n_bis)
        assert set(np.unique(got).tolist()) <= {0.0, float(np.float32(hm.bisection_step_deg(n_bis)))}, n_bis
    rt.close()


def test_bit_exact_properties(native_lib):
    """Point order and batching, azimuth nesting, bisection nesting, and the production and counting builds with and
    without WIDE addressing all give the same bits."""
    s = scene()
    dem = mc.corrugated_dem()
    lat, lon = points(21, 40)
    ref = None
    for flags in FLAG_SETS:
        rt = make(s, dem, flags)
        a = rt.horizon(lat, lon, n_az=32, n_bis=9)
        if ref is None:
            ref = a
        assert_bit_equal(a, ref, f"flags {flags} against production")
        perm = np.random.default_rng(flags).permutation(lat.size)
        assert_bit_equal(rt.horizon(lat[perm], lon[perm], n_az=32, n_bis=9), a[perm], f"flags {flags}: point order")
        parts = [rt.horizon(lat[i:i + 7], lon[i:i + 7], n_az=32, n_bis=9) for i in range(0, lat.size, 7)]
        assert_bit_equal(np.concatenate(parts), a, f"flags {flags}: batching")
        assert_bit_equal(rt.horizon(lat[5:6], lon[5:6], n_az=32, n_bis=9), a[5:6], f"flags {flags}: a point alone")
        # azimuth nesting: entry 2a at 2 n_az is entry a at n_az (also across the one-wave-per-point split at 64)
        for n_az in (4, 16, 64):
            lo_ = rt.horizon(lat, lon, n_az=n_az, n_bis=9)
            hi_ = rt.horizon(lat, lon, n_az=2 * n_az, n_bis=9)
            assert_bit_equal(hi_[:, ::2], lo_, f"flags {flags}: azimuth nesting at {n_az}")
        # bisection nesting: n_bis + 1 gives the n_bis value or that minus one half-step
        for n_bis in (1, 9, 15):
            b0 = rt.horizon(lat, lon, n_az=32, n_bis=n_bis).astype(np.float64)
            b1 = rt.horizon(lat, lon, n_az=32, n_bis=n_bis + 1).astype(np.float64)
            half = 180.0 * 2.0 ** -(n_bis + 1)
            same, lower = b1 == b0, np.abs(b1 - (b0 - half)) <= 1e-5 * max(1.0, half)
            assert (same | lower).all(), f"flags {flags}: bisection nesting at {n_bis}"
        rt.close()


def test_counters_match_the_model(native_lib):
    """shadow_rays = probes with n . d > 0 and height_samples = 5 per (point, azimuth) + every step of every probe march,
    the model's counts, on a case with no flagged probe (2 crater points x 8 azimuths x 6 probes)."""
    s = scene()
    dem = mc.crater_dem()
    lat, lon = points(100, 2)
    m = hm.horizon(s, dem, lat, lon, 8, 6)
    assert not m["flagged"].any()
    for flags in (_lib.F_COUNT_STATS, _lib.F_COUNT_STATS | _lib.F_FORCE_WIDE):
        rt = make(s, dem, flags)
        st = {}
        got = rt.horizon(lat, lon, n_az=8, n_bis=6, stats=st)
        rt.close()
        assert np.array_equal(got, m["elev"])
        assert st["shadow_rays"] == m["shadow_rays"], (st, m["shadow_rays"])
        assert st["height_samples"] == m["height_samples"], (st, m["height_samples"])
        assert st["launches"] == 1 and st["dem_fetches"] > 0


def consistency(rt, s, dem, lat, lon, ep, n_az, n_bis):
    """Per (point, epoch): the horizon stage's f, the series' lit at n_sun = 1 and 64, and the band about the horizon."""
    hz = rt.horizon(lat, lon, n_az=n_az, n_bis=n_bis)
    f = rt.horizon_sun(lat, lon, hz, ep)
    lit1 = rt.illumination_series(lat, lon, ep, n_sun=1)[..., 0]
    lit64 = rt.illumination_series(lat, lon, ep, n_sun=64)[..., 0]
    e_s, phi, alpha = hm.sun_position(s, dem, lat, lon, ep)
    hh, h0, h1 = hm.horizon_at(hz, phi)
    band = np.abs(h1 - h0) + hm.bisection_step_deg(n_bis)
    return f, lit1, lit64, e_s - hh, band, alpha


def check_consistency(f, lit1, lit64, gap, band, alpha, max_share):
    sure1 = np.abs(gap) > band
    bad1 = np.argwhere(sure1 & ((f > 0.5) != (lit1 > 0)))
    sure64 = np.abs(gap) > band + alpha
    disc = (f == 0) | (f == 1)
    bad64 = np.argwhere(sure64 & ((~disc) | (f != lit64) | ~((lit64 == 0) | (lit64 == 1))))
    assert sure1.sum() > 0.5 * gap.size and sure64.sum() > 0.4 * gap.size
    msg = (f"n_sun 1: {len(bad1)} of {sure1.sum()} outside the band disagree {[tuple(b) for b in bad1[:10]]}; "
           f"n_sun 64: {len(bad64)} of {sure64.sum()} {[tuple(b) for b in bad64[:10]]}")
    assert len(bad1) <= max_share * sure1.sum(), msg
    assert len(bad64) <= max_share * sure64.sum(), msg
    print(msg)


def test_consistent_with_the_series_behind_a_plateau(native_lib):
    """Over a lunation, points east of a 10 km plateau's edge: the centre above the interpolated horizon (f > 0.5) is the
    series' lit at n_sun = 1, and f in {0, 1} is its lit at n_sun = 64, wherever the centre / the whole disc lies more than a
    band (the neighbouring samples' spread + one bisection step) from the horizon: no disagreement."""
    s = scene()
    dem = plateau_dem(720, 1440, -20.0, 0.0, 30.0, 10.0)
    lat = np.array([0.0, 5.0, -10.0, 0.0, 20.0])
    lon = np.array([0.5, 1.0, 2.0, 4.0, 1.5])
    rt = make(s, dem, 0)
    check_consistency(*consistency(rt, s, dem, lat, lon, lunation(), 256, 14), max_share=0.0)
    rt.close()


def test_consistent_with_the_series_on_relief(native_lib):
    """The same on cratered and steep relief: at most 1 % disagreements outside the band (terrain between two azimuth
    samples is not in the interpolated horizon)."""
    s = scene()
    ep = lunation()
    for dem in (mc.crater_dem(), mc.corrugated_dem()):
        lat, lon = points(31, 24)
        rt = make(s, dem, 0)
        check_consistency(*consistency(rt, s, dem, lat, lon, ep, 256, 14), max_share=0.01)
        rt.close()


def f_tolerance(info, n_az):
    """How far the kernel's float32 f may lie from the model's float64 f, per (point, epoch).  The light's direction, the local
    frame and atan2f / asinf agree with float64 to a few ulp: 5e-5 deg covers the elevation e_s and the azimuth phi_s (the
    Lb table rounds the light's position to 2^-24 of ~2e4 R, 1e-7 rad; the frame's float32 sin / cos, 6e-8 rad).  An azimuth
    error moves the interpolated horizon by its slope, (h1 - h0) per 360 / n_az degrees; the float32 interpolation adds an
    ulp of h.  With r = (h - e_s) / alpha, df/dr = -(2 / pi) sqrt(1 - r^2), and near r = +-1 f changes as |dr|^1.5."""
    d_ang = 5e-5
    d_h = np.abs(info["h1"] - info["h0"]) * (n_az / 360.0) * d_ang + 1e-5
    r = (info["h"] - info["e_s"]) / info["alpha"]
    d_r = (d_ang + d_h) / info["alpha"] + np.abs(r) * 1e-6
    return (2 / np.pi) * (np.sqrt(np.maximum(0.0, 1.0 - r * r)) + np.sqrt(2 * d_r)) * d_r + 2e-6


def test_sun_fraction_matches_the_model(native_lib):
    """FULL f against the float64 model (horizon_model.sun_fraction) fed the kernel's own horizons, over a lunation at one-hour
    steps, at polar points where the Sun grazes the horizon (partial discs) and at mid-latitudes: every (point, epoch) within
    f_tolerance, partial discs present.  SUMMARY's mean agrees with the model's.  A point light (radius 0) gives the step
    e_s > h wherever the centre lies outside the float32 error from the horizon."""
    s = scene()
    dem = mc.crater_dem()
    rng = np.random.default_rng(51)
    lat = np.concatenate([rng.uniform(-89.0, -80.0, 16), rng.uniform(80.0, 89.0, 8), rng.uniform(-50.0, 50.0, 8)])
    lon = rng.uniform(-180.0, 180.0, lat.size)
    ep = lunation(step_h=1)
    n_az = 256
    rt = make(s, dem, 0)
    hz = rt.horizon(lat, lon, n_az=n_az, n_bis=14)
    f = rt.horizon_sun(lat, lon, hz, ep)
    summ = rt.horizon_sun(lat, lon, hz, ep, summary=True)
    ep0 = ep.copy()
    ep0[:, 3] = 0.0                                             # a point light at the Sun's centre
    f0 = rt.horizon_sun(lat, lon, hz, ep0)
    rt.close()
    fm, info = hm.sun_fraction(s, dem, lat, lon, hz, ep)
    tol = f_tolerance(info, n_az)
    err = np.abs(f - fm)
    partial = (fm > 1e-3) & (fm < 1.0 - 1e-3)
    worst = np.unravel_index(np.argmax(err / tol), err.shape)
    print(f"{partial.sum()} partial discs of {fm.size}; max |f - model| {err.max():.2e}, worst error / tolerance "
          f"{(err / tol).max():.3f} at {worst}")
    assert partial.sum() >= 100
    assert (err <= tol).all(), (f"{(err > tol).sum()} (point, epoch) beyond the tolerance; worst {worst}: kernel "
                                f"{f[worst]!r}, model {fm[worst]!r}, tolerance {tol[worst]:.2e}")
    m = f.shape[1]
    assert np.all(np.abs(summ[:, 0] - fm.mean(1)) <= tol.sum(1) / m + 1e-6)
    # the point light
    gap = info["e_s"] - info["h"]
    d_h = np.abs(info["h1"] - info["h0"]) * (n_az / 360.0) * 5e-5 + 1e-5
    sure = np.abs(gap) > 5e-5 + d_h
    assert sure.mean() > 0.99
    assert np.array_equal(f0[sure], (gap[sure] > 0).astype(np.float32))
    assert set(np.unique(f0).tolist()) <= {0.0, 1.0}


def test_summary_is_the_reduction_of_full(native_lib):
    """SUMMARY's counts and longest dark run equal FULL's reduction exactly; its mean agrees with FULL's float64 sum to 1e-6
    relative.  Host and device horizons give the same bits."""
    s = scene()
    dem = mc.crater_dem()
    lat, lon = points(41, 50)
    ep = lunation(step_h=1)                                   # 710 epochs: eleven 64-epoch chunks, runs across them
    rt = make(s, dem, 0)
    hz = rt.horizon(lat, lon, n_az=64, n_bis=12)
    full = rt.horizon_sun(lat, lon, hz, ep)
    summ = rt.horizon_sun(lat, lon, hz, ep, summary=True)
    buf = DeviceBuffer(hz.nbytes)
    buf.upload(hz)
    assert_bit_equal(rt.horizon_sun(lat, lon, buf, ep, n_az=64), full, "FULL from device horizons")
    assert_bit_equal(rt.horizon_sun(lat, lon, buf, ep, summary=True, n_az=64), summ, "SUMMARY from device horizons")
    assert_bit_equal(rt.horizon(lat, lon, n_az=64, n_bis=12, out=buf).download(np.float32, hz.shape), hz, "device horizons")
    buf.free()
    rt.close()
    want = hm.summarize(full)
    m = full.shape[1]
    assert full.shape == (50, m) and np.isfinite(full).all() and full.min() >= 0.0 and full.max() <= 1.0
    assert np.array_equal(summ[:, 1], want[:, 1].astype(np.float32))
    assert np.array_equal(summ[:, 2], want[:, 2].astype(np.float32))
    assert np.array_equal(summ[:, 3], want[:, 3].astype(np.float32))
    assert np.allclose(summ[:, 0], want[:, 0], rtol=1e-6, atol=0.0) and np.all((summ[:, 0] == 0) == (want[:, 0] == 0))
    assert (want[:, 3] > 64).any()                            # dark runs cross chunk boundaries
    assert ((full > 0) & (full < 1)).any()                    # partial discs occur


def test_leaves_the_context_state_alone(native_lib):
    s = scene().with_size(48, 32, spp_per_launch=16)
    dem = mc.crater_dem()
    lat, lon = np.array([10.0, -20.0, 33.0]), np.array([20.0, 95.0, -80.0])
    ep = lunation(step_h=24)

    def run(with_horizon):
        rt = make(s, dem, _lib.F_COUNT_STATS)
        st1 = rt.render(1)
        v0 = rt.config()
        if with_horizon:
            hz = rt.horizon(lat, lon, n_az=32, n_bis=8)
            rt.horizon_sun(lat, lon, hz, ep)
            rt.horizon_sun(lat, lon, hz, ep, summary=True)
        pt = rt.illumination_at(lat, lon, n_sun=16)
        st2 = rt.render(1)
        out = rt.read_linear(), rt.read_hits(), rt.samples_done(), st1, st2, pt, v0 == rt.config()
        rt.close()
        return out
    a, b = run(False), run(True)
    assert_bit_equal(b[0], a[0], "linear radiance")
    assert_bit_equal(b[1], a[1], "hit buffer")
    assert_bit_equal(b[5], a[5], "illumination_at after the horizon stage")
    assert b[2] == a[2] == 32 and b[6]
    for k in ("primary_hits", "shadow_rays", "height_samples", "bounce_rays"):
        assert b[4][k] == a[4][k], k


def test_full_size_polar_year(native_lib):
    """The headline DEM (23040 x 46080, WIDE addressing), a 256 x 256 south-polar window at n_az = 256, a year of hourly
    epochs through sunlight.illumination_statistics: finite, in range, and runs consistent with the lit fractions."""
    DEM_H, DEM_W = 23040, 46080
    src = synth_ldem(DEM_H, DEM_W)
    dem, _ = dem_from_ldem(src, DEM_H, DEM_W, 1)
    src.free()
    rt = MoonRT(16, 16)
    rt.bind_dem(dem, DEM_H, DEM_W)
    rt.apply_scene(scene())
    rt.set_params(flags=0)
    la, lo = MoonRT.grid_nodes(lat=(-84.0, -90.0), lon=(-180.0, 180.0), shape=(256, 256))
    LA, LO = np.meshgrid(la, lo, indexing="ij")
    r = illumination_statistics(rt, LA.ravel(), LO.ravel(), datetime(2025, 1, 1, tzinfo=timezone.utc), 365, step_min=60,
                                n_az=256, n_bis=14, observer=OBS, chunk=32768)
    rt.close()
    dem.free()
    m = len(r.times)
    print(f"65536 points x {m} epochs: {r.stats['kernel_ms']:.1f} ms of kernels in {r.stats['launches']} launches; "
          f"mean lit share {r.lit_fraction.mean():.3f}")
    assert m == 8760 and r.mean_fraction.shape == (65536,)
    for v in (r.mean_fraction, r.lit_fraction, r.full_fraction):
        assert np.isfinite(v).all() and v.min() >= 0.0 and v.max() <= 1.0
    assert (r.full_fraction <= r.mean_fraction + 1e-6).all() and (r.mean_fraction <= r.lit_fraction + 1e-6).all()
    hours = m * 1.0
    assert np.isfinite(r.longest_dark_h).all() and (r.longest_dark_h >= 0).all() and (r.longest_dark_h <= hours).all()
    # a spot never lit is dark throughout; a spot lit at every date has no dark run; the dark hours bound the longest night
    assert (r.longest_dark_h[r.lit_fraction == 0] == hours).all()
    assert (r.longest_dark_h[r.lit_fraction == 1] == 0).all()
    assert (r.longest_dark_h <= (1.0 - r.lit_fraction) * hours + 1e-6).all()
    assert (r.longest_dark_h > 0).any() and (r.lit_fraction > 0).any()
