"""Sun illumination over many dates on the MI355X (DESIGN.md sections 3.7 and 4.9): the series against a per-date loop of
illumination_at bit for bit, against the float64 model, terrain_sun_events on the smooth sphere and behind a plateau, the
render state left alone, and the full-size DEM."""
import math
from datetime import datetime, timedelta, timezone

import numpy as np
import pytest

import illum_model as im
import model_cases as mc
from common import assert_bit_equal
from moonrtx_amd import _lib
from moonrtx_amd import ephemeris as E
from moonrtx_amd.renderer import MoonRT, synth_ldem, dem_from_ldem
from moonrtx_amd.scene import named_scene
from moonrtx_amd.sunlight import terrain_sun_events
from test_gpu_illumination import make, mu_tol, plateau_dem

pytestmark = pytest.mark.gpu

OBS = E.Observer(52.2, 21.0, 0.0)
T0 = datetime(2025, 3, 7, 21, 0, tzinfo=timezone.utc)
COUNTERS = ("shadow_rays", "height_samples", "dem_fetches", "mip_fetches")


class Epoch:
    """An epoch row as the attributes illum_model and MoonRT read (the light and Moon frame of one date)."""
    def __init__(self, row, base):
        self.light_pos, self.light_radius, self.light_radiance = row[0:3], row[3], row[4]
        self.center, self.u, self.v = row[5:8], row[8:11], row[11:14]
        self.radius, self.scene_epsilon, self.marching_step = base.radius, base.scene_epsilon, base.marching_step


def loop(rt, radius, lat, lon, ep, first, count, n_sun, stats):
    """What the series promises, computed the old way: per epoch set_moon_frame + set_light + illumination_at."""
    N = len(lat)
    f = np.zeros(N, int) if first is None else np.asarray(first)
    out = np.empty((N, count, 4), np.float32)
    for k in range(ep.shape[0]):
        p = np.flatnonzero((f <= k) & (k < f + count))
        if p.size == 0:
            continue
        rt.set_moon_frame(ep[k, 5:8], radius, ep[k, 8:11], ep[k, 11:14])
        rt.set_light(ep[k, 0:3], ep[k, 3], ep[k, 4])
        out[p, k - f[p]] = rt.illumination_at(lat[p], lon[p], n_sun=n_sun, stats=stats)
    return out


def terminator_points(ep0, n, rng, spread=10.0):
    """n points scattered around both terminators of the first epoch (so that an hourly series crosses them)."""
    class S:
        light_pos, center, u, v = ep0[0:3], ep0[5:8], ep0[8:11], ep0[11:14]
    la0, lo0 = im.subsolar_latlon(S)
    side = np.where(rng.random(n) < 0.5, 90.0, -90.0)
    return rng.uniform(-50.0, 50.0, n), lo0 + side + rng.uniform(-spread, spread, n)


def cases(rng, ep):
    """(name, lat, lon, first, count): the full product with repeated points and points on a map's nodes; random windows
    whose length is no multiple of 64/n; one point; short windows (a wave spans several points)."""
    m = ep.shape[0]
    la, lo = terminator_points(ep[0], 9, rng)
    gl, gn = MoonRT.grid_nodes((30.0, -30.0), (lo[0] - 6.0, lo[0] + 6.0), (3, 4))
    GL, GN = np.meshgrid(gl, gn, indexing="ij")
    lat = np.concatenate([la, GL.ravel()[:4], la[:3]])                    # repeats
    lon = np.concatenate([lo, GN.ravel()[:4], lo[:3]])
    n = lat.size
    yield "full product", lat, lon, None, m
    yield "windows", lat, lon, rng.integers(0, m - 37 + 1, n), 37
    yield "one point", lat[:1], lon[:1], np.array([m - 5]), 5
    yield "short windows", lat, lon, rng.integers(0, m - 3 + 1, n), 3


@pytest.fixture(scope="module")
def relief():
    s = named_scene("S1", 16, 16)
    ep = E.sun_epochs([T0 + timedelta(hours=h) for h in range(40)], OBS)
    return s, mc.crater_dem(), ep


@pytest.mark.parametrize("n_sun", [1, 4, 16, 64])
def test_series_equals_the_per_date_loop_bit_for_bit(native_lib, relief, n_sun):
    s, dem, ep = relief
    for flags in (0, _lib.F_COUNT_STATS, _lib.F_FORCE_WIDE, _lib.F_FORCE_WIDE | _lib.F_COUNT_STATS):
        rng = np.random.default_rng(7 + n_sun)
        rt = make(s, dem, flags)
        lit_seen, rays = set(), 0
        for name, lat, lon, first, count in cases(rng, ep):
            st_s, st_l = {}, {}
            got = rt.illumination_series(lat, lon, ep, n_sun=n_sun, first=first, count=count, stats=st_s)
            want = loop(rt, s.radius, lat, lon, ep, first, count, n_sun, st_l)
            assert_bit_equal(got, want, f"series vs loop: {name}, n_sun {n_sun}, flags {flags}")
            for k in COUNTERS:
                assert st_s[k] == st_l[k], (name, k, st_s, st_l)
            rays += st_s["shadow_rays"]
            lit_seen |= set(np.unique(got[..., 0] > 0).tolist())
        assert (rays > 0) == bool(flags & _lib.F_COUNT_STATS)    # (a lone point may see no Sun in its window)
        assert lit_seen == {False, True}      # the windows cross a terminator
        rt.close()


def test_series_matches_the_model_on_relief(native_lib):
    """crater and egg-crate DEMs, 24 hourly dates, points around both terminators: lit is the model's per (point, epoch)
    except where a sample is flagged; mu and irr agree within mu_tol."""
    s = named_scene("S1", 16, 16)
    ep = E.sun_epochs([T0 + timedelta(hours=2 * h) for h in range(24)], OBS)
    samples = MoonRT.sun_samples(16).astype(np.float64)
    rng = np.random.default_rng(11)
    lat, lon = terminator_points(ep[0], 12, rng, spread=14.0)
    kinds = set()
    for name, dem in (("craters", mc.crater_dem()), ("egg-crate", mc.corrugated_dem())):
        rt = make(s, dem, 0)
        got = rt.illumination_series(lat, lon, ep, n_sun=16)
        rt.close()
        flagged = total = 0
        for k in range(ep.shape[0]):
            e = Epoch(ep[k], s)
            m = im.illuminate(e, dem, lat, lon, samples)
            ok = ~m["flagged"].any(1)
            flagged += int((~ok).sum()); total += ok.size
            g = got[:, k]
            assert np.array_equal(g[ok, 0], m["lit"][ok].astype(np.float32)), (name, k)
            Lb, _ = im.sun_dir_moon_frame(e)
            sin2 = (e.light_radius / np.linalg.norm(Lb)) ** 2
            full = 2 * e.light_radiance * sin2 / (1 + math.sqrt(1 - sin2))
            tol = mu_tol(dem.shape, lat)
            assert (np.abs(g[:, 2] - m["mu"]) < tol).all(), (name, k)
            assert (np.abs(g[ok, 1] - m["irr"][ok]) < tol[ok] * full).all(), (name, k)
            kinds |= {0.0 if x == 0 else 1.0 if x == 1 else 0.5 for x in g[:, 0]}
        print(f"{name}: flagged (point, epoch) pairs {flagged / total:.2%}")
        assert flagged < 0.2 * total
    assert {0.0, 1.0} <= kinds


def first_light_date(lon_target, start):
    """The first hour after `start` at which the subsolar longitude has fallen below lon_target (degrees)."""
    prev = None
    for h in range(24 * 31):
        t = start + timedelta(hours=h)
        d = (E.calculate_moon_ephemeris(t, False, OBS).subsolar_lon - lon_target + 180.0) % 360.0 - 180.0
        if prev is not None and prev >= 0.0 > d and abs(d) < 10.0:
            return t
        prev = d
    raise AssertionError("no crossing within a month")


def model_state(s, dem, lat, lon, t, n_sun):
    e = Epoch(E.sun_epochs([t], OBS)[0], s)
    m = im.illuminate(e, dem, [lat], [lon], MoonRT.sun_samples(n_sun).astype(np.float64))
    return m["lit"][0], bool(m["flagged"].any())


def test_sun_events_on_the_smooth_sphere(native_lib):
    """D = 1: at both ends of every bracket the float64 model shows the old state at t_lo and the new one at t_hi (unless
    flagged); first_light and full_disc happen with the sphere's Sun altitude within the Sun's radius of 0."""
    s = named_scene("S1", 16, 16)
    dem = np.ones((90, 180), np.float32)
    rt = make(s, dem, 0)
    ep0 = E.sun_epochs([T0], OBS)[0]
    class S0:
        light_pos, center, u, v = ep0[0:3], ep0[5:8], ep0[8:11], ep0[11:14]
    la0, lo0 = im.subsolar_latlon(S0)
    # morning terminator 90 deg east of the subsolar point moves west ~0.5 deg/h: points a few degrees west of it rise
    lat = np.array([0.0, 20.0, -35.0, 5.0, 0.0, -10.0])
    lon = np.array([lo0 + 88.0, lo0 + 86.0, lo0 + 89.0, lo0 - 91.0, lo0 - 92.5, lo0 - 94.0])
    res = terrain_sun_events(rt, lat, lon, T0, 0.5, step_min=10, n_sun=16, refine=15, observer=OBS)
    rt.close()
    kinds = {e.kind for e in res.events}
    assert kinds == {"first_light", "full_disc", "disc_cut", "last_light"}, kinds
    r_sun = math.degrees(math.asin(ep0[3] / np.linalg.norm(ep0[0:3] - ep0[5:8])))
    rate = 0.6 / 60.0 * 10.0 / 16.0          # deg of Sun altitude per refined bracket, an upper bound
    for e in res.events:
        assert not e.flicker, e
        rising = e.kind in ("first_light", "full_disc")
        state = (lambda x: x > 0) if e.kind in ("first_light", "last_light") else (lambda x: x == 1)
        lo_lit, lo_fl = model_state(s, dem, lat[e.point], lon[e.point], e.t_lo, 16)
        hi_lit, hi_fl = model_state(s, dem, lat[e.point], lon[e.point], e.t_hi, 16)
        if not lo_fl:
            assert state(lo_lit) != rising, (e, lo_lit)
        if not hi_fl:
            assert state(hi_lit) == rising, (e, hi_lit)
        if e.kind in ("first_light", "full_disc"):
            assert abs(e.sun_alt_sphere) <= r_sun + 0.05 + rate, e
    fl = [e for e in res.events if e.kind == "first_light"]
    fd = [e for e in res.events if e.kind == "full_disc"]
    assert fl and fd and all(e.sun_alt_sphere < 0 for e in fl) and all(e.sun_alt_sphere > 0 for e in fd)
    print(f"{len(res.events)} events; first light at sphere altitude {[round(e.sun_alt_sphere, 3) for e in fl]}, full disc at "
          f"{[round(e.sun_alt_sphere, 3) for e in fd]} (Sun radius {r_sun:.3f} deg)")


def test_first_light_behind_a_plateau(native_lib):
    """The plateau of test_shadow_length_of_a_plateau (lon -20..0, |lat| <= 30, 10 km): a point on the equator 5 deg west of
    it sees the point-light Sun (n_sun = 1) rise over the plateau later than on the bare sphere, by the plateau's angular
    height seen from the point -- within one bracket, one texel and one march step of the edge."""
    h, w, H_km = 1440, 2880, 10.0
    s = named_scene("S1", 16, 16)
    R = s.radius
    lon_p = -25.0
    start = first_light_date(lon_p + 90.0 + 1.0, datetime(2025, 3, 1, tzinfo=timezone.utc)) - timedelta(hours=2)
    times = {}
    for name, dem in (("sphere", np.ones((h, w), np.float32)), ("plateau", plateau_dem(h, w, -20.0, 0.0, 30.0, H_km))):
        rt = make(s, dem, 0)
        res = terrain_sun_events(rt, [0.0], [lon_p], start, 0.5, step_min=10, n_sun=1, refine=15, observer=OBS)
        rt.close()
        fl = [e for e in res.events if e.kind == "first_light"]
        assert len(fl) == 1 and not fl[0].flicker, res.events
        times[name] = fl[0]
    D0 = 1.0 / (1.0 + H_km / 1737.4)

    def elevation(edge_deg):     # the plateau's west top edge seen from the lifted base point, degrees above the horizon
        ph, pe = math.radians(lon_p), math.radians(edge_deg)
        q = (R * D0 + s.scene_epsilon) * np.array([math.sin(ph), math.cos(ph)])
        d = R * np.array([math.sin(pe), math.cos(pe)]) - q
        up, east = q / np.linalg.norm(q), np.array([math.cos(ph), -math.sin(ph)])
        return math.degrees(math.atan2(d @ up, d @ east))
    tol_lon = 360.0 / w + math.degrees(s.marching_step / R)
    lo, hi = elevation(-20.0 + tol_lon), elevation(-20.0 - tol_lon)
    bracket = 0.6 / 60.0 * 10.0 / 16.0
    delay = times["plateau"].sun_alt_sphere - times["sphere"].sun_alt_sphere
    print(f"first light: sphere at {times['sphere'].sun_alt_sphere:.4f} deg, plateau at {times['plateau'].sun_alt_sphere:.4f} deg; "
          f"delay {delay:.4f} deg, angular height {elevation(-20.0):.4f} deg [{lo:.4f}, {hi:.4f}]")
    assert times["plateau"].t_lo > times["sphere"].t_hi
    assert abs(times["sphere"].sun_alt_sphere) < 0.05 + bracket
    assert lo - 2 * bracket - 0.01 <= delay <= hi + 2 * bracket + 0.01


def test_series_leaves_the_context_state_alone(native_lib, relief):
    s, dem, ep = relief
    s = s.with_size(48, 32, spp_per_launch=16)
    lat, lon = np.array([10.0, -20.0, 33.0]), np.array([20.0, 95.0, -80.0])

    def run(with_series):
        rt = make(s, dem, _lib.F_COUNT_STATS)
        st1 = rt.render(1)
        if with_series:
            rt.illumination_series(lat, lon, ep, n_sun=16)
            rt.illumination_series(lat, lon, ep, n_sun=4, first=[0, 5, 9], count=7)
        pt = rt.illumination_at(lat, lon, n_sun=16)
        st2 = rt.render(1)
        out = rt.read_linear(), rt.read_hits(), rt.samples_done(), st1, st2, pt
        rt.close()
        return out
    a, b = run(False), run(True)
    assert_bit_equal(b[0], a[0], "linear radiance")
    assert_bit_equal(b[1], a[1], "hit buffer")
    assert_bit_equal(b[5], a[5], "illumination_at after a series")
    assert b[2] == a[2] == 32
    for k in ("primary_hits", "shadow_rays", "height_samples", "bounce_rays"):
        assert b[4][k] == a[4][k], k


def test_full_size_month_of_dates(native_lib):
    """DESIGN.md 4.9's case: the headline DEM (23040 x 46080), 1024 random points over the whole Moon, 30 days at 10-minute
    steps (4321 epochs), n_sun = 16; 16 random (point, epoch) entries equal illumination_at bit for bit."""
    DEM_H, DEM_W = 23040, 46080
    src = synth_ldem(DEM_H, DEM_W)
    dem, _ = dem_from_ldem(src, DEM_H, DEM_W, 1)
    src.free()
    s = named_scene("S1", 16, 16)
    rt = MoonRT(16, 16)
    rt.bind_dem(dem, DEM_H, DEM_W)
    rt.apply_scene(s)
    rt.set_params(flags=0)
    rng = np.random.default_rng(2025)
    lat = np.degrees(np.arcsin(rng.uniform(-1.0, 1.0, 1024)))
    lon = rng.uniform(-180.0, 180.0, 1024)
    ep = E.sun_epochs([datetime(2025, 3, 1, tzinfo=timezone.utc) + timedelta(minutes=10 * k) for k in range(4321)], OBS)
    st = {}
    got = rt.illumination_series(lat, lon, ep, n_sun=16, stats=st)
    print(f"1024 points x 4321 epochs x 16 Sun samples: {st['kernel_ms']:.2f} ms in {st['launches']} launch(es)")
    assert got.shape == (1024, 4321, 4) and np.isfinite(got).all()
    assert 0.3 < (got[..., 0] > 0).mean() < 0.7 and got[..., 0].max() == 1.0
    for p, k in zip(rng.integers(0, 1024, 16), rng.integers(0, 4321, 16)):
        rt.set_moon_frame(ep[k, 5:8], s.radius, ep[k, 8:11], ep[k, 11:14])
        rt.set_light(ep[k, 0:3], ep[k, 3], ep[k, 4])
        assert_bit_equal(got[p, k][None], rt.illumination_at(lat[p:p + 1], lon[p:p + 1], n_sun=16), f"entry ({p}, {k})")
    rt.close()
    dem.free()
