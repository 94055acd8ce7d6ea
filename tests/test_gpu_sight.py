"""Terrain line of sight on the MI355X (DESIGN.md sections 3.12 and 4.13): the float64 model (tests/sight_model.py) on relief,
with a march step of several texels as well; the smooth sphere's closed forms; the bowl's rim; the bit-exact properties of
3.12; symmetry, and a tall mast on a peak behind a ridge; agreement with the horizons; the render state left alone; the
full-size DEM."""
import dataclasses
import math

import numpy as np
import pytest

import horizon_model as hm
import model_cases as mc
import sight_model as sm
import synth_np
from bowl_dem import bowl_dem, bowl_geometry
from common import assert_bit_equal
from moonrtx_amd import _lib
from moonrtx_amd.renderer import MoonRT, synth_ldem, dem_from_ldem
from moonrtx_amd.scene import named_scene
from test_gpu_illumination import make

pytestmark = pytest.mark.gpu

RM = 1737400.0          # metres of D = 1 for the synthetic DEMs
INF = float("inf")


def scene():
    return named_scene("S1", 16, 16)


def window(lat0, lon0, half, shape):
    la, lo = MoonRT.grid_nodes(lat=(lat0 + half, lat0 - half), lon=(lon0 - half, lon0 + half), shape=shape)
    LA, LO = np.meshgrid(la, lo, indexing="ij")
    return LA.ravel(), LO.ravel(), dict(lat=(lat0 + half, lat0 - half), lon=(lon0 - half, lon0 + half), shape=shape)


def coarse_case():
    """A march step of 3.4 texels: 720 x 1440 craters (texel 0.044 scene units) marched at 0.15."""
    s = dataclasses.replace(scene(), marching_step=0.15)
    return s, synth_np.dem(720, 1440, seed=9, craters=300)


CASES = {
    "craters": lambda: (scene(), mc.crater_dem(), (12.0, 30.0, 40.0), 5.0),
    "corrugated": lambda: (scene(), mc.corrugated_dem(), (-20.0, 100.0, 15.0), 2.0),
    "coarse-step": lambda: coarse_case() + ((5.0, -40.0, 300.0), 6.0),
}


# least unflagged shares, from the model alone on the CPU (craters / corrugated / coarse-step): 0.95 / 0.99 / 1.00 at
# n_bis = 0; at 12 the last probes graze the relief that decides them: 0.22 / 0.67 / 0.70
FLOORS = {("craters", 0): 0.9, ("corrugated", 0): 0.9, ("coarse-step", 0): 0.9,
          ("craters", 12): 0.15, ("corrugated", 12): 0.5, ("coarse-step", 12): 0.5}


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("n_bis", [0, 12])
def test_relief_matches_the_model(native_lib, name, n_bis):
    """Every unflagged target equals the model bit for bit (m at n_bis = 0 and 12), and so do the counters of the unflagged
    targets on their own."""
    s, dem, obs, half = CASES[name]()
    lat, lon, g = window(obs[0], obs[1], half, (16, 16))
    mast = 3000.0 if n_bis else 0.0
    m = sm.sight(s, dem, lat, lon, obs, target_h_m=2.0, mast_max_m=mast, n_bis=n_bis, radius_m=RM)
    rt = make(s, dem, 0)
    got = rt.viewshed(obs, target_height_m=2.0, mast_max_m=mast, n_bis=n_bis, radius_m=RM, **g).ravel()
    ok = ~m["flagged"]
    bad = np.flatnonzero(ok & (got != m["m"]))
    share = float((m["m"][ok] == 0).mean())
    print(f"{name} n_bis {n_bis}: unflagged {ok.mean():.3f}, in view {share:.3f}, finite {np.isfinite(m['m']).mean():.3f}")
    assert ok.mean() > FLOORS[name, n_bis], ok.mean()
    assert 0.0 < share < 1.0 or n_bis, share
    assert bad.size == 0, f"{bad.size} unflagged targets differ: {[(i, got[i], m['m'][i]) for i in bad[:6]]}"
    rt.close()
    # the counters, on the unflagged targets alone
    sel = np.flatnonzero(ok)[:40]
    m2 = sm.sight(s, dem, lat[sel], lon[sel], obs, target_h_m=2.0, mast_max_m=mast, n_bis=n_bis, radius_m=RM)
    assert not m2["flagged"].any()
    rt = make(s, dem, _lib.F_COUNT_STATS)
    st = {}
    got2 = rt.line_of_sight(lat[sel], lon[sel], obs, target_height_m=2.0, mast_max_m=mast, n_bis=n_bis, radius_m=RM, stats=st)
    rt.close()
    assert np.array_equal(got2, m2["m"])
    assert st["shadow_rays"] == m2["shadow_rays"], (st, m2["shadow_rays"])
    assert st["height_samples"] == m2["height_samples"], (st, m2["height_samples"])
    assert st["launches"] == 1 and st["dem_fetches"] > 0


def test_smooth_sphere(native_lib):
    """D = 0.999: visibility is the closed form outside the band a step's sag leaves; the mast height is the closed form
    within one final bisection step plus that sag."""
    s = scene()
    D = 0.999
    R = s.radius * D
    dem = np.full((180, 360), D, np.float32)
    rt = make(s, dem, 0)
    sag = s.marching_step ** 2 / (8 * R)
    for h_obs, h_t in ((0.0, 0.0), (2000.0, 0.0), (500.0, 3000.0)):
        a = s.scene_epsilon + float(sm.scene_height(s, h_obs, RM))
        b = s.scene_epsilon + float(sm.scene_height(s, h_t, RM))
        lim = math.degrees(math.acos(R / (R + a)) + math.acos(R / (R + b)))
        th = np.linspace(0.01, 2.0 * lim, 200)
        lat, lon = -th * 0.6, 30.0 + th * 0.8 / math.cos(0.0)     # off the equator, a great circle only roughly
        P = sm.raised(s, dem, lat, lon, np.full(th.size, h_t), RM)
        Q = sm.raised(s, dem, [0.0], [30.0], [h_obs], RM)[0]
        ang = np.arccos(np.clip((P @ Q) / np.linalg.norm(P, axis=1) / np.linalg.norm(Q), -1, 1))
        want = sm.sphere_visible(R, a, b, ang)
        low = np.array([chord_low(Q, p) for p in P])
        near = np.abs(low - R) < 4 * sag + 2e-5
        got = rt.line_of_sight(lat, lon, (0.0, 30.0, h_obs), target_height_m=h_t, radius_m=RM)
        assert set(np.unique(got).tolist()) <= {0.0, INF}
        assert np.array_equal((got == 0)[~near], want[~near]), (h_obs, h_t)
        assert (~near).sum() > 150
    # mast heights
    h_obs, mast, n_bis = 50.0, 20000.0, 12
    a = s.scene_epsilon + float(sm.scene_height(s, h_obs, RM))
    b = s.scene_epsilon
    lim = math.degrees(math.acos(R / (R + a)) + math.acos(R / (R + b)))
    th = np.linspace(lim * 1.2, lim * 3.0, 64)
    got = rt.line_of_sight(np.zeros(th.size), th, (0.0, 0.0, h_obs), mast_max_m=mast, n_bis=n_bis, radius_m=RM)
    rt.close()
    want = sm.sphere_mast(R, a, b, np.radians(th)) * RM / s.radius
    sag_m = 4 * sag * RM / s.radius + 1.0
    assert np.all(got >= want - sag_m) and np.all(got - want <= mast / 2 ** (n_bis - 1) + sag_m), (got - want)


def chord_low(A, B):
    t = B - A
    u = float(np.clip(-(A @ t) / (t @ t), 0.0, 1.0))
    return float(np.linalg.norm(A + u * t))


def test_bowl(native_lib):
    """From the floor of a spherical bowl: every node well inside the rim is in view, every node outside is not, and an
    outside node's mast is the grazing line over the rim's crest -- within the crest's blur of one texel and one step either
    side, and one final bisection step."""
    s = scene()
    h, w = 1440, 2880
    tc, dD = 6.0, 0.2
    dem = bowl_dem(h, w, 0.0, 0.0, tc, dD)
    obs = (0.0, 0.0, 100.0)
    rt = make(s, dem, 0)
    # inside, clear of the rim by 15 % of its radius
    lat, lon, g = window(0.0, 0.0, tc, (48, 48))
    ang = np.degrees(np.arccos(np.cos(np.radians(lat)) * np.cos(np.radians(lon))))
    vs = rt.viewshed(obs, radius_m=RM, **g).ravel()
    inside, outside = ang < 0.85 * tc, ang > tc * 1.02
    assert inside.sum() > 500 and outside.sum() > 200
    assert (vs[inside] == 0).all(), np.c_[lat, lon][inside & (vs != 0)][:5]
    assert (vs[outside] == INF).all(), np.c_[lat, lon][outside & (vs == 0)][:5]
    # masts along the equator east of the rim
    mast, n_bis = 80000.0, 14
    phi = np.linspace(tc * 1.05, tc * 1.6, 12)
    got = rt.line_of_sight(np.zeros(phi.size), phi, obs, mast_max_m=mast, n_bis=n_bis, radius_m=RM)
    rt.close()
    R = s.radius
    _, _, Rs, c0 = bowl_geometry(tc, dD)
    O = sm.raised(s, dem, [0.0], [0.0], [obs[2]], RM)[0]

    def profile(psi):       # the bowl's surface radius (units of R) at angle psi from the centre, on the sphere outside
        if psi >= math.radians(tc):
            return 1.0
        sn = math.sin(psi)
        return c0 * math.cos(psi) - math.sqrt(max(Rs * Rs - c0 * c0 * sn * sn, 0.0))

    def graze(psi, phi_t):  # the height over the target's base at which the line from O over the crest point at psi arrives
        C = R * profile(psi) * np.array([math.sin(psi), math.cos(psi), 0.0])
        T0 = sm.raised(s, dem, [0.0], [math.degrees(phi_t)], [0.0], RM)[0]
        u = np.array([math.sin(phi_t), math.cos(phi_t), 0.0])
        # O + k (C - O) = T0 + x u in the equatorial plane
        A = np.array([[(C - O)[0], -u[0]], [(C - O)[1], -u[1]]])
        k, x = np.linalg.solve(A, (T0 - O)[:2])
        return x * RM / R
    blur = (math.pi / h + s.marching_step / R)          # one texel and one step, radians
    res = mast / 2 ** (n_bis - 1)
    for p, m in zip(np.radians(phi), got):
        cands = [graze(math.radians(tc) + f * blur, p) for f in np.linspace(-1.0, 1.0, 41)]
        lo_, hi_ = min(cands), max(cands)
        assert np.isfinite(m) and lo_ - res <= m <= hi_ + res, (math.degrees(p), m, lo_, hi_)


def test_bit_exact_properties(native_lib):
    """Bands concatenate to the map and points on nodes are the nodes; a target does not depend on the others; production
    and counting builds, WIDE addressing and no skipping agree; the bisection nests; m == 0 is the n_bis = 0 call."""
    s = scene()
    dem = mc.corrugated_dem()
    obs = (-10.0, 60.0, 1000.0)
    lat, lon, g = window(-10.0, 60.0, 3.0, (24, 40))
    args = dict(target_height_m=1.5, mast_max_m=4000.0, n_bis=9, radius_m=RM)
    ref = None
    for flags in (0, _lib.F_COUNT_STATS, _lib.F_FORCE_WIDE, _lib.F_NO_SKIP, _lib.F_COUNT_STATS | _lib.F_FORCE_WIDE | _lib.F_NO_SKIP):
        rt = make(s, dem, flags)
        a = rt.viewshed(obs, **g, **args)
        if ref is None:
            ref = a
            # the model alone on the CPU: 0.11 in view, 0.55 within mast_max
            assert 0.05 < (a == 0).mean() < 0.95 and 0.2 < np.isfinite(a).mean() < 0.9
        assert_bit_equal(a, ref, f"flags {flags} against production")
        bands = np.concatenate([rt.viewshed(obs, rows=(r, min(r + 7, 24)), **g, **args) for r in range(0, 24, 7)])
        assert_bit_equal(bands, a, f"flags {flags}: bands")
        pts = rt.line_of_sight(lat, lon, obs, **args)
        assert_bit_equal(pts, a.ravel(), f"flags {flags}: points on nodes")
        perm = np.random.default_rng(flags).permutation(lat.size)
        assert_bit_equal(rt.line_of_sight(lat[perm], lon[perm], obs, **args), pts[perm], f"flags {flags}: order")
        assert_bit_equal(rt.line_of_sight(lat[100:101], lon[100:101], obs, **args), pts[100:101], f"flags {flags}: alone")
        per = np.tile(np.asarray(obs), (lat.size, 1))
        assert_bit_equal(rt.line_of_sight(lat, lon, per, **args), pts, f"flags {flags}: one observer per target")
        if flags == 0:
            # bisection nesting: t at n_bis + 1 is t at n_bis or that minus 2^-n_bis (t = m / mast_max, dyadic)
            for nb in (1, 5, 9):
                a0 = rt.viewshed(obs, **g, **dict(args, n_bis=nb)).astype(np.float64)
                a1 = rt.viewshed(obs, **g, **dict(args, n_bis=nb + 1)).astype(np.float64)
                assert np.array_equal(a0 == 0, a1 == 0) and np.array_equal(np.isinf(a0), np.isinf(a1))
                f = np.isfinite(a0) & (a0 > 0)
                t0 = np.round(a0[f] / args["mast_max_m"] * 2 ** 24) / 2 ** 24
                t1 = np.round(a1[f] / args["mast_max_m"] * 2 ** 24) / 2 ** 24
                assert ((t1 == t0) | (t1 == t0 - 2.0 ** -nb)).all(), nb
            z = rt.viewshed(obs, **g, **dict(args, n_bis=0, mast_max_m=0.0))
            assert set(np.unique(z).tolist()) <= {0.0, INF}
            assert np.array_equal(z == 0, a == 0)
        rt.close()


def test_symmetry(native_lib):
    """n_bis = 0: swapping the observer and the target, with their heights, gives the same bits (away from |O|^2 = |T|^2)."""
    s = scene()
    dem = mc.crater_dem()
    rng = np.random.default_rng(4)
    n = 256
    la1, lo1 = rng.uniform(-40, 40, n), rng.uniform(0, 60, n)
    la2, lo2 = la1 + rng.uniform(-1.5, 1.5, n), lo1 + rng.uniform(-1.5, 1.5, n)
    rt = make(s, dem, 0)
    seen = []
    for h1, h2 in ((0.0, 0.0), (3.0, 150.0), (60.0, 10.0)):
        fw = rt.line_of_sight(la1, lo1, np.c_[la2, lo2, np.full(n, h2)], target_height_m=h1, radius_m=RM)
        bw = rt.line_of_sight(la2, lo2, np.c_[la1, lo1, np.full(n, h1)], target_height_m=h2, radius_m=RM)
        P1 = sm.raised(s, dem, la1, lo1, np.full(n, h1), RM)
        P2 = sm.raised(s, dem, la2, lo2, np.full(n, h2), RM)
        tie = np.abs(np.linalg.norm(P1, axis=1) - np.linalg.norm(P2, axis=1)) < 1e-5
        assert_bit_equal(fw[~tie], bw[~tie], f"heights {h1}, {h2}")
        seen.append(fw == 0)
    rt.close()
    assert 0.1 < np.mean(seen) < 0.9, np.mean(seen)      # both answers occur (the model alone: 0.14 at ground level)


def peak_ridge_dem(ridge=True):
    """The equator: a 9 km peak (D = 1) about lon 0, a 5 km ridge along lon 1 (ridge=True), D = 0.995 elsewhere."""
    h, w = 720, 1440
    lat = 90 - (np.arange(h) + 0.5) * (180 / h)
    lon = -180 + (np.arange(w) + 0.5) * (360 / w)
    LA, LO = np.meshgrid(lat, lon, indexing="ij")
    D = np.full((h, w), 0.995, np.float32)
    D[(np.abs(LA) < 1.0) & (np.abs(LO) < 0.5)] = 1.0
    if ridge:
        D[(np.abs(LA) < 6.0) & (np.abs(LO - 1.5) < 0.3)] = 0.998
    return D


def test_tall_mast_on_a_peak_behind_a_ridge(native_lib):
    """A 2 km mast on the peak, a target on the plain 3 degrees east, a ridge between: blocked whichever end observes.  (A
    march from the mast's end, outside the bounding sphere and heading down, would end at its first step and call it clear.)
    Without the ridge both see each other."""
    s = scene()
    for ridge in (True, False):
        rt = make(s, peak_ridge_dem(ridge), 0)
        a = rt.line_of_sight([0.0], [3.0], (0.0, 0.0, 2000.0), radius_m=RM)[0]
        b = rt.line_of_sight([0.0], [0.0], (0.0, 3.0, 0.0), target_height_m=2000.0, radius_m=RM)[0]
        rt.close()
        assert a == b == (INF if ridge else 0.0), (ridge, a, b)


def test_agrees_with_the_horizon(native_lib):
    """An observer ~1e8 m out along azimuth a and elevation e from each target is in view iff e is above the target's horizon
    at a -- except within one horizon bisection step, for the model's flagged targets, and where n . d <= 0 (a horizon probe
    refuses such a direction; the line of sight marches it)."""
    s = scene()
    dem = mc.crater_dem()
    rng = np.random.default_rng(8)
    n, n_az, n_bis = 200, 64, 14
    lat, lon = rng.uniform(-50, 50, n), rng.uniform(-180, 180, n)
    az = rng.integers(0, n_az, n)
    rt = make(s, dem, 0)
    hz = rt.horizon(lat, lon, n_az=n_az, n_bis=n_bis)[np.arange(n), az].astype(np.float64)
    e = hz + rng.uniform(-6.0, 6.0, n)
    o, nrm, U, N, E = hm.frame(s, dem, lat, lon)
    phi = 2 * np.pi * az / n_az
    er = np.radians(e)
    d = (np.cos(er) * np.cos(phi))[:, None] * N + (np.cos(er) * np.sin(phi))[:, None] * E + np.sin(er)[:, None] * U
    Q = o + 600.0 * d
    ql = np.degrees(np.arctan2(Q[:, 2], np.hypot(Q[:, 0], Q[:, 1])))
    qo = np.degrees(np.arctan2(Q[:, 0], Q[:, 1]))
    oq, uq = sm.ends(s, dem, ql, qo)
    hq = ((Q - oq) * uq).sum(1) / s.radius * RM
    assert (hq > 5e7).all() and (hq < 1.1e9).all()
    obs = np.c_[ql, qo, hq]
    got = rt.line_of_sight(lat, lon, obs, radius_m=RM)
    rt.close()
    m = sm.sight(s, dem, lat, lon, obs, radius_m=RM)
    step = hm.bisection_step_deg(n_bis)
    cos_nd = (nrm * d).sum(1)
    keep = (np.abs(e - hz) > step + 1e-3) & ~m["flagged"] & (cos_nd > 1e-3)
    assert keep.sum() > 0.35 * n, keep.sum()      # the model alone on the CPU: 0.45
    want = e > hz
    assert np.array_equal((got == 0)[keep], want[keep]), np.c_[lat, lon, e, hz, got][keep & ((got == 0) != want)][:5]


def test_leaves_the_render_state_alone(native_lib):
    s = scene().with_size(48, 32, spp_per_launch=16)
    dem = mc.crater_dem()

    def run(with_sight):
        rt = make(s, dem, _lib.F_COUNT_STATS)
        st1 = rt.render(1)
        if with_sight:
            rt.viewshed((10.0, 20.0, 50.0), lat=(15, 5), lon=(15, 25), shape=(16, 16), mast_max_m=1000.0, n_bis=6, radius_m=RM)
            rt.line_of_sight([1.0, 2.0], [3.0, 4.0], (0.0, 0.0, 1e8), radius_m=RM)
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


def test_full_size(native_lib):
    """The headline DEM (23040 x 46080, WIDE addressing): a 1024 x 1024 viewshed about a local observer, at n_bis = 0 and 12."""
    DEM_H, DEM_W = 23040, 46080
    src = synth_ldem(DEM_H, DEM_W)
    dem, scale = dem_from_ldem(src, DEM_H, DEM_W, 1)
    src.free()
    rt = MoonRT(16, 16)
    rt.bind_dem(dem, DEM_H, DEM_W)
    rt.apply_scene(scene())
    rt.set_params(flags=0)
    obs = (-45.0, 30.0, 10.0)
    g = dict(lat=(-44.0, -46.0), lon=(28.6, 31.4), shape=(1024, 1024))
    st = {}
    v0 = rt.viewshed(obs, radius_m=1737400.0 * scale, stats=st, **g)
    st12 = {}
    v12 = rt.viewshed(obs, mast_max_m=2000.0, n_bis=12, radius_m=1737400.0 * scale, stats=st12, **g)
    rt.close()
    dem.free()
    share = float((v0 == 0).mean())
    print(f"full size: in view {share:.3f} ({st['kernel_ms']:.2f} ms), with masts up to 2 km: "
          f"{float(np.isfinite(v12).mean()):.3f} ({st12['kernel_ms']:.2f} ms)")
    assert v0.shape == v12.shape == (1024, 1024)
    assert set(np.unique(v0).tolist()) <= {0.0, INF}
    assert 0.001 < share < 0.999
    assert np.array_equal(v12 == 0, v0 == 0)
    fin = v12[np.isfinite(v12)]
    assert (fin >= 0).all() and (fin <= 2000.0).all() and np.isfinite(v12).mean() > share
