"""Scenes and checks shared by tests/test_oracle_model_paths.py (the C oracle) and tests/test_gpu_model.py (the HIP kernels):
a renderer under test is compared with the float64 model oracle/numpy_paths.py, per pixel with the spec's RNG, and held to
analytic known answers.  `render(scene, dem, color, bg, blocks)` -> (linear (H, W, 4), hits (H, W, 4), stats)."""
import functools

import numpy as np

import synth_np
from moonrtx_amd.scene import make_scene, named_scene
from oracle import numpy_paths

TOL = 1e-5                      # linear radiance, per pixel without a flagged sample (2^-10 / 100)
MAX_FLAGGED = 0.005             # of the samples: within a band of a decision (Sun-disk rim, environment texel edges) ...
MAX_FLAGGED_PIXELS = 0.1        # ... and of the pixels holding one (more samples per pixel, more chances)
SEGS = [(1, 1), (2, 2), (1, 3), (2, 4), (4, 4)]


@functools.lru_cache(maxsize=None)
def crater_dem():
    return synth_np.dem(360, 720, seed=5, craters=60)


@functools.lru_cache(maxsize=None)
def corrugated_dem():
    return synth_np.corrugated_dem(720, 1440)


@functools.lru_cache(maxsize=None)
def colour():
    return synth_np.colour_map(90, 180)


def env_texture(h=32, w=64):
    """Structure in both axes: red ramps with the azimuth, green with the elevation, blue is a one-texel checker (so a
    mirrored azimuth, a half-texel shift or a transposed lookup changes the value)."""
    r, c = np.mgrid[0:h, 0:w]
    out = np.empty((h, w, 4), np.uint8)
    out[..., 0] = 20 + (c * 197) // w
    out[..., 1] = 20 + (r * 211) // h
    out[..., 2] = np.where((r + c) % 2 == 0, 200, 60)
    out[..., 3] = 255
    return out


def paths_scene(seg, spp=16, width=48, height=24):
    """S1 with a colour map, an environment and a Sun disk right of the Moon: the frame's right edge sees it on primary
    misses, and continuation rays from the eastern half of the disc see it (it subtends ~20 degrees there)."""
    s = named_scene("S1", width, height, spp_per_launch=spp)
    s.sun_pos, s.sun_radius = (22.0, -20.0, 0.0), 8.0
    s.path_seg_min, s.path_seg_max = seg
    return s


def check_per_pixel(render, scene, dem, color, bg, blocks=2, strict=True, counted=True):
    """Renderer vs model with the spec's RNG.  strict: every pixel without a flagged sample within TOL, coverage equal,
    hit-buffer positions within the bound below; counted: the renderer counts samples.  Returns (linear, model).

    TOL is a bar on the MEAN of >= 16 samples: a single sample's hit may lie one final bisection bracket away from the
    model's (see the hit-buffer bound), which moves its radiance continuously by up to ~3e-5 on the crater relief."""
    assert blocks * scene.spp_per_launch >= 16
    lin, hits, st = render(scene, dem, color, bg, blocks)
    m = numpy_paths.render(scene, dem, color, bg, blocks=blocks)
    a = lin.astype(np.float64)
    d = np.abs(a[..., :3] - m["linear"][..., :3]).max(-1)
    fl = m["flagged"]
    assert a[..., :3].max() > 0.05, "scene rendered black: test is vacuous"
    if counted:
        assert st["primary_hits"] == m["stats"]["primary_hits"]
    if strict:
        assert m["sample_flagged"].mean() < MAX_FLAGGED and fl.mean() < MAX_FLAGGED_PIXELS, (fl.mean(), m["flag_counts"])
        assert d[~fl].max() < TOL, (d[~fl].max(), int((d[~fl] > TOL).sum()), m["flag_counts"])
    else:
        # steep relief: a hit one bisection bracket away (the spec's float32 entry and positions) turns the normal by up
        # to ~2e-3 rad, which the model cannot attribute per sample -- it may carry a shadow ray or a continuation ray
        # across a decision (what test_numpy_march_per_pixel_on_steep_terrain allows for the direct term)
        assert (d < TOL).mean() > 0.95 and np.median(d) < 1e-6, ((d < TOL).mean(), np.median(d))
        fl = np.zeros_like(fl)
        assert abs(a[..., :3].mean() - m["linear"][..., :3].mean()) < 2e-4 * m["linear"][..., :3].mean()
    # coverage: a count of samples, exact
    assert np.array_equal(a[~fl, 3], m["linear"][~fl, 3])
    # hit buffer (sample 0 of the last block): terrain hits differ along the ray by at most one final bisection bracket
    # plus the entry shift, plus the float32 rounding of a distance of ~290 (3e-5); Sun-disk hits by the spec's float32 root (bq^2 - c at 280 units: 1e-4 relative)
    ok = ~m["hit0_flagged"]
    hm = m["hits"]
    assert np.array_equal((hits[..., 3] > 0)[ok], (hm[..., 3] > 0)[ok])
    sun = ok & (np.linalg.norm(hm[..., :3] - np.asarray(scene.center), axis=-1) > 1.01 * scene.radius)
    ter = ok & (hm[..., 3] > 0) & ~sun
    dh = np.abs(hits.astype(np.float64) - hm).max(-1)
    assert ter.sum() > 100 and dh[ter].max() < numpy_paths.bracket(scene) + numpy_paths.ENTRY_SHIFT + 4e-5, dh[ter].max()
    if sun.any():
        assert (dh[sun] / hm[sun, 3]).max() < 1e-4
    return lin, m


# ---------------------------------------------------------------------------------------------- analytic known answers
def sphere_in_uniform_environment(render):
    """DEM = 1, a constant environment E, no direct light: every continuation ray from the convex sphere escapes and the
    cosine-weighted estimator of a constant radiance is exact, so EVERY sample is albedo * E on the disc and E off it:
    pixel = albedo E cov + E (1 - cov).  (2, 4) cannot reach its roulette: the same frame bit for bit."""
    dem = np.ones((90, 180), np.float32)
    E = 150
    bg = np.full((16, 32, 4), E, np.uint8)
    s = named_scene("S1", 40, 40, spp_per_launch=16)
    s.light_radiance, s.sun_radius = 0.0, 0.0
    s.const_albedo = (0.3, 0.5, 0.7)
    s.path_seg_min, s.path_seg_max = 2, 2
    lin, _, st = render(s, dem, None, bg, 1)
    e = np.float32(E) * np.float32(1 / 255)
    cov = lin[..., 3].astype(np.float64)
    alb = np.array(s.const_albedo, np.float32).astype(np.float64)
    want = alb * float(e) * cov[..., None] + float(e) * (1 - cov[..., None])
    assert 0.3 < cov.mean() < 0.9 and (cov == 1).sum() > 100 and (cov == 0).sum() > 100
    assert np.abs(lin[..., :3] - want).max() < 4e-7, np.abs(lin[..., :3] - want).max()
    assert st["bounce_rays"] == st["primary_hits"] > 0
    s.path_seg_max = 4
    lin4, _, st4 = render(s, dem, None, bg, 1)
    assert np.array_equal(lin4.view(np.uint32), lin.view(np.uint32))
    assert st4["bounce_rays"] == st4["primary_hits"] == st["primary_hits"]


def roulette_is_unbiased(render):
    """Russian roulette with 1/p: (2, 4) and (4, 4) (which has none) estimate the same mean.  Steep relief, a uniform bright
    environment and a high albedo make segments 3 and 4 carry a large share.  Per pixel the difference of the two frames
    has mean zero and only sampling noise (the scene cancels); its spread across pixels gives the z bound."""
    dem = corrugated_dem()
    bg = np.full((8, 16, 4), 255, np.uint8)
    s = named_scene("S1", 40, 40, spp_per_launch=64)
    s.light_radiance, s.sun_radius = 0.0, 0.0
    s.const_albedo = (0.6, 0.6, 0.6)
    s.vfov_deg = 1.2                                     # the corrugated limb region fills the frame
    s.target = (6.0, 0.0, 3.0)
    s.path_seg_min, s.path_seg_max = 4, 4
    a, _, sa = render(s, dem, None, bg, 1)
    s.path_seg_min, s.path_seg_max = 2, 4
    b, _, sb = render(s, dem, None, bg, 1)
    s.path_seg_min, s.path_seg_max = 2, 2
    c, _, _ = render(s, dem, None, bg, 1)
    on = (a[..., 3] == 1) & (b[..., 3] == 1)
    assert on.mean() > 0.9 and sb["bounce_rays"] < sa["bounce_rays"]
    x = (b[..., 0] - a[..., 0]).astype(np.float64)[on]
    z = x.mean() / (x.std(ddof=1) / np.sqrt(x.size))
    # segments 3-4 matter: the (2, 2) frame is well below, or the test could not see a missing 1/p
    y = (a[..., 0] - c[..., 0]).astype(np.float64)[on]
    assert y.mean() / (x.std(ddof=1) / np.sqrt(x.size)) > 30, y.mean()
    assert abs(z) < 4.0, z


def sun_disk_through_continuation_rays(render):
    """A smooth sphere, no environment, no direct light, a large Sun disk (radiance L) fully above the local horizon of the
    pixels compared: a Lambertian point sees it with projected solid angle pi sin^2(alpha) cos(theta), so its radiance is
    albedo L sin^2(alpha) cos(theta) (alpha: the disk's angular radius from the point, theta: from the normal to the disk
    centre).  Evaluated in float64 at sample 0's hit (an unbiased point of the pixel); the pixel differences from it are
    sampling noise with zero mean."""
    dem = np.ones((90, 180), np.float32)
    s = named_scene("S2", 48, 48, spp_per_launch=64)
    s.light_radiance = 0.0
    s.sun_pos, s.sun_radius, s.sun_radiance = (0.0, -2500.0, 0.0), 1500.0, 2.0      # behind the camera, facing the Moon
    s.path_seg_min, s.path_seg_max = 2, 2
    lin, hits, st = render(s, dem, None, None, 1)
    assert st["bounce_sun_hits"] > 0
    p = hits[..., :3].astype(np.float64) - np.asarray(s.center)
    n = p / np.linalg.norm(p, axis=-1, keepdims=True).clip(1e-9)
    to = np.asarray(s.sun_pos, float) - np.asarray(s.center, float) - p
    dist = np.linalg.norm(to, axis=-1)
    sin_a = s.sun_radius / dist
    cos_t = (n * to).sum(-1) / dist
    above = np.arccos(np.clip(cos_t, -1, 1)) + np.arcsin(np.clip(sin_a, 0, 1)) < np.radians(85.0)
    sel = (lin[..., 3] == 1) & above
    assert sel.sum() > 300
    alb = float(s.const_albedo[0])
    want = alb * s.sun_radiance * sin_a ** 2 * cos_t
    x = lin[..., 0].astype(np.float64)[sel] - want[sel]
    z = x.mean() / (x.std(ddof=1) / np.sqrt(x.size))
    assert abs(z) < 4.0 and abs(x.mean()) < 0.01 * want[sel].mean(), (z, x.mean(), want[sel].mean())


def colour_map_grid(render):
    """D4: a constant colour map c is const_albedo = c / 255 (to rounding); one marked cell of a 45 x 90 map over a 90 x 180
    DEM lights up exactly where ITS grid puts it (the bilinear convention of tests/golden/elevation_bilinear.json, on the
    colour map's own size): at 1 spp the hit buffer is the sample, so the albedo is predicted per pixel."""
    dem = np.ones((90, 180), np.float32)
    s = make_scene(64, 64, 0.0, 0.0, spp_per_launch=1, libration=(0, 0))
    s.vfov_deg = 1.2                                     # lat, lon within ~3 degrees of (0, 0)
    base = 50
    flat = np.full((45, 90, 4), base, np.uint8); flat[..., 3] = 255
    s.const_albedo = (base / 255.0,) * 3
    lc, _, _ = render(s, dem, None, None, 1)
    lm, hits, _ = render(s, dem, flat, None, 1)
    assert lc[..., 0].max() > 0.05
    assert np.allclose(lm[..., :3], lc[..., :3], rtol=1e-6, atol=0)
    mark = flat.copy()
    i, j = 22, 45                                        # row centre lat 0, column centre lon +2 degrees
    mark[i, j, :3] = 255
    lk, hits_k, _ = render(s, dem, mark, None, 1)
    ez = np.asarray(s.u, float); v0 = np.asarray(s.v, float); v0 = v0 - (v0 @ ez) * ez; v0 /= np.linalg.norm(v0)
    M = np.stack([np.cross(ez, v0), v0, ez])
    q = (hits_k[..., :3].astype(np.float64) - np.asarray(s.center)) @ M.T
    lat = np.arctan2(q[..., 2], np.hypot(q[..., 0], q[..., 1])); lon = np.arctan2(q[..., 0], q[..., 1])
    row = (np.pi / 2 - lat) / np.pi * 45 - 0.5
    col = (lon + np.pi) / (2 * np.pi) * 90 - 0.5
    wgt = np.clip(1 - np.abs(row - i), 0, 1) * np.clip(1 - np.abs(col - j), 0, 1)
    on = hits_k[..., 3] > 0
    ratio = np.where(lm[..., 0] > 0, lk[..., 0] / np.where(lm[..., 0] > 0, lm[..., 0], 1), 1.0)
    want = (base + (255 - base) * wgt) / base
    assert on.sum() > 1000 and (wgt[on] > 0.5).sum() > 20
    assert np.abs(ratio - want)[on & (lm[..., 0] > 1e-3)].max() < 2e-3
