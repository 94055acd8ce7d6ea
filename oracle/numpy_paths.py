"""numpy model of the FULL sample: camera ray, march, colour texture, light sample, path continuation, environment,
Sun disk, coverage and hit buffer (TEST INFRASTRUCTURE, NOT PRODUCT).

The independent restatement of SURVEY.md section 2.1 rows D4-D10 / DESIGN.md section 3.3 that oracle/numpy_march.py
is for D1-D5 with constant albedo.  Written from the model statements, not from the C: float64 throughout, library
trig, exact (lat, lon) and texel coordinates at every march step and bisection point, a ray-sphere test for the Sun
disk.  An error in the arithmetic spec is shared by the C oracle and the HIP kernels; against this model it shows.

    D4  albedo = bilinear RGBA8 colour map at the hit's (lat, lon) on the map's OWN grid, / 255 (const_albedo without one)
    D5  one uniform sample of the cone the light sphere subtends, from p + scene_epsilon n; shadow ray marched to r > R
    D6  after the light sample at vertex i: throughput *= albedo; beyond path_seg_min Russian roulette with
        p = min(max(albedo), 1) and throughput /= p; a cosine-weighted direction about the normal (r = sqrt(u));
        marched like a shadow ray; a hit is bisected and gets its own normal, albedo and light sample;
        uniforms at dims 4 + 5 (i - 1) + {0: roulette, 1, 2: direction, 3, 4: light sample}
    D7  a primary miss, or a continuation ray that leaves the bounding sphere, sees the nearest environment texel by the
        scene-frame direction's elevation el = atan2(z, hypot(x, y)) and azimuth az = atan2(x, y) (the DEM's lat / lon
        convention): row = floor((pi/2 - el) / pi * h), col = floor((az + pi) / (2 pi) * w) mod w
    D8  the flat Sun-disk sphere: on a primary miss (ray-sphere test from the eye; coverage 1, hit buffer = the disk
        point) and on a continuation ray that leaves (tested before the environment); shadow rays pass through it
    D9  mean over blocks * S samples of (r, g, b, coverage); sample gs = block * S + i
    D10 hit buffer: sample 0 of the last block, scene coordinates and distance from the eye

Every sample also records how close it came to each discrete decision: a march step that touches the surface, the
bounding sphere's exit, the light's cos > 0, Russian roulette's u < p, the Sun disk's |q| < r, an environment texel
boundary (and, recorded only, a bisection point against the surface).  A sample within the band of one may
legitimately come out the other way in float32; `render` returns these samples so tests exclude exactly their pixels,
and counts them.
"""
import numpy as np

from oracle.numpy_march import _dem_bilinear, _duff_basis, spec_uniforms

# Half-widths of the bands about each decision.  Lengths are in scene units (R = 10 for the Moon: 1e-5 = 1.7 m): the spec
# marches from the float32 sphere entry (moved ALONG the ray by <= 2e-5) in float32 positions with quadratic texel
# coordinates; the others are a generous multiple of the float32 resolution of the compared quantity.
BANDS = dict(
    march=3e-5,         # |r - R D| at a step where the ray touches the surface (see _march)
    exit=3e-5,          # |r - R| (primary: |s - smax|) at a step that is near the surface as well
    cosine=2e-6,        # n . w of the light sample against 0
    roulette=2e-6,      # u against p
    sun=2e-3,           # |q|^2 against r^2, relative to r^2 (the spec's primary test is bq^2 - c in float32 at 280 units)
    env=1e-4,           # distance of the texel coordinates from a texel boundary, in texels
    bisect=1e-6,        # |r - R D| at a bisection point: RECORDED, not excluded -- a flip next to the crossing moves the
)                       # hit by less than one final bracket (step / 2^nbis) and the radiance continuously
EXCLUDED = ("march", "exit", "cosine", "roulette", "sun", "env")
KINDS = tuple(BANDS)
ENTRY_SHIFT = 2e-5      # the spec's float32 sphere entry lies up to this far ALONG the ray from the exact one


def bracket(scene):
    """Width of the final bisection bracket, step / 2^nbis."""
    w = scene.marching_step
    while w > scene.marching_step_eps:
        w *= 0.5
    return w


def _norm(v):
    return np.sqrt((v * v).sum(-1))


def _latlon(p):
    return np.arctan2(p[..., 2], np.hypot(p[..., 0], p[..., 1])), np.arctan2(p[..., 0], p[..., 1])


def _surface_margin(dem, R, q):
    """r - R D(lat, lon): <= 0 is at or below the surface."""
    lat, lon = _latlon(q)
    return _norm(q) - R * _dem_bilinear(dem, lat, lon)


class _Flags:
    """Per-sample record of the nearest approach to each decision, as a multiple of its band (< 1 = inside)."""

    def __init__(self, n, bands):
        self.bands = bands
        self.near = {k: np.full(n, np.inf) for k in KINDS}

    def note(self, kind, idx, dist, slack=0.0):
        """dist: distance of each sample from the decision; slack: how far the model's own input to it may be off."""
        if idx.size:
            np.minimum.at(self.near[kind], idx, np.maximum(np.abs(dist) - slack, 0.0) / self.bands[kind])

    def flagged(self):
        return {k: v < 1.0 for k, v in self.near.items()}


def _march(dem, R, step, o, d, idx, flags, smax=None):
    """Steps s_k = k step, k = 1, 2, ... from o along unit d while inside (primary: s_k <= smax; otherwise |q| <= R); the
    first step at / below the surface is a hit.  Returns (hit, k).  idx = sample index of each ray (for the flags).

    A step within the band of the surface is a DISCRETE decision only if the ray touches the surface there: a step just
    above the surface that the next step does not follow below it, or a hit step that the next step does not follow
    deeper.  A near-zero step next to a real crossing merely moves the bracket by one step; the bisection then finds the
    same crossing (what tests compare to 1e-5)."""
    band = flags.bands["march"]
    n = len(o)
    hit = np.zeros(n, bool)
    k_hit = np.zeros(n, np.int64)
    pend = np.zeros(n, bool)                # the previous step was just above the surface
    act = np.arange(n)
    k = 1
    while act.size:
        s = k * step
        q = o[act] + s * d[act]
        m = _surface_margin(dem, R, q)
        edge = _norm(q) - R if smax is None else s - smax[act]
        inside = edge <= 0
        below = inside & (m <= 0)
        near_surf = m < band
        flags.note("exit", idx[act[near_surf]], edge[near_surf])
        p = pend[act]
        touch = act[p & ~below]
        flags.note("march", idx[touch], np.zeros(touch.size))
        pend[act] = inside & ~below & near_surf
        shallow = np.flatnonzero(below & (m > -band))
        if shallow.size:                    # a hit just below the surface: does the ray go deeper?
            a = act[shallow]
            m2 = _surface_margin(dem, R, o[a] + (k + 1) * step * d[a])
            flags.note("march", idx[a[m2 > -band]], m[shallow][m2 > -band])
        hit[act[below]] = True
        k_hit[act[below]] = k
        act = act[inside & ~below]
        k += 1
    return hit, k_hit


def _bisect(dem, R, step, eps, o, d, k, idx, flags):
    """Bisection of [s_{k-1}, s_k] down to width <= eps; the hit is the OUTSIDE end."""
    lo = (k - 1) * step
    hi = k * step * np.ones(len(o))
    lo = lo * np.ones(len(o))
    width = step
    while width > eps:
        mid = 0.5 * (lo + hi)
        m = _surface_margin(dem, R, o + mid[:, None] * d)
        flags.note("bisect", idx, m)
        bel = m <= 0
        hi = np.where(bel, mid, hi)
        lo = np.where(bel, lo, mid)
        width *= 0.5
    return o + lo[:, None] * d, lo


def _vertex(dem, color, R, albedo, p):
    """Normal (gradient of r - R D, D differentiated one texel either side) and albedo at surface points p."""
    hgt, wid = dem.shape
    r = _norm(p)
    rho = np.maximum(np.hypot(p[:, 0], p[:, 1]), 1e-6)
    lat, lon = _latlon(p)
    dla, dlo = np.pi / hgt, 2 * np.pi / wid
    dlat = (_dem_bilinear(dem, np.clip(lat + dla, -np.pi / 2, np.pi / 2), lon)
            - _dem_bilinear(dem, np.clip(lat - dla, -np.pi / 2, np.pi / 2), lon)) / (2 * dla)
    dlon = (_dem_bilinear(dem, lat, lon + dlo) - _dem_bilinear(dem, lat, lon - dlo)) / (2 * dlo)
    sphi, cphi, slam, clam = p[:, 2] / r, rho / r, p[:, 0] / rho, p[:, 1] / rho
    north = np.stack([-sphi * slam, -sphi * clam, cphi], -1)
    east = np.stack([clam, -slam, np.zeros_like(clam)], -1)
    nrm = p / r[:, None] - (R / r * dlat)[:, None] * north - (R / rho * dlon)[:, None] * east
    nrm /= _norm(nrm)[:, None]
    if color is None:
        alb = np.broadcast_to(np.asarray(albedo, float), (len(p), 3)).copy()
    else:       # D4: the colour map's own grid, same bilinear convention as the DEM
        alb = np.stack([_dem_bilinear(color[..., ch], lat, lon) for ch in range(3)], -1) / 255.0
    return nrm, alb


def _basis(n, spec_rng):
    if spec_rng:
        return _duff_basis(n)
    hlp = np.where(np.abs(n[:, [2]]) < 0.9, [[0, 0, 1.0]], [[1.0, 0, 0]])
    b1 = np.cross(hlp, n); b1 /= _norm(b1)[:, None]
    return b1, np.cross(n, b1)


def _light(sc, dem, R, Lb, p, nrm, ua, ub, idx, flags, spec_rng, counts, dn):
    """D5: 2 radiance (1 - cos theta_max) max(n.w, 0) V for one uniform direction w in the light's cone."""
    o = p + sc.scene_epsilon * nrm
    tl = Lb - o
    dist = _norm(tl)
    ld = tl / dist[:, None]
    sin2 = np.minimum((sc.light_radius / dist) ** 2, 1.0)
    omc = sin2 / (1 + np.sqrt(1 - sin2))
    ct = 1 - ua * omc
    st = np.sqrt(np.maximum(0, 1 - ct * ct))
    ph = 2 * np.pi * ub
    b1, b2 = _basis(ld, spec_rng)
    wi = st[:, None] * (np.cos(ph)[:, None] * b1 + np.sin(ph)[:, None] * b2) + ct[:, None] * ld
    cosi = (nrm * wi).sum(-1)
    flags.note("cosine", idx, cosi, dn)
    lit = cosi > 0
    sh = np.flatnonzero(lit)
    counts["shadow_rays"] += sh.size
    blocked, _ = _march(dem, R, sc.marching_step, o[sh], wi[sh], idx[sh], flags)
    lit[sh[blocked]] = False
    return np.where(lit, 2 * sc.light_radiance * omc * cosi, 0.0)


def _env(bg, dirs, idx, flags, dd=0.0):
    """D7: nearest texel by elevation / azimuth of scene-frame unit directions (dd: their uncertainty in radians)."""
    h, w = bg.shape[:2]
    el, az = _latlon(dirs)
    row = (np.pi / 2 - el) / np.pi * h
    col = (az + np.pi) / (2 * np.pi) * w
    flags.note("env", idx, np.abs(row - np.rint(row)), dd * h / np.pi)
    flags.note("env", idx, np.abs(col - np.rint(col)), dd * w / (2 * np.pi * np.maximum(np.cos(el), 1e-3)))
    r = np.clip(np.floor(row), 0, h - 1).astype(np.int64)
    c = np.floor(col).astype(np.int64) % w
    return bg[r, c, :3].astype(np.float64) / 255.0


def _sun(centre, radius, o, d, idx, flags, dd=0.0, dp=0.0):
    """D8: does the ray o + t d (t > 0) meet the sphere (centre, radius)?  Returns (hit, t of the near intersection).
    dd, dp: uncertainty of the direction (radians) and of the origin (length)."""
    s = centre - o
    tc = s @ d.T if s.ndim == 1 else (s * d).sum(-1)
    q2 = (s * s).sum(-1) - tc * tc
    r2 = radius * radius
    slack = 2 * radius * (np.abs(tc) * dd + dp) / r2
    slack = slack[tc > 0] if np.ndim(slack) else slack
    flags.note("sun", idx[tc > 0], (q2 - r2)[tc > 0] / r2, slack)
    hit = (tc > 0) & (q2 < r2)
    return hit, tc - np.sqrt(np.maximum(r2 - q2, 0.0))


def render(scene, dem, color=None, bg=None, blocks=1, spec_rng=True, seed=1234, bands=None):
    """The model's frame after `blocks` accumulation blocks of scene.spp_per_launch samples.

    spec_rng=True: the spec's counter-based uniforms and Duff bases (the same rays as the oracle up to rounding, so the
    comparison is per pixel); False: numpy's own RNG and another basis (statistical checks).

    Returns a dict:
      linear   (H, W, 4) mean (r, g, b, coverage), float64
      hits     (H, W, 4) sample 0 of the last block: scene position + distance from the eye, zeros on a miss
      var      (H, W, 3) per-pixel sample variance of the radiance (for statistical bounds)
      flagged  (H, W) bool: some sample of the pixel lay within the band of a decision in EXCLUDED
      hit0_flagged (H, W) bool: the hit-buffer sample did
      flag_counts  {decision: number of samples within its band}
      stats    primary_hits, shadow_rays, bounce_rays, bounce_sun_hits, samples
      samples  (blocks * S, H, W, 4) every sample; sample_flagged (blocks * S, H, W)
    """
    bands = dict(BANDS, **(bands or {}))
    dem = np.asarray(dem)
    color = None if color is None else np.asarray(color)
    bg = None if bg is None else np.asarray(bg)
    W, H, S = scene.width, scene.height, scene.spp_per_launch
    R = float(scene.radius)
    seg_min, seg_max = int(scene.path_seg_min), max(int(scene.path_seg_max), 1)
    dims = 4 + 5 * (seg_max - 1)
    n = blocks * S * H * W
    # samples in the order (gs, y, x)
    if spec_rng:
        U = np.stack([np.stack([u.ravel() for u in spec_uniforms(scene, gs, dims)]) for gs in range(blocks * S)], 1)
        U = U.reshape(dims, n)
    else:
        U = np.random.default_rng(seed).random((dims, n))
    sidx = np.arange(n)
    xs = sidx % W
    ys = (sidx // W) % H
    gs = sidx // (W * H)
    flags = _Flags(n, bands)
    counts = dict(primary_hits=0, shadow_rays=0, bounce_rays=0, bounce_sun_hits=0, samples=n)

    eye, tgt, up = (np.asarray(v, float) for v in (scene.eye, scene.target, scene.up))
    wv = tgt - eye; wv /= np.linalg.norm(wv)
    uv = np.cross(wv, up); uv /= np.linalg.norm(uv)
    vv = np.cross(uv, wv)
    th = np.tan(np.radians(scene.vfov_deg) / 2)
    ez = np.asarray(scene.u, float); ez /= np.linalg.norm(ez)
    v0 = np.asarray(scene.v, float); v0 = v0 - (v0 @ ez) * ez; v0 /= np.linalg.norm(v0)
    M = np.stack([np.cross(ez, v0), v0, ez])                     # scene -> moon frame (east 90, lon 0, north)
    centre = np.asarray(scene.center, float)
    Lb = M @ (np.asarray(scene.light_pos, float) - centre)
    sun_on = scene.sun_radius > 0
    sun_scene = np.asarray(scene.sun_pos, float)
    sun_moon = M @ (sun_scene - centre)
    step, eps = scene.marching_step, scene.marching_step_eps
    shift = bracket(scene) + ENTRY_SHIFT

    colour = np.zeros((n, 3))
    cover = np.zeros(n)
    hitpos = np.zeros((n, 4))

    # D1 camera ray, entry into the bounding sphere
    fx = xs + U[0]; fy = ys + U[1]
    sx = (fx / W * 2 - 1) * th * W / H
    sy = (1 - fy / H * 2) * th
    d = wv + sx[:, None] * uv + sy[:, None] * vv
    d /= _norm(d)[:, None]
    oc = eye - centre
    b = d @ oc
    disc = b * b - (oc @ oc - R * R)
    sq = np.sqrt(np.maximum(disc, 0))
    t0 = np.maximum(-b - sq, 0)
    t1 = -b + sq
    on = np.flatnonzero((disc > 0) & (t1 > 0))
    pe = (oc + t0[on, None] * d[on]) @ M.T
    dm = d[on] @ M.T
    hit, k = _march(dem, R, step, pe, dm, on, flags, smax=(t1 - t0)[on])
    cur = on[hit]                                                # samples whose path is alive, and where they are
    p, lo = _bisect(dem, R, step, eps, pe[hit], dm[hit], k[hit], cur, flags)
    din = dm[hit]
    counts["primary_hits"] = cur.size
    cover[cur] = 1.0
    hitpos[cur, :3] = centre + p @ M
    hitpos[cur, 3] = t0[cur] + lo

    # primary misses: D8 Sun disk, else D7 environment
    miss = np.setdiff1d(sidx, cur, assume_unique=True)
    if sun_on and miss.size:
        sh, ts = _sun(sun_scene, scene.sun_radius, eye, d[miss], miss, flags)
        m = miss[sh]
        colour[m] = scene.sun_radiance
        cover[m] = 1.0
        hitpos[m, :3] = eye + ts[sh, None] * d[m]
        hitpos[m, 3] = ts[sh]
        miss = miss[~sh]
    if bg is not None and miss.size:
        colour[miss] = _env(bg, d[miss], miss, flags)

    # the path
    thr = np.ones((cur.size, 3))
    seg = 1
    while cur.size:
        nrm, alb = _vertex(dem, color, R, scene.const_albedo, p)
        # the spec's hit may lie up to one final bracket + its entry shift away along the ray: how far the normal turns
        dn = np.zeros(cur.size)
        for sgn in (1.0, -1.0):
            n2, _ = _vertex(dem, None, R, scene.const_albedo, p + sgn * shift * din)
            dn = np.maximum(dn, _norm(n2 - nrm))
        ul1, ul2 = (U[2], U[3]) if seg == 1 else (U[4 + 5 * (seg - 2) + 3], U[4 + 5 * (seg - 2) + 4])
        wgt = _light(scene, dem, R, Lb, p, nrm, ul1[cur], ul2[cur], cur, flags, spec_rng, counts, dn)
        colour[cur] += thr * alb * wgt[:, None]
        if seg >= seg_max:
            break
        d0 = 4 + 5 * (seg - 1)
        thr = thr * alb
        if seg + 1 > seg_min:                                    # Russian roulette
            pr = np.minimum(alb.max(-1), 1.0)
            u = U[d0][cur]
            flags.note("roulette", cur, u - pr)
            live = u < pr
            cur, p, nrm, dn, thr = cur[live], p[live], nrm[live], dn[live], thr[live] / pr[live, None]
        uh1, uh2 = U[d0 + 1][cur], U[d0 + 2][cur]
        rr, zz, ph = np.sqrt(uh1), np.sqrt(1 - uh1), 2 * np.pi * uh2
        b1, b2 = _basis(nrm, spec_rng)
        wd = (rr * np.cos(ph))[:, None] * b1 + (rr * np.sin(ph))[:, None] * b2 + zz[:, None] * nrm
        o = p + scene.scene_epsilon * nrm
        counts["bounce_rays"] += cur.size
        bh, bk = _march(dem, R, step, o, wd, cur, flags)
        esc = np.flatnonzero(~bh)
        if esc.size:
            e = cur[esc]
            left = esc
            if sun_on:
                sh, _ = _sun(sun_moon, scene.sun_radius, o[esc], wd[esc], e, flags, 2 * dn[esc], shift)
                colour[e[sh]] += thr[esc[sh]] * scene.sun_radiance
                counts["bounce_sun_hits"] += int(sh.sum())
                left = esc[~sh]
            if bg is not None and left.size:
                colour[cur[left]] += thr[left] * _env(bg, wd[left] @ M, cur[left], flags, 2 * dn[left])
        stay = np.flatnonzero(bh)
        p, _ = _bisect(dem, R, step, eps, o[stay], wd[stay], bk[stay], cur[stay], flags)
        cur, thr, din = cur[stay], thr[stay], wd[stay]
        seg += 1

    near = flags.flagged()
    any_flag = np.zeros(n, bool)
    for kd in EXCLUDED:
        any_flag |= near[kd]
    per = (blocks * S, H, W)
    samples = np.concatenate([colour, cover[:, None]], -1).reshape(per + (4,))
    last0 = (blocks - 1) * S
    return dict(
        linear=samples.mean(0),
        var=samples[..., :3].var(0, ddof=1) if blocks * S > 1 else np.zeros((H, W, 3)),
        hits=hitpos.reshape(per + (4,))[last0],
        flagged=any_flag.reshape(per).any(0),
        hit0_flagged=any_flag.reshape(per)[last0],
        flag_counts={k: int(v.sum()) for k, v in near.items()},
        stats=counts,
        samples=samples,
        sample_flagged=any_flag.reshape(per),
    )

