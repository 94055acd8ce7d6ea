"""float64 model of the terrain line of sight, TEST INFRASTRUCTURE.

An end (lat, lon, h metres) -> the vertex and lifted origin of tests/horizon_model.py (oracle/numpy_paths.py: _vertex) ->
P = o + hs u, hs = the float32 value of h / radius_m * R (the spec rounds it once; the model takes that value).  A probe
marches the segment from its lower end (the target on a tie) toward the other one with numpy_paths._march, ending at the
nearer of the far end and the bounding sphere's exit; a lower end outside the sphere marches from where the segment enters
it, or not at all when the segment misses the sphere.  Per target the mast bisection of the spec.  Library trig, exact
texel coordinates.  A probe is FLAGGED if it came within the band of a discrete decision the float32 kernel may take the
other way: a march step touching the surface, the sphere exit or the far end there (numpy_paths' bands), and -- within the
exit band, in scene units -- which end is lower, whether the lower end is outside the sphere, whether the segment meets the
sphere and whether it enters before its end.  A target is flagged if any of its probes is."""
import numpy as np

from horizon_model import frame
from oracle.numpy_paths import BANDS, _Flags, _march


def scene_height(scene, h_m, radius_m):
    """hs of the spec: (float)(h / radius_m * R), as float64."""
    return (np.asarray(h_m, np.float64) / float(radius_m) * float(scene.radius)).astype(np.float32).astype(np.float64)


def ends(scene, dem, lat_deg, lon_deg):
    """Per point: the lifted origin o and the radial unit vector u, (P, 3) each."""
    o, _, U, _, _ = frame(scene, dem, lat_deg, lon_deg)
    return o, U


def probe(scene, dem, T, O, idx, flags):
    """Clear (bool per probe) and the spec's step count of each probe, for target ends T and observer ends O ((K, 3))."""
    R = float(scene.radius)
    step = scene.marching_step
    K = len(T)
    rT, rO = np.sqrt((T * T).sum(-1)), np.sqrt((O * O).sum(-1))
    flags.note("exit", idx, rT - rO)
    from_t = rT <= rO
    lo = np.where(from_t[:, None], T, O)
    hi = np.where(from_t[:, None], O, T)
    t = hi - lo
    L = np.sqrt((t * t).sum(-1))
    clear = np.ones(K, bool)
    steps = np.zeros(K, np.int64)
    live = L > 0
    d = np.where(live[:, None], t / np.where(live, L, 1.0)[:, None], 0.0)
    org = lo.copy()
    smax = L.copy()
    r0 = np.sqrt((lo * lo).sum(-1))
    out = live & (r0 > R)
    flags.note("exit", idx[live], (r0 - R)[live])
    if out.any():
        b = (lo[out] * d[out]).sum(-1)
        closest = np.sqrt(np.maximum(r0[out] ** 2 - b * b, 0.0))       # the line's nearest approach to the centre
        meets = (b < 0) & (closest <= R)
        flags.note("exit", idx[out], np.where(b < 0, closest - R, np.inf))
        s_in = -b - np.sqrt(np.maximum(b * b - (r0[out] ** 2 - R * R), 0.0))
        enters = meets & (s_in < L[out])
        flags.note("exit", idx[out][meets], (s_in - L[out])[meets])
        oi = np.flatnonzero(out)
        live[oi[~enters]] = False
        org[oi] = lo[oi] + s_in[:, None] * d[oi]
        smax[oi] = L[oi] - s_in
    run = np.flatnonzero(live)
    if run.size:
        o, dd = org[run], d[run]
        b = (o * dd).sum(-1)
        c = (o * o).sum(-1) - R * R
        t_exit = -b + np.sqrt(np.maximum(b * b - c, 0.0))
        sm = np.minimum(smax[run], t_exit)
        blocked, k_hit = _march(dem, R, step, o, dd, idx[run], flags, smax=sm)
        clear[run[blocked]] = False
        steps[run] = np.where(blocked, k_hit, np.floor(np.maximum(sm, 0.0) / step).astype(np.int64))
    return clear, steps


def sight(scene, dem, lat_deg, lon_deg, observer, target_h_m=0.0, mast_max_m=0.0, n_bis=0, radius_m=1737400.0):
    """dict(m (N,) float32 -- the spec's output --, t_hi (N,) float64 (inf where m is), flagged (N,), probes (N,),
    shadow_rays, height_samples (the spec's counters)).  observer: one (lat, lon, h_m) triple or (N, 3)."""
    dem = dem if hasattr(dem, "shape") else np.asarray(dem)
    la = np.asarray(lat_deg, float).ravel()
    lo = np.asarray(lon_deg, float).ravel()
    N = la.size
    ob = np.asarray(observer, float).reshape(-1, 3)
    ob = np.broadcast_to(ob, (N, 3)) if ob.shape[0] == 1 else ob
    oT, uT = ends(scene, dem, la, lo)
    oO, uO = ends(scene, dem, ob[:, 0], ob[:, 1])
    O = oO + scene_height(scene, ob[:, 2], radius_m)[:, None] * uO
    flags = _Flags(N, BANDS)
    probes = np.zeros(N, np.int64)
    samples = 10 * N

    def run(sel, t):
        nonlocal samples
        hs = scene_height(scene, target_h_m + t * mast_max_m, radius_m)
        hs = np.broadcast_to(hs, sel.shape)
        T = oT[sel] + hs[:, None] * uT[sel]
        clear, steps = probe(scene, dem, T, O[sel], sel, flags)
        probes[sel] += 1
        samples += int(steps.sum())
        return clear

    t_hi = np.full(N, np.inf)
    all_ = np.arange(N)
    c0 = run(all_, np.zeros(N))
    t_hi[c0] = 0.0
    rest = all_[~c0]
    if n_bis > 0 and rest.size:
        c1 = run(rest, np.ones(rest.size))
        rest = rest[c1]
        t_hi[rest] = 1.0
        t_lo = np.zeros(rest.size)
        th = np.ones(rest.size)
        for _ in range(n_bis - 1):
            if not rest.size:
                break
            mid = 0.5 * (t_lo + th)
            c = run(rest, mid)
            th = np.where(c, mid, th)
            t_lo = np.where(c, t_lo, mid)
        t_hi[rest] = th
    with np.errstate(invalid="ignore"):
        m = np.where(np.isinf(t_hi), np.inf, t_hi * mast_max_m).astype(np.float32)
    near = flags.flagged()
    fl = near["march"] | near["exit"]
    return dict(m=m, t_hi=t_hi, flagged=fl, probes=probes, shadow_rays=int(probes.sum()), height_samples=samples)


def raised(scene, dem, lat_deg, lon_deg, h_m, radius_m=1737400.0):
    """The raised ends P (N, 3) of points with heights h_m (metres)."""
    o, u = ends(scene, dem, lat_deg, lon_deg)
    return o + scene_height(scene, h_m, radius_m)[..., None] * u


def sphere_visible(R, a, b, theta):
    """Two points a and b above a sphere of radius R, theta apart at its centre, see each other over it."""
    return theta < np.arccos(R / (R + a)) + np.arccos(R / (R + b))


def sphere_mast(R, a, b, theta):
    """The least extra height x over b at which the upper point sees the one at a (0 if it does already)."""
    need = R / np.cos(theta - np.arccos(R / (R + a))) - R
    return np.maximum(need - b, 0.0)
