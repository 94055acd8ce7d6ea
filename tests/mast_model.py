"""float64 model of the raised horizons and the joint windows, TEST INFRASTRUCTURE.

Raised horizon: tests/horizon_model.py's bisection from the raised end of tests/sight_model.py, P = o + hs u with hs the
float32 value of h / radius_m * R.  A point with hs == 0 runs horizon_model.horizon's arithmetic operation for operation
(the facet test n . d > 0, the march from the lifted origin); a point with hs > 0 marches every probe, from where the probe
enters the bounding sphere when P lies outside it (clear when it heads away from the sphere or misses it).  A (point,
azimuth) is FLAGGED if any of its probes came within the band of a discrete decision: horizon_model's, and -- within the
exit band, in scene units -- whether P is outside the sphere and whether the probe meets it (sight_model's).

Windows: the eight columns of mrtx_horizon_windows reduced from two FULL fraction arrays with numpy."""
import numpy as np

from horizon_model import frame, longest_run, normal_slack, steps_inside
from oracle.numpy_paths import BANDS, _Flags, _march
from sight_model import scene_height


def origins(scene, dem, lat_deg, lon_deg, h_m, radius_m=1737400.0):
    """(P (N, 3) raised origins, hs (N,) the raises in scene units, and horizon_model.frame's o, nrm, U, N, E)."""
    o, nrm, U, N, E = frame(scene, dem, lat_deg, lon_deg)
    hs = np.broadcast_to(scene_height(scene, h_m, radius_m), (o.shape[0],)).astype(np.float64)
    return o + hs[:, None] * U, hs, (o, nrm, U, N, E)


def horizon(scene, dem, lat_deg, lon_deg, h_m, n_az, n_bis, radius_m=1737400.0):
    """horizon_model.horizon from mast tops h_m (metres; one value or one per point) above the points: the same dict."""
    dem = dem if hasattr(dem, "shape") else np.asarray(dem)
    R = float(scene.radius)
    step = scene.marching_step
    O, hs, (o, nrm, U, N, E) = origins(scene, dem, lat_deg, lon_deg, h_m, radius_m)
    P = o.shape[0]
    phi = 2 * np.pi * np.arange(n_az) / n_az
    h = np.cos(phi)[None, :, None] * N[:, None, :] + np.sin(phi)[None, :, None] * E[:, None, :]    # (P, n_az, 3)
    h = h.reshape(-1, 3)
    pi = np.repeat(np.arange(P), n_az)
    up = (hs > 0)[pi]
    r0 = np.sqrt((O * O).sum(-1))[pi]
    outside = up & (r0 > R)
    lo_t = np.zeros(P * n_az)
    hi_t = np.ones(P * n_az)
    flags = _Flags(P * n_az, BANDS)
    idx = np.arange(P * n_az)
    flags.note("exit", idx[up], (r0 - R)[up])
    rays, samples = 0, 5 * P * n_az
    slack = np.repeat(normal_slack(dem.shape, lat_deg), n_az)
    for _ in range(n_bis):
        mid = 0.5 * (lo_t + hi_t)
        e = 2 * np.pi * (mid - 0.5) * 0.5
        d = np.cos(e)[:, None] * h + np.sin(e)[:, None] * U[pi]
        d /= np.sqrt((d * d).sum(-1))[:, None]
        cosi = (nrm[pi] * d).sum(-1)
        flags.note("cosine", idx[~up], cosi[~up], slack[~up])
        probe = up | (cosi > 0)
        rays += int(probe.sum())
        org = O[pi].copy()
        run = probe.copy()
        clear = np.zeros(P * n_az, bool)
        out = np.flatnonzero(outside)
        if out.size:
            b = (org[out] * d[out]).sum(-1)
            closest = np.sqrt(np.maximum(r0[out] ** 2 - b * b, 0.0))       # the line's nearest approach to the centre
            meets = (b < 0) & (closest <= R)
            flags.note("exit", idx[out], np.where(b < 0, closest - R, np.inf))
            flags.note("exit", idx[out], np.where(closest <= R, b, np.inf))
            s_in = -b - np.sqrt(np.maximum(b * b - (r0[out] ** 2 - R * R), 0.0))
            org[out] = org[out] + s_in[:, None] * d[out]
            run[out[~meets]] = False
            clear[out[~meets]] = True
        go = np.flatnonzero(run)
        if go.size:
            blocked, k_hit = _march(dem, R, step, org[go], d[go], idx[go], flags)
            clear[go[~blocked]] = True
            samples += int(steps_inside(R, step, org[go], d[go], blocked, k_hit).sum())
        hi_t = np.where(clear, mid, hi_t)
        lo_t = np.where(clear, lo_t, mid)
    near = flags.flagged()
    fl = near["march"] | near["exit"] | near["cosine"]
    elev = ((hi_t - 0.5) * 180.0).astype(np.float32)
    return dict(elev=elev.reshape(P, n_az), lo=lo_t.reshape(P, n_az), hi=hi_t.reshape(P, n_az), flagged=fl.reshape(P, n_az),
                shadow_rays=rays, height_samples=samples)


def first_longest_run(mask):
    """(length, first index) of the earliest longest run of True in a 1-D boolean sequence; (0, -1) if there is none."""
    best, start, cur = 0, -1, 0
    for i, v in enumerate(np.asarray(mask, bool)):
        cur = cur + 1 if v else 0
        if cur > best:
            best, start = cur, i - cur + 1
    return best, start


def windows(f_a, f_b, min_a, min_b):
    """((N, 8) float64 columns of mrtx_horizon_windows, (N, 3) int64 counts of ok_a, ok_b, both) from the FULL fractions
    f_a, f_b (N, m) float32; the thresholds are compared as float32, as the kernel does."""
    f_a, f_b = np.asarray(f_a, np.float32), np.asarray(f_b, np.float32)
    n, m = f_a.shape
    ok_a, ok_b = f_a >= np.float32(min_a), f_b >= np.float32(min_b)
    both = ok_a & ok_b
    out = np.empty((n, 8))
    cnt = np.stack([ok_a.sum(1), ok_b.sum(1), both.sum(1)], -1).astype(np.int64)
    for p in range(n):
        run, first = first_longest_run(both[p])
        assert run == longest_run(both[p])
        out[p] = (cnt[p, 0] / m, longest_run(~ok_a[p]), cnt[p, 1] / m, longest_run(~ok_b[p]), cnt[p, 2] / m, run, first,
                  longest_run(~both[p]))
    return out, cnt
