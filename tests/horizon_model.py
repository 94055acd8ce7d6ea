"""float64 model of the terrain horizon and of the Sun against it (DESIGN.md sections 3.8 and 3.9), TEST INFRASTRUCTURE.

Horizon: node (lat, lon) -> the vertex and lifted origin of tests/illum_model.py (oracle/numpy_paths.py: _vertex) -> local
frame U = u, E = (cos lon, -sin lon, 0), N = (-sin lat sin lon, -sin lat cos lon, cos lat) -> per azimuth a / n_az turn the
bisection of the spec over t in [0, 1], each probe at elevation (t - 1/2) / 2 turn: cos = n . d against 0, then the shadow
march of numpy_paths._march.  Library trig, exact texel coordinates.  A (point, azimuth) is FLAGGED if any of its probes came
within the band of a discrete decision (cos against 0, a march step touching the surface, the sphere exit there): float32 may
decide that probe the other way, and the bisection then brackets a different interval.

Sun: per (point, epoch) the direction to the light centre from the lifted origin, its elevation and azimuth in (N, E, U),
the angular radius asin(radius / distance), the horizon interpolated at the azimuth and the disc's visible share."""
import math

import numpy as np

from oracle.numpy_march import _dem_bilinear
from oracle.numpy_paths import BANDS, _Flags, _march, _vertex


def frame(scene, dem, lat_deg, lon_deg):
    """Per point: lifted origin o, normal n, and the local frame U, N, E (each (P, 3))."""
    R = float(scene.radius)
    la = np.radians(np.asarray(lat_deg, float).ravel())
    lo = np.radians(np.asarray(lon_deg, float).ravel())
    U = np.stack([np.cos(la) * np.sin(lo), np.cos(la) * np.cos(lo), np.sin(la)], -1)
    N = np.stack([-np.sin(la) * np.sin(lo), -np.sin(la) * np.cos(lo), np.cos(la)], -1)
    E = np.stack([np.cos(lo), -np.sin(lo), np.zeros_like(lo)], -1)
    D = _dem_bilinear(dem, la, lo)
    p = (R * D)[:, None] * U
    nrm, _ = _vertex(dem, None, R, (1.0, 1.0, 1.0), p)
    return p + scene.scene_epsilon * nrm, nrm, U, N, E


def steps_inside(R, step, o, d, hit, k_hit):
    """height_samples of each probe march: k at a hit, otherwise every step k * step still inside the sphere r <= R."""
    b = (o * d).sum(-1)
    c = (o * o).sum(-1) - R * R
    t1 = -b + np.sqrt(np.maximum(b * b - c, 0.0))
    return np.where(hit, k_hit, np.floor(t1 / step).astype(np.int64))


def normal_slack(shape, lat_deg):
    """How far the kernel's float32 normal may tilt from the model's (tests/test_gpu_illumination.py: mu_tol): n . d of a probe
    is flagged within this much of 0 (the probes converge on the horizon, which is the tangent plane where nothing rises above
    it)."""
    c = np.maximum(np.cos(np.radians(np.asarray(lat_deg, float).ravel())), 1e-3)
    return 1e-5 + 8 * 2.0 ** -24 * np.maximum(shape[0] / (2 * math.pi), shape[1] / (4 * math.pi * c))


def horizon(scene, dem, lat_deg, lon_deg, n_az, n_bis):
    """dict(elev (P, n_az) float32 degrees -- the bisection's result, t_hi of each bracket --, lo / hi (the brackets, float64),
    flagged (P, n_az), shadow_rays, height_samples (the spec's counters))."""
    dem = dem if hasattr(dem, "shape") else np.asarray(dem)
    R = float(scene.radius)
    o, nrm, U, N, E = frame(scene, dem, lat_deg, lon_deg)
    P = o.shape[0]
    phi = 2 * np.pi * np.arange(n_az) / n_az
    h = np.cos(phi)[None, :, None] * N[:, None, :] + np.sin(phi)[None, :, None] * E[:, None, :]    # (P, n_az, 3)
    h = h.reshape(-1, 3)
    pi = np.repeat(np.arange(P), n_az)
    lo_t = np.zeros(P * n_az)
    hi_t = np.ones(P * n_az)
    flags = _Flags(P * n_az, BANDS)
    idx = np.arange(P * n_az)
    rays, samples = 0, 5 * P * n_az
    slack = np.repeat(normal_slack(dem.shape, lat_deg), n_az)
    for _ in range(n_bis):
        mid = 0.5 * (lo_t + hi_t)
        e = 2 * np.pi * (mid - 0.5) * 0.5
        d = np.cos(e)[:, None] * h + np.sin(e)[:, None] * U[pi]
        d /= np.sqrt((d * d).sum(-1))[:, None]
        cosi = (nrm[pi] * d).sum(-1)
        flags.note("cosine", idx, cosi, slack)
        up = np.flatnonzero(cosi > 0)
        clear = np.zeros(P * n_az, bool)
        if up.size:
            blocked, k_hit = _march(dem, R, scene.marching_step, o[pi[up]], d[up], idx[up], flags)
            clear[up[~blocked]] = True
            rays += int(up.size)
            samples += int(steps_inside(R, scene.marching_step, o[pi[up]], d[up], blocked, k_hit).sum())
        hi_t = np.where(clear, mid, hi_t)
        lo_t = np.where(clear, lo_t, mid)
    near = flags.flagged()
    fl = near["march"] | near["exit"] | near["cosine"]
    elev = ((hi_t - 0.5) * 180.0).astype(np.float32)
    return dict(elev=elev.reshape(P, n_az), lo=lo_t.reshape(P, n_az), hi=hi_t.reshape(P, n_az), flagged=fl.reshape(P, n_az),
                shadow_rays=rays, height_samples=samples)


def disc_fraction(h, e_s, alpha):
    """Share of a disc of angular radius alpha centred at elevation e_s above a horizontal line at elevation h (arrays or
    scalars, any angle unit); alpha = 0: the step e_s > h."""
    h, e_s, alpha = np.broadcast_arrays(*(np.asarray(v, float) for v in (h, e_s, alpha)))
    with np.errstate(divide="ignore", invalid="ignore"):
        x = np.clip((h - e_s) / np.where(alpha > 0, alpha, 1.0), -1.0, 1.0)
        f = (np.arccos(x) - x * np.sqrt(1.0 - x * x)) / np.pi
    return np.where(alpha > 0, f, (e_s > h).astype(float))


def sun_position(scene, dem, lat_deg, lon_deg, epochs):
    """(e_s, phi_s, alpha) in degrees, each (P, m): the light centre's elevation and azimuth (0 = north, 90 = east, in
    [0, 360)) from the lifted origin and its angular radius, for the (m, 14) epochs of ephemeris.sun_epochs."""
    o, _, U, N, E = frame(scene, dem, lat_deg, lon_deg)
    ep = np.asarray(epochs, float).reshape(-1, 14)
    Lb = np.empty((ep.shape[0], 3))
    for k, row in enumerate(ep):
        ez = row[8:11] / np.linalg.norm(row[8:11])
        v0 = row[11:14] - (row[11:14] @ ez) * ez
        v0 /= np.linalg.norm(v0)
        M = np.stack([np.cross(ez, v0), v0, ez])
        Lb[k] = M @ (row[0:3] - row[5:8])
    t = Lb[None, :, :] - o[:, None, :]
    dist = np.sqrt((t * t).sum(-1))
    l = t / dist[..., None]
    xu = (l * U[:, None, :]).sum(-1)
    xn = (l * N[:, None, :]).sum(-1)
    xe = (l * E[:, None, :]).sum(-1)
    e_s = np.degrees(np.arctan2(xu, np.hypot(xn, xe)))
    phi = np.degrees(np.arctan2(xe, xn)) % 360.0
    alpha = np.degrees(np.arcsin(np.minimum(1.0, ep[:, 3][None, :] / dist)))
    return e_s, phi, alpha


def horizon_at(hz, phi_deg):
    """The (P, n_az) horizons linearly interpolated at azimuths phi (P, m) degrees, wrapping at 360; also the two samples."""
    hz = np.asarray(hz, float)
    n_az = hz.shape[1]
    x = (np.asarray(phi_deg, float) % 360.0) / 360.0 * n_az
    i0 = np.floor(x).astype(np.int64) % n_az
    i1 = (i0 + 1) % n_az
    w = x - np.floor(x)
    rows = np.arange(hz.shape[0])[:, None]
    h0, h1 = hz[rows, i0], hz[rows, i1]
    return h0 + w * (h1 - h0), h0, h1


def sun_fraction(scene, dem, lat_deg, lon_deg, hz, epochs):
    """(P, m) float64 visible share of the light's disc, and (e_s, phi_s, alpha, h(phi_s), h0, h1) for the band checks."""
    e_s, phi, alpha = sun_position(scene, dem, lat_deg, lon_deg, epochs)
    hh, h0, h1 = horizon_at(hz, phi)
    return disc_fraction(hh, e_s, alpha), dict(e_s=e_s, phi=phi, alpha=alpha, h=hh, h0=h0, h1=h1)


def summarize(f):
    """SUMMARY of FULL fractions (P, m): (mean, share with f > 0, share with f == 1, longest run of f == 0), float64."""
    f = np.asarray(f)
    m = f.shape[1]
    out = np.empty((f.shape[0], 4))
    out[:, 0] = f.astype(np.float64).sum(1) / m
    out[:, 1] = (f > 0).sum(1) / m
    out[:, 2] = (f == 1).sum(1) / m
    out[:, 3] = [longest_run(row == 0) for row in f]
    return out


def longest_run(mask):
    """Length of the longest run of True in a 1-D boolean sequence."""
    best = cur = 0
    for v in np.asarray(mask, bool):
        cur = cur + 1 if v else 0
        best = max(best, cur)
    return best


def bisection_step_deg(n_bis):
    return 180.0 * 2.0 ** -n_bis


def elevation_of(o, q):
    """Elevation (degrees) of point q seen from o above the plane normal to o (the radial horizontal)."""
    v = np.asarray(q, float) - np.asarray(o, float)
    u = np.asarray(o, float) / np.linalg.norm(o)
    return math.degrees(math.asin(float(v @ u) / float(np.linalg.norm(v))))
