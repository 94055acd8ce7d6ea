"""float64 model of the terrain-scattered flux, TEST INFRASTRUCTURE.

View samples: the float32 direction table of the spec, mapped in float64 about the model's normal (tests/horizon_model.py:
frame, on oracle/numpy_paths.py's _vertex) with library sqrt / trig and the Duff et al. basis, marched with
numpy_paths._march and refined with numpy_paths._bisect from the lifted origin.  A ray is FLAGGED if it came within the band
of a discrete decision (a march step touching the surface, the sphere exit there): float32 may decide it the other way.
Gather: the spec's reduction in its stated order, in float32 exactly as the kernel rounds it."""
import math

import numpy as np

import horizon_model as hm
from oracle.numpy_paths import BANDS, _Flags, _bisect, _march


def directions(k):
    """The (k, 2) float32 (uh1, uh2) table: ((j + 1/2) / k, frac(j * 0.6180339887498949)), float64 rounded once."""
    j = np.arange(int(k), dtype=np.float64)
    t = j * 0.6180339887498949
    return np.stack([(j + 0.5) / k, t - np.floor(t)], -1).astype(np.float32)


def duff_basis(n):
    """Duff et al. 2017, float64, per row of n (P, 3): (b1, b2)."""
    sg = np.where(n[:, 2] >= 0.0, 1.0, -1.0)
    a = -1.0 / (sg + n[:, 2])
    b = n[:, 0] * n[:, 1] * a
    b1 = np.stack([1.0 + sg * n[:, 0] ** 2 * a, sg * b, -sg * n[:, 0]], -1)
    b2 = np.stack([b, sg + n[:, 1] ** 2 * a, -n[:, 1]], -1)
    return b1, b2


def view_hits(scene, dem, lat_deg, lon_deg, k):
    """dict(hit (P, K) bool, lat / lon (P, K) float64 degrees of the hit (NaN: sky), share (P,), flagged (P, K))."""
    dem = np.asarray(dem)
    R, step = float(scene.radius), float(scene.marching_step)
    o, nrm, _, _, _ = hm.frame(scene, dem, lat_deg, lon_deg)
    P = o.shape[0]
    dirs = directions(k).astype(np.float64)
    rr, zz = np.sqrt(dirs[:, 0]), np.sqrt(1.0 - dirs[:, 0])
    ph = 2.0 * math.pi * dirs[:, 1]
    x, y = rr * np.cos(ph), rr * np.sin(ph)
    b1, b2 = duff_basis(nrm)
    d = (zz[None, :, None] * nrm[:, None, :] + y[None, :, None] * b2[:, None, :] + x[None, :, None] * b1[:, None, :])
    d = d.reshape(-1, 3)
    d /= np.sqrt((d * d).sum(-1))[:, None]
    oo = np.repeat(o, k, axis=0)
    idx = np.arange(P * k)
    flags = _Flags(P * k, BANDS)
    hit, kh = _march(dem, R, step, oo, d, idx, flags)
    lat = np.full(P * k, np.nan)
    lon = np.full(P * k, np.nan)
    h = np.flatnonzero(hit)
    if h.size:
        p, _ = _bisect(dem, R, step, float(scene.marching_step_eps), oo[h], d[h], kh[h], idx[h], flags)
        lat[h] = np.degrees(np.arctan2(p[:, 2], np.hypot(p[:, 0], p[:, 1])))
        lon[h] = np.degrees(np.arctan2(p[:, 0], p[:, 1]))
    near = flags.flagged()
    fl = near["march"] | near["exit"]      # a bisection flip moves the hit by less than one final bracket (numpy_paths)
    hit = hit.reshape(P, k)
    return dict(hit=hit, lat=lat.reshape(P, k), lon=lon.reshape(P, k), share=hit.mean(1), flagged=fl.reshape(P, k))


def angle_between(lat1, lon1, lat2, lon2):
    """Angular distance in radians between (lat, lon) degree pairs (float64, any shape)."""
    a1, o1, a2, o2 = (np.radians(np.asarray(v, np.float64)) for v in (lat1, lon1, lat2, lon2))
    u1 = np.stack([np.cos(a1) * np.sin(o1), np.cos(a1) * np.cos(o1), np.sin(a1)], -1)
    u2 = np.stack([np.cos(a2) * np.sin(o2), np.cos(a2) * np.cos(o2), np.sin(a2)], -1)
    c = np.linalg.norm(np.cross(u1, u2), axis=-1)
    return np.arctan2(c, (u1 * u2).sum(-1))


def gather(index, exitance, albedo_h, emissivity):
    """Q_sec (N, m) float32: (1/K) x the float32 sum over j = 0 .. K-1 with index[p, j] >= 0, in that order, of
    (1 - A_h) M_vis + eps M_ir, each product, term and partial sum rounded to float32."""
    index = np.asarray(index)
    ex = np.asarray(exitance, np.float32)
    n, k = index.shape
    omah, eps = np.float32(1.0 - albedo_h), np.float32(emissivity)
    s = np.zeros((n, ex.shape[1]), np.float32)
    for j in range(k):
        q = index[:, j]
        sel = q >= 0
        e = ex[np.where(sel, q, 0)]
        term = (omah * e[..., 0]) + (eps * e[..., 1])
        s = np.where(sel[:, None], s + term, s).astype(np.float32)
    return (s * np.float32(1.0 / k)).astype(np.float32)
