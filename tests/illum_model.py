"""float64 model of the Sun illumination stage, TEST INFRASTRUCTURE.

Node (lat, lon) -> unit vector u -> p = R D(lat, lon) u -> normal (oracle/numpy_paths.py: _vertex) -> lifted origin
o = p + scene_epsilon n -> for each (u2, u3) of the library's own table (MoonRT.sun_samples) one direction in the light's
cone, cos = n . w, and a shadow ray marched through the float64 height field (numpy_paths._march).  Library trig, exact
texel coordinates at every step.  Samples that come within the band of a discrete decision -- a march step touching the
surface, the bounding sphere's exit there, cos against 0 -- are FLAGGED: float32 may decide them the other way.
"""
import numpy as np

from oracle.numpy_march import _dem_bilinear, _duff_basis
from oracle.numpy_paths import BANDS, _Flags, _march, _vertex


def sun_dir_moon_frame(scene):
    """Unit vector to the light centre from the Moon centre, in the moon frame (east 90, lon 0, north)."""
    ez = np.asarray(scene.u, float); ez = ez / np.linalg.norm(ez)
    v0 = np.asarray(scene.v, float); v0 = v0 - (v0 @ ez) * ez; v0 /= np.linalg.norm(v0)
    M = np.stack([np.cross(ez, v0), v0, ez])
    Lb = M @ (np.asarray(scene.light_pos, float) - np.asarray(scene.center, float))
    return Lb, M


def subsolar_latlon(scene):
    """(lat, lon) in degrees of the light centre seen from the Moon centre, the spec's lon = atan2(a, b)."""
    Lb, _ = sun_dir_moon_frame(scene)
    return np.degrees(np.arctan2(Lb[2], np.hypot(Lb[0], Lb[1]))), np.degrees(np.arctan2(Lb[0], Lb[1]))


def illuminate(scene, dem, lat_deg, lon_deg, samples):
    """Per node: dict(lit, irr, mu, D) (float64, shape (N,)), V (N, n) per-sample visibility (cos > 0 and escaping),
    flagged (N, n), shadow_rays (the samples with cos > 0) and carried (N, n), what each sample carries when it arrives."""
    dem = dem if hasattr(dem, "shape") else np.asarray(dem)
    R = float(scene.radius)
    la = np.radians(np.asarray(lat_deg, float).ravel())
    lo = np.radians(np.asarray(lon_deg, float).ravel())
    N, n = la.size, len(samples)
    u = np.stack([np.cos(la) * np.sin(lo), np.cos(la) * np.cos(lo), np.sin(la)], -1)
    D = _dem_bilinear(dem, la, lo)
    p = (R * D)[:, None] * u
    nrm, _ = _vertex(dem, None, R, (1.0, 1.0, 1.0), p)
    o = p + scene.scene_epsilon * nrm
    Lb, _ = sun_dir_moon_frame(scene)
    tl = Lb - o
    dist = np.sqrt((tl * tl).sum(-1))
    ld = tl / dist[:, None]
    mu = (nrm * ld).sum(-1)
    sin2 = np.minimum((scene.light_radius / dist) ** 2, 1.0)
    omc = sin2 / (1 + np.sqrt(1 - sin2))
    b1, b2 = _duff_basis(ld)
    u2 = np.asarray(samples, float)[:, 0]
    u3 = np.asarray(samples, float)[:, 1]
    # every (node, sample) pair, node-major
    ni = np.repeat(np.arange(N), n)
    ct = 1 - u2[None, :] * omc[:, None]
    st = np.sqrt(np.maximum(0.0, 1 - ct * ct))
    ph = 2 * np.pi * u3[None, :]
    w = (st * np.cos(ph))[..., None] * b1[:, None, :] + (st * np.sin(ph))[..., None] * b2[:, None, :] + ct[..., None] * ld[:, None, :]
    w = w.reshape(-1, 3)
    cosi = (nrm[ni] * w).sum(-1)
    flags = _Flags(N * n, BANDS)
    idx = np.arange(N * n)
    flags.note("cosine", idx, cosi)
    up = np.flatnonzero(cosi > 0)
    blocked, _ = _march(dem, R, scene.marching_step, o[ni[up]], w[up], idx[up], flags)
    V = np.zeros(N * n, bool)
    V[up[~blocked]] = True
    carried = 2 * scene.light_radiance * omc[ni] * cosi
    near = flags.flagged()
    fl = near["march"] | near["exit"] | near["cosine"]
    V = V.reshape(N, n)
    return dict(lit=V.mean(1), irr=np.where(V, carried.reshape(N, n), 0.0).mean(1), mu=mu, D=D, V=V,
                flagged=fl.reshape(N, n), shadow_rays=int(up.size), cos_pos=(cosi > 0).reshape(N, n), cosi=cosi.reshape(N, n),
                carried=carried.reshape(N, n))
