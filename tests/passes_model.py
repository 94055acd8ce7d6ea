"""float64 model of the orbiter passes, TEST INFRASTRUCTURE, numpy only.

look: per (point, satellite, epoch) the satellite's elevation es, azimuth, range and margin g = es - max(horizon at that
azimuth, elevation mask), from horizon_model.frame's lifted origin and local frame and horizon_model.horizon_at's interpolation.
tolerances: how far the kernel's float32 values may lie from these, derived from the number formats (below), not tuned.
summary / passes: plain-loop reductions of a margin table to the eight SUMMARY columns and to PASS_DTYPE records, the two
fractions formed in np.float32 exactly as the spec forms them.  emulate32: the kernel's operations restated in numpy float32, so
that the CPU suite can hold the tolerance against a float32 evaluation without a GPU.  case: the shared test case."""
import functools
import math
from datetime import datetime, timezone

import numpy as np

import horizon_model as hm
import model_cases as mc
from moonrtx_amd import orbits
from moonrtx_amd._lib import PASS_DTYPE
from moonrtx_amd.scene import named_scene

RADIUS_M = 1737400.0
N_AZ = 64
START = datetime(2026, 1, 1, tzinfo=timezone.utc)
STEP_S = 60.0


def scene():
    return named_scene("S1", 16, 16)


def scene_positions(s, pos_m, radius_m=RADIUS_M):
    """(S, m, 3) positions in scene units: x / radius_m * R."""
    pos = np.asarray(pos_m, np.float64)
    pos = pos[None] if pos.ndim == 2 else pos
    return pos / float(radius_m) * float(s.radius)


def look(s, dem, lat, lon, hz, pos_m, height_m=0.0, min_elev_deg=0.0, radius_m=RADIUS_M):
    """dict of (P, S, m) float64 arrays: es, az (degrees in [0, 360)), range_m, g, and what the tolerances need (h0, h1, the
    range and |X| in scene units, |o|)."""
    o, _, U, N, E = hm.frame(s, dem, lat, lon)
    R = float(s.radius)
    hs = np.broadcast_to(np.asarray(height_m, np.float64), (o.shape[0],)) / float(radius_m) * R
    P = o + hs[:, None] * U
    X = scene_positions(s, pos_m, radius_m)
    t = X[None] - P[:, None, None, :]
    rng = np.sqrt((t * t).sum(-1))
    l = t / rng[..., None]
    xu = (l * U[:, None, None, :]).sum(-1)
    xn = (l * N[:, None, None, :]).sum(-1)
    xe = (l * E[:, None, None, :]).sum(-1)
    es = np.degrees(np.arctan2(xu, np.hypot(xn, xe)))
    az = np.degrees(np.arctan2(xe, xn)) % 360.0
    shape = es.shape
    hh, h0, h1 = hm.horizon_at(hz, az.reshape(shape[0], -1))
    hh, h0, h1 = hh.reshape(shape), h0.reshape(shape), h1.reshape(shape)
    g = es - np.maximum(hh, float(min_elev_deg))
    return dict(es=es, az=az, range_m=rng * (float(radius_m) / R), g=g, hh=hh, h0=h0, h1=h1, range=rng,
                x_norm=np.broadcast_to(np.sqrt((X * X).sum(-1))[None], shape), o_norm=np.sqrt((P * P).sum(-1))[:, None, None])


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def tolerances(info, n_az):
    """(d_dir, d_az, tol_g) in degrees per (point, satellite, epoch).  The unit direction, the frame and atan2f agree with
    float64 to 5e-5 deg (test_gpu_horizon.f_tolerance's figure); the satellite's position and the origin are each rounded to
    float32, which turns the direction by at most sqrt(3) (ulp32|X| + ulp32|o|) / range.  An azimuth error is the direction's
    divided by cos(es); it moves the interpolated horizon by its slope, |h1 - h0| per 360 / n_az degrees, and the float32
    interpolation adds 1e-5."""
    d_dir = 5e-5 + np.degrees(math.sqrt(3.0) * (ulp32(info["x_norm"]) + ulp32(info["o_norm"])) / info["range"])
    d_az = d_dir / np.maximum(np.cos(np.radians(info["es"])), 1e-12)
    d_h = np.abs(info["h1"] - info["h0"]) * (n_az / 360.0) * d_az + 1e-5
    return d_dir, d_az, d_dir + d_h


def range_tolerance(info, s, radius_m=RADIUS_M):
    """How far the kernel's float32 range may lie from the model's, metres: range * 4e-7 for the float32 differences, sum,
    square root and scaling, plus the ulp of the two end points -- sqrt(3) (ulp32|X| + ulp32|o|), the displacement of the
    satellite and of the origin that d_dir allows across the line of sight, here taken along it.  (The ulp of the range itself
    would not do: 100 km overhead the range is a twentieth of |X| and |o|, whose rounding it inherits.)"""
    to_m = float(radius_m) / float(s.radius)
    return info["range_m"] * 4e-7 + math.sqrt(3.0) * (ulp32(info["x_norm"]) + ulp32(info["o_norm"])) * to_m


def _longest(bits):
    best, start, cur = 0, -1, 0
    for i, v in enumerate(bits):
        cur = cur + 1 if v else 0
        if cur > best:
            best, start = cur, i - cur + 1
    return best, start


def summary(g, es):
    """The (P, 8) float32 SUMMARY columns of a (P, S, m) margin table and its elevations, by plain loops."""
    g, es = np.asarray(g), np.asarray(es)
    P, S, m = g.shape
    out = np.empty((P, 8), np.float32)
    for p in range(P):
        view = g[p] > 0
        c = [int(view[:, k].sum()) for k in range(m)]
        any_ = [v >= 1 for v in c]
        run, first = _longest(any_)
        n_runs = sum(1 for k in range(m) if any_[k] and (k == 0 or not any_[k - 1]))
        e_max = np.float32(-90.0)
        for v in es[p][view]:
            e_max = max(e_max, np.float32(v))
        out[p] = (np.float32(sum(any_) / float(m)), _longest([not v for v in any_])[0], run, first, n_runs, e_max,
                  np.float32(sum(c) / float(m)), np.float32(sum(1 for v in c if v >= 2) / float(m)))
    return out


def passes(g, es, range_m):
    """The PASS_DTYPE records of (P, S, m) float32 margins, elevations and ranges: one per maximal run of g > 0 of one (point,
    satellite), ascending (point, sat, first); the fractions are one float32 subtraction and one float32 division."""
    g, es, rm = (np.asarray(v, np.float32) for v in (g, es, range_m))
    P, S, m = g.shape
    recs = []
    for p in range(P):
        for s in range(S):
            row = g[p, s]
            k = 0
            while k < m:
                if not row[k] > 0:
                    k += 1
                    continue
                first = k
                while k + 1 < m and row[k + 1] > 0:
                    k += 1
                last = k
                flags = (1 if first == 0 else 0) | (2 if last == m - 1 else 0)
                with np.errstate(all="ignore"):
                    rise = np.float32(0) if first == 0 else row[first] / (row[first] - row[first - 1])
                    setf = np.float32(0) if last == m - 1 else row[last] / (row[last] - row[last + 1])
                e = es[p, s, first:last + 1]
                at = first + int(np.argmax(e))                  # the earliest of equal maxima
                recs.append((p, s, first, last - first + 1, at, flags, rise, setf, e.max(), rm[p, s, first:last + 1].min()))
                k += 1
    return np.array(recs, PASS_DTYPE) if recs else np.zeros(0, PASS_DTYPE)


# ---- the kernel's operations in numpy float32 ----------------------------------------------------------------------------------
F = np.float32


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def emulate32(s, dem, lat, lon, hz, pos_m, height_m=0.0, min_elev_deg=0.0, radius_m=RADIUS_M):
    """sat_look in float32: the lifted origin is the model's rounded to float32, the frame comes from float32 (sin, cos)
    tables as point_frame forms it, every product, fma, square root, division, atan2 and floor is float32.  dict of (P, S, m)
    float32 es, az, range_m, g."""
    o, _, _, _, _ = hm.frame(s, dem, lat, lon)
    R = float(s.radius)
    la, lo = np.radians(np.asarray(lat, float).ravel()), np.radians(np.asarray(lon, float).ravel())
    sl, cl, sn, cn = (v.astype(F) for v in (np.sin(la), np.cos(la), np.sin(lo), np.cos(lo)))
    ua, ub, uc = cl * sn, cl * cn, sl
    Na, Nb, Nc = -(sl * sn), -(sl * cn), cl
    o32 = o.astype(F)
    hs = (np.broadcast_to(np.asarray(height_m, np.float64), la.shape) / float(radius_m) * R).astype(F)
    Pa, Pb, Pc = _fma(hs, ua, o32[:, 0]), _fma(hs, ub, o32[:, 1]), _fma(hs, uc, o32[:, 2])
    X = scene_positions(s, pos_m, radius_m).astype(F)
    ex = lambda v: v[:, None, None]                             # noqa: E731
    ta, tb, tc = X[None, ..., 0] - ex(Pa), X[None, ..., 1] - ex(Pb), X[None, ..., 2] - ex(Pc)
    dist = np.sqrt(_fma(tc, tc, _fma(tb, tb, ta * ta)))
    inv = (F(1) / dist).astype(F)
    a, b, c = ta * inv, tb * inv, tc * inv
    shape = a.shape
    bc = lambda v: np.broadcast_to(ex(v), shape)                # noqa: E731
    xu = _fma(bc(uc), c, _fma(bc(ub), b, bc(ua) * a))
    xn = _fma(bc(Nc), c, _fma(bc(Nb), b, bc(Na) * a))
    xe = _fma(bc(-sn), b, bc(cn) * a)
    k_deg, k_turn = F(57.2957795130823209), F(0.159154943091895336)
    es = (np.arctan2(xu, np.sqrt(_fma(xe, xe, xn * xn))).astype(F) * k_deg).astype(F)
    ph = (np.arctan2(xe, xn).astype(F) * k_turn).astype(F)
    ph = np.where(ph < 0, (ph + F(1)).astype(F), ph)
    n_az = hz.shape[1]
    x = (ph * F(n_az)).astype(F)
    x0 = np.floor(x)
    w = (x - x0).astype(F)
    i0 = x0.astype(np.int64) & (n_az - 1)
    i1 = (i0 + 1) & (n_az - 1)
    rows = np.arange(shape[0])[:, None, None]
    hz = np.asarray(hz, F)
    h0, h1 = hz[rows, i0], hz[rows, i1]
    hh = _fma(w, (h1 - h0).astype(F), h0)
    g = (es - np.maximum(hh, F(min_elev_deg))).astype(F)
    az = (ph * F(360)).astype(F)
    return dict(es=es, az=np.where(az >= 360, F(0), az), range_m=(dist * F(float(radius_m) / R)).astype(F), g=g)


# ---- the shared case -----------------------------------------------------------------------------------------------------------
ORBITS = ((100e3, 90.0, 0.0, 0.0), (700e3, 86.0, 60.0, 120.0), (6500e3, 57.0, 120.0, 240.0))    # altitude, inc, raan, m0


def positions(m, orbit_rows=ORBITS):
    """(S, m, 3) Moon-fixed metres of circular orbits, two-body with the J2 drift, one epoch per STEP_S."""
    return np.stack([orbits.kepler_fixed_positions(orbits.Elements(RADIUS_M + alt, 0.0, inc, raan, 0.0, m0, START), START, m, STEP_S)
                     for alt, inc, raan, m0 in orbit_rows])


@functools.lru_cache(maxsize=None)
def case(m=512):
    """24 points of the crater DEM (8 near each pole, 8 at mid-latitudes), the three orbits over m epochs, and a random horizon
    table in [-3, 8] degrees at N_AZ azimuths."""
    rng = np.random.default_rng(271)
    lat = np.concatenate([rng.uniform(-89.0, -80.0, 8), rng.uniform(80.0, 89.0, 8), rng.uniform(-50.0, 50.0, 8)])
    lon = rng.uniform(-180.0, 180.0, lat.size)
    hz = rng.uniform(-3.0, 8.0, (lat.size, N_AZ)).astype(np.float32)
    return dict(scene=scene(), dem=mc.crater_dem(), lat=lat, lon=lon, hz=hz, pos=positions(m), m=m)
