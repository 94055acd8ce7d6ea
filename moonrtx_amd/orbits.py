"""Relay orbiters for MoonRT.horizon_passes: Moon-fixed position tables from Kepler elements, and the
contact windows of a constellation against the terrain horizons of a set of sites.

The Moon-fixed frame is the library's body axes, the ones the point tables use: x = r cos(lat) sin(lon), y = r cos(lat) cos(lon),
z = r sin(lat) -- x toward 90 deg east on the equator, y toward the prime meridian, z toward the north pole.  Orbits are
integrated in the right-handed frame (X toward the prime meridian, Y toward 90 deg east, Z north) and relabelled at the end.

Limits of kepler_fixed_positions: two-body motion about a point mass, optionally with the secular J2 drift of the node, the
periapsis and the mean anomaly.  No mascons, no higher harmonics, no Earth or Sun as third bodies, no radiation pressure, a Moon
that spins uniformly about its z axis: the accuracy is that of planning (low lunar orbits drift by kilometres per day against
this model).  Real ephemerides and orbits that no Kepler ellipse describes, a near-rectilinear halo orbit for one, come in as
the caller's own (S, m, 3) position table."""
import math
from datetime import timedelta
from typing import NamedTuple, Optional

import numpy as np

GM_MOON = 4.9028e12             # m^3 s^-2
J2_MOON = 2.0323e-4
R_EQ_MOON = 1737400.0           # m
SPIN_PERIOD_S = 27.321661 * 86400.0
SPIN_RATE = 2.0 * math.pi / SPIN_PERIOD_S      # rad s^-1 about +z


class Elements(NamedTuple):
    a_m: float                  # semi-major axis, metres
    e: float                    # eccentricity, 0 <= e < 1
    inc_deg: float              # inclination to the Moon's equator
    raan_deg: float             # right ascension of the ascending node: from the inertial X axis, which lies on the prime
                                # meridian at `epoch`
    argp_deg: float             # argument of periapsis
    m0_deg: float               # mean anomaly at `epoch`
    epoch: object               # timezone-aware datetime


def fixed_from_latlon(lat_deg, lon_deg, r_m):
    """(..., 3) float64 Moon-fixed positions (the library's body axes) of selenographic latitude, east longitude (degrees) and
    distance from the centre (metres)."""
    la, lo, r = np.broadcast_arrays(np.radians(np.asarray(lat_deg, np.float64)), np.radians(np.asarray(lon_deg, np.float64)),
                                    np.asarray(r_m, np.float64))
    return np.stack([r * np.cos(la) * np.sin(lo), r * np.cos(la) * np.cos(lo), r * np.sin(la)], -1)


def latlon_from_fixed(pos_m):
    """(lat_deg, lon_deg in (-180, 180], r_m) of (..., 3) Moon-fixed positions: fixed_from_latlon's inverse."""
    p = np.asarray(pos_m, np.float64)
    r = np.sqrt((p * p).sum(-1))
    lat = np.degrees(np.arctan2(p[..., 2], np.hypot(p[..., 0], p[..., 1])))
    lon = np.degrees(np.arctan2(p[..., 0], p[..., 1]))
    return lat, np.where(lon <= -180.0, lon + 360.0, lon), r


def mean_motion(a_m):
    """n = sqrt(GM / a^3), rad s^-1."""
    return math.sqrt(GM_MOON / float(a_m) ** 3)


def period_s(a_m):
    """The two-body period 2 pi sqrt(a^3 / GM), seconds."""
    return 2.0 * math.pi / mean_motion(a_m)


def j2_rates(el):
    """(node rate, periapsis rate, mean-anomaly rate beyond n) in rad s^-1: the secular first-order J2 drift,
    -1.5 n J2 (R/p)^2 cos i, 0.75 n J2 (R/p)^2 (5 cos^2 i - 1) and 0.75 n J2 (R/p)^2 sqrt(1 - e^2) (3 cos^2 i - 1)."""
    n = mean_motion(el.a_m)
    p = el.a_m * (1.0 - el.e * el.e)
    k = n * J2_MOON * (R_EQ_MOON / p) ** 2
    ci = math.cos(math.radians(el.inc_deg))
    return -1.5 * k * ci, 0.75 * k * (5.0 * ci * ci - 1.0), 0.75 * k * math.sqrt(1.0 - el.e * el.e) * (3.0 * ci * ci - 1.0)


def solve_kepler(mean_anomaly, e, tol=1e-14, max_iter=64):
    """The eccentric anomaly E of M = E - e sin E by Newton's method, iterated until the float64 residual |E - e sin E - M| is at
    most tol at every entry (M is first wrapped into [-pi, pi])."""
    if not 0.0 <= e < 1.0:
        raise ValueError(f"the eccentricity must lie in [0, 1) (got {e})")
    M = np.remainder(np.asarray(mean_anomaly, np.float64) + math.pi, 2.0 * math.pi) - math.pi
    E = M + e * np.sin(M) if e < 0.8 else np.where(M < 0.0, -math.pi, math.pi) * np.ones_like(M)
    for _ in range(max_iter):
        res = E - e * np.sin(E) - M
        if np.all(np.abs(res) <= tol):
            return E
        E = E - res / (1.0 - e * np.cos(E))
    raise RuntimeError("Kepler's equation did not converge")


def kepler_inertial(el, t_s, j2=True):
    """(positions (m, 3), velocities (m, 3)) in metres and m/s at t_s seconds after el.epoch, in the right-handed inertial
    frame that coincides with the Moon-fixed (prime meridian, 90 deg east, north) at the epoch."""
    t = np.atleast_1d(np.asarray(t_s, np.float64))
    if not (el.a_m > 0.0):
        raise ValueError("the semi-major axis must be > 0")
    n = mean_motion(el.a_m)
    dO, dw, dM = j2_rates(el) if j2 else (0.0, 0.0, 0.0)
    E = solve_kepler(math.radians(el.m0_deg) + (n + dM) * t, el.e)
    b = math.sqrt(1.0 - el.e * el.e)
    cE, sE = np.cos(E), np.sin(E)
    x, y = el.a_m * (cE - el.e), el.a_m * b * sE                 # in the orbit's plane, x toward the periapsis
    rr = el.a_m * (1.0 - el.e * cE)
    vx, vy = -el.a_m * el.a_m * n * sE / rr, el.a_m * el.a_m * n * b * cE / rr
    O = math.radians(el.raan_deg) + dO * t
    w = math.radians(el.argp_deg) + dw * t
    ci, si = math.cos(math.radians(el.inc_deg)), math.sin(math.radians(el.inc_deg))
    cO, sO, cw, sw = np.cos(O), np.sin(O), np.cos(w), np.sin(w)
    Px, Py, Pz = cO * cw - sO * sw * ci, sO * cw + cO * sw * ci, sw * si
    Qx, Qy, Qz = -cO * sw - sO * cw * ci, -sO * sw + cO * cw * ci, cw * si
    pos = np.stack([Px * x + Qx * y, Py * x + Qy * y, Pz * x + Qz * y], -1)
    vel = np.stack([Px * vx + Qx * vy, Py * vx + Qy * vy, Pz * vx + Qz * vy], -1)
    return pos, vel


def kepler_fixed_positions(elements, start, m, step_s, j2=True):
    """(m, 3) float64 Moon-fixed positions (metres, the library's body axes) of an orbiter at start + k step_s, k = 0 .. m - 1.
    Two-body propagation of `elements` (Kepler's equation by Newton's method to a float64 residual of 1e-14; GM = 4.9028e12
    m^3 s^-2); j2 adds the secular rates of the node, the periapsis and the mean anomaly (J2 = 2.0323e-4, R_eq = 1 737 400 m).
    The inertial frame coincides with the Moon-fixed one at elements.epoch and the Moon spins about +z once per 27.321661
    days.  Planning accuracy only: see the module's docstring for what is left out."""
    if m < 1:
        raise ValueError("m must be >= 1")
    t = (start - elements.epoch).total_seconds() + float(step_s) * np.arange(int(m), dtype=np.float64)
    pos, _ = kepler_inertial(elements, t, j2)
    th = SPIN_RATE * t                                           # the prime meridian has turned east by th
    c, s = np.cos(th), np.sin(th)
    X, Y = c * pos[:, 0] + s * pos[:, 1], -s * pos[:, 0] + c * pos[:, 1]
    return np.stack([Y, X, pos[:, 2]], -1)


class RelayPasses(NamedTuple):
    records: np.ndarray           # _lib.PASS_DTYPE, ascending (point, sat, first)
    aos: list                     # acquisition of signal of each pass (at `start` for a pass already under way)
    los: list                     # loss of signal (at the last date for a pass still under way)
    duration_s: np.ndarray        # LOS - AOS, seconds


class RelayCoverage(NamedTuple):
    times: list                   # the dates used
    share_any: np.ndarray         # (N,) share of the dates with at least one satellite in view
    share_two: np.ndarray         # (N,) share with two or more
    mean_in_view: np.ndarray      # (N,) mean number of satellites in view
    longest_outage_h: np.ndarray  # (N,) longest run of dates with none in view, hours (run x step)
    longest_contact_h: np.ndarray  # (N,) longest unbroken contact, handovers included, hours
    first_contact: np.ndarray     # (N,) int: index into `times` of that contact's first date (the earliest such; -1: none)
    contacts_per_day: np.ndarray  # (N,) separate contacts per day
    max_elev_deg: np.ndarray      # (N,) highest culmination of a satellite in view (-90: never in view)
    passes: Optional[RelayPasses]  # with list_passes
    stats: dict                   # summed counters and kernel times


def pass_times(records, start, step_s):
    """RelayPasses of PASS_DTYPE records: AOS = start + (first - rise_frac) step_s, LOS = start + (first + count - 1 + set_frac)
    step_s, the crossings of the margin interpolated linearly between the dates on either side."""
    r = np.asarray(records)
    t0 = (r["first"].astype(np.float64) - r["rise_frac"].astype(np.float64)) * float(step_s)
    t1 = ((r["first"] + r["count"] - 1).astype(np.float64) + r["set_frac"].astype(np.float64)) * float(step_s)
    return RelayPasses(r, [start + timedelta(seconds=float(v)) for v in t0], [start + timedelta(seconds=float(v)) for v in t1],
                       t1 - t0)


def relay_passes(rt, lat, lon, positions_m, start, step_s, height_m=0.0, min_elev_deg=5.0, n_az=256, n_bis=14,
                 list_passes=False, chunk=65536, radius_m=1737400.0):
    """When can the points (lat, lon in degrees) talk to a relay constellation?  positions_m: (S, m, 3) or (m, 3) Moon-fixed
    metres at start + k step_s (kepler_fixed_positions, or the caller's own table).  Each point's horizon is marched once from
    a mast top height_m above it (MoonRT.horizon) and kept in a device buffer; the satellites are then held against it on every
    date (MoonRT.horizon_passes): in view above both the terrain and the elevation mask min_elev_deg.  Points are streamed
    `chunk` at a time and no (points x satellites x dates) table is formed.  Returns RelayCoverage; list_passes adds every
    pass with its AOS, LOS and duration."""
    from .renderer import DeviceBuffer
    from .sunlight import _heights
    la = np.atleast_1d(np.asarray(lat, np.float64)).ravel()
    lo = np.atleast_1d(np.asarray(lon, np.float64)).ravel()
    if la.shape != lo.shape:
        raise ValueError("lat and lon must have the same number of points")
    pos = np.asarray(positions_m, np.float64)
    pos = pos[None] if pos.ndim == 2 else pos
    if pos.ndim != 3 or pos.shape[2] != 3:
        raise ValueError("positions_m must be (S, m, 3) or (m, 3)")
    m = pos.shape[1]
    times = [start + timedelta(seconds=k * float(step_s)) for k in range(m)]
    rt.horizon_azimuths(n_az)       # checks n_az
    h = np.broadcast_to(np.asarray(0.0 if height_m is None else height_m, np.float64).ravel(), (la.size,))
    raised = _heights(h, radius_m, la.size)
    chunk = max(1, min(int(chunk), la.size, (1 << 31) // int(n_az)))
    out = np.empty((la.size, 8), np.float32)
    recs = []
    stats = {}
    buf = DeviceBuffer(chunk * int(n_az) * 4, rt.config()["device"])
    try:
        for a in range(0, la.size, chunk):
            b = min(a + chunk, la.size)
            rt.horizon(la[a:b], lo[a:b], n_az=n_az, n_bis=n_bis, stats=stats, out=buf, **raised(a, b))
            kw = dict(height_m=h[a:b], min_elev_deg=min_elev_deg, n_az=n_az, radius_m=radius_m, stats=stats)
            out[a:b] = rt.horizon_passes(la[a:b], lo[a:b], buf, pos, mode="summary", **kw)
            if list_passes:
                part = rt.horizon_passes(la[a:b], lo[a:b], buf, pos, mode="list", **kw)
                part["point"] += a
                recs.append(part)
    finally:
        buf.free()
    hours = float(step_s) / 3600.0
    days = m * float(step_s) / 86400.0
    passes = pass_times(np.concatenate(recs), start, step_s) if list_passes else None
    return RelayCoverage(times, out[:, 0], out[:, 7], out[:, 6], out[:, 1].astype(np.float64) * hours,
                         out[:, 2].astype(np.float64) * hours, out[:, 3].astype(np.int64), out[:, 4].astype(np.float64) / days,
                         out[:, 5], passes, stats)
