"""Least-cost rover traverses over the terrain: the field MoonRT.traverse returns, route extraction
from its predecessors, and penalty maps built from the other terrain stages' outputs.

A penalty P multiplies an edge's effort by the mean of its two end nodes' penalties; +inf makes a node impassable.  The
library accepts P finite in [1e-3, 1e6] or +inf.

Timed traverses (section 3.19) are at the end: availability masks as bits, the field MoonRT.traverse_timed returns, routes
with their waits, and the drive mask of a window."""
import math

import numpy as np

# direction k = the step from a node v to its predecessor u: N, NE, E, SE, S, SW, W, NW
DI = np.array([-1, -1, 0, 1, 1, 1, 0, -1])
DJ = np.array([0, 1, 1, 1, 0, -1, -1, -1])
SOURCE, NO_PRED, UNREACHABLE = 8, 254, 255
P_MIN, P_MAX = 1e-3, 1e6


def window_dict(window):
    """A window as a dict (row0, col0, rows, cols, stride, wrap) from a dict or a (row0, col0, rows, cols[, stride[, wrap]])
    sequence."""
    keys = ("row0", "col0", "rows", "cols", "stride", "wrap")
    if isinstance(window, dict):
        w = {"stride": 1, "wrap": 0}
        w.update(window)
    else:
        vals = list(window)
        if not 4 <= len(vals) <= 6:
            raise ValueError("a window is (row0, col0, rows, cols[, stride[, wrap]])")
        w = dict(zip(keys, vals + [1, 0][len(vals) - 4:]))
    unknown = set(w) - set(keys)
    if unknown:
        raise ValueError(f"unknown window keys {sorted(unknown)}")
    return {k: int(w[k]) for k in keys}


class TraverseField:
    """What MoonRT.traverse returns: cost (rows, cols) float64, pred (rows, cols) uint8, the window, the per-row edge
    lengths (rows, 3) float32 (L_ew, L_ns, L_dg), radius_m, the node lat / lon axes and D, the window's (rows, cols) node
    heights in units of the radius (a copy: the field does not refer to a context).  `heights(i, j)` gives the nodes'
    heights above the sphere in metres, (D - 1) radius_m, or NaN when the field holds no D."""

    def __init__(self, cost, pred, window, lengths, radius_m=1737400.0, lat=None, lon=None, D=None):
        self.cost = np.asarray(cost, np.float64)
        self.pred = np.asarray(pred, np.uint8)
        self.window = window_dict(window)
        self.lengths = np.asarray(lengths, np.float32).reshape(-1, 3)
        self.radius_m = float(radius_m)
        self.lat, self.lon = lat, lon
        self.D = None if D is None else np.asarray(D, np.float32)
        if self.cost.shape != self.pred.shape or self.cost.shape != (self.window["rows"], self.window["cols"]):
            raise ValueError("cost and pred must both have the window's shape (rows, cols)")
        if self.D is not None and self.D.shape != self.cost.shape:
            raise ValueError("D must have the window's shape (rows, cols)")

    def heights(self, i, j):
        i, j = np.asarray(i, np.int64), np.asarray(j, np.int64)
        if self.D is None:
            return np.full(i.shape, np.nan)
        return (self.D[i, j].astype(np.float64) - 1.0) * self.radius_m

    def step_length(self, i, k):
        """The length, metres, of the edge from a node in row i to its neighbour in direction k."""
        di, dj = int(DI[k]), int(DJ[k])
        if di == 0:
            return float(self.lengths[i, 0])
        return float(self.lengths[i - 1 if di < 0 else i, 1 if dj == 0 else 2])


class RouteError(ValueError):
    pass


def route(field, target):
    """The least-cost route from a source to `target` = (i, j), following the predecessors.  Returns a dict of arrays from
    the source to the target: i, j (node indices), lat, lon (degrees; NaN if the field has no axes), height_m, cost (the
    cumulative cost, the field's values, the source's start cost included) and length_m (the cumulative length of the
    steps, float64 sums of the float32 edge lengths).  Raises RouteError on an unreachable target, a node without a
    predecessor (code 254), an unknown code or a chain that does not end at a source."""
    rows, cols = field.cost.shape
    wrap = field.window["wrap"]
    i, j = int(target[0]), int(target[1])
    if not (0 <= i < rows and 0 <= j < cols):
        raise RouteError(f"target ({i}, {j}) lies outside the {rows} x {cols} window")
    path = [(i, j)]
    steps = []
    for _ in range(rows * cols):
        code = int(field.pred[i, j])
        if code == SOURCE:
            break
        if code == UNREACHABLE:
            raise RouteError(f"node ({i}, {j}) is unreachable from every source")
        if code == NO_PRED:
            raise RouteError(f"node ({i}, {j}) has no predecessor (code 254)")
        if code > 7:
            raise RouteError(f"node ({i}, {j}) holds the unknown predecessor code {code}")
        ni, nj = i + int(DI[code]), j + int(DJ[code])
        if wrap:
            nj %= cols
        if not (0 <= ni < rows and 0 <= nj < cols):
            raise RouteError(f"the predecessor of node ({i}, {j}) lies outside the window")
        steps.append(field.step_length(i, code))
        i, j = ni, nj
        path.append((i, j))
    else:
        raise RouteError("the predecessor chain does not end at a source")
    path.reverse()
    steps.reverse()
    ii = np.array([p[0] for p in path], np.int64)
    jj = np.array([p[1] for p in path], np.int64)
    lat = field.lat[ii] if field.lat is not None else np.full(ii.shape, np.nan)
    lon = field.lon[jj] if field.lon is not None else np.full(ii.shape, np.nan)
    return {"i": ii, "j": jj, "lat": np.asarray(lat, np.float64), "lon": np.asarray(lon, np.float64),
            "height_m": field.heights(ii, jj), "cost": field.cost[ii, jj],
            "length_m": np.concatenate([[0.0], np.cumsum(np.asarray(steps, np.float64))])}


def route_csv(r, path):
    """Write a route (the dict `route` returns) as CSV, one node per line."""
    with open(path, "w") as f:
        f.write("i,j,lat_deg,lon_deg,height_m,cost,length_m\n")
        for k in range(len(r["i"])):
            f.write(",".join([str(int(r["i"][k])), str(int(r["j"][k]))] +
                             [repr(float(r[c][k])) for c in ("lat", "lon", "height_m", "cost", "length_m")]) + "\n")


# ---- penalty builders: each returns a float32 map the library accepts, +inf where the node is closed
def penalty_from_viewshed(view, base=None):
    """Keep line of sight to an observer: +inf where MoonRT.viewshed's extra mast height is not 0 (the node does not see the
    observer at the target height), else `base` (1, or a penalty map to combine with)."""
    v = np.asarray(view, np.float32)
    b = np.ones(v.shape, np.float32) if base is None else np.asarray(base, np.float32)
    return np.where(v == 0.0, b, np.float32(np.inf)).astype(np.float32)


def penalty_from_sunlit(share, weight=4.0, min_share=None):
    """Prefer sunlit ground: P = 1 + weight (1 - share) for a sunlit share in [0, 1] (the `mean` of
    MoonRT.illumination_statistics / horizon_sun's summary, or the `lit` channel of an illumination map); +inf below
    min_share when one is given."""
    s = np.clip(np.asarray(share, np.float64), 0.0, 1.0)
    p = 1.0 + float(weight) * (1.0 - s)
    if min_share is not None:
        p = np.where(s < float(min_share), np.inf, p)
    return _clamp(p)


def penalty_from_temperature(t_max, limit_k, soft_k=None):
    """Avoid hot ground: +inf where the maximum surface temperature t_max (K; MoonRT.surface_temperature's summary max)
    exceeds limit_k; with soft_k < limit_k, P rises linearly from 1 at soft_k to 10 at limit_k."""
    t = np.asarray(t_max, np.float64)
    p = np.ones(t.shape)
    if soft_k is not None:
        p = 1.0 + 9.0 * np.clip((t - float(soft_k)) / (float(limit_k) - float(soft_k)), 0.0, 1.0)
    p = np.where(t > float(limit_k), np.inf, p)
    return _clamp(p)


def _grade_and(relief, field):
    """(grade-like array) of a ReliefMap's field or of a plain array."""
    return np.asarray(getattr(relief, field) if hasattr(relief, field) else relief, np.float64)


def penalty_from_slope(relief, max_slope_deg, weight=4.0):
    """Keep off steep ground at the scale of the vehicle: +inf where the footprint's grade (MoonRT.relief's `grade`, or a
    plain array of grades) exceeds the limit or is NaN, else P = 1 + weight grade / tan(max_slope_deg), rising from 1 on
    level ground to 1 + weight at the limit."""
    g = _grade_and(relief, "grade")
    gmax = max_slope_grade(max_slope_deg)
    p = 1.0 + float(weight) * (g / gmax)
    return _clamp(np.where(g > gmax, np.inf, p))


def penalty_from_roughness(relief, max_rms_m, weight=4.0):
    """Keep off rough ground: +inf where the footprint's roughness (MoonRT.relief's `rms_m`, or a plain array, metres) exceeds
    max_rms_m or is NaN, else P = 1 + weight rms_m / max_rms_m."""
    r = _grade_and(relief, "rms_m")
    m = float(max_rms_m)
    if not m > 0.0:
        raise ValueError("max_rms_m must be > 0")
    p = 1.0 + float(weight) * (r / m)
    return _clamp(np.where(r > m, np.inf, p))


def _clamp(p):
    p = np.asarray(p, np.float64)
    out = np.where(np.isinf(p), np.inf, np.clip(p, P_MIN, P_MAX)).astype(np.float32)
    out[np.isnan(p)] = np.inf
    return out


def max_slope_grade(max_slope_deg):
    """The grade (rise over run) of a slope limit in degrees; 90 or more: no limit (+inf)."""
    d = float(max_slope_deg)
    if not d > 0.0:
        raise ValueError("max_slope_deg must be > 0")
    return math.inf if d >= 90.0 else math.tan(math.radians(d))


# ---- timed traverses: time in integer ticks, availability as bits
NEVER = np.uint64(0xFFFFFFFFFFFFFFFF)


def mask_words(n_epochs):
    """W64, the uint64 words of one node's availability row: (n_epochs + 63) // 64."""
    return (int(n_epochs) + 63) // 64


def pack_mask(bits):
    """(..., m) booleans to (..., W64) uint64: bit k & 63 of word k >> 6 is epoch k, the bits past m - 1 are 0."""
    b = np.asarray(bits, bool)
    m = b.shape[-1]
    pad = np.zeros(b.shape[:-1] + (mask_words(m) * 64,), np.uint8)
    pad[..., :m] = b
    return np.ascontiguousarray(np.packbits(pad, axis=-1, bitorder="little")).view("<u8")


def unpack_mask(words, n_epochs):
    """(..., W64) uint64 to (..., n_epochs) booleans."""
    w = np.ascontiguousarray(words, "<u8")
    if w.shape[-1] != mask_words(n_epochs):
        raise ValueError(f"{n_epochs} epochs take {mask_words(n_epochs)} words per row (got {w.shape[-1]})")
    return np.unpackbits(w.view(np.uint8), axis=-1, bitorder="little")[..., :int(n_epochs)].astype(bool)


def edge_ticks(w, ticks_per_cost):
    """q of an edge of float32 weight w: x = float64(w) * ticks_per_cost; 1 if x <= 1, else ceil(x); None if the edge is
    not driven (w infinite or x > 2^31)."""
    w = float(np.float32(w))
    if math.isinf(w) or math.isnan(w):
        return None
    x = w * float(ticks_per_cost)
    if not x <= 2147483648.0:
        return None
    return 1 if x <= 1.0 else int(math.ceil(x))


class TimedField(TraverseField):
    """What MoonRT.traverse_timed returns: arrival (rows, cols) uint64 ticks (NEVER where unreachable), pred, the window,
    lengths, axes and D of a TraverseField, the tick scales (ticks_per_cost, ticks_per_epoch, n_epochs), the effort model
    (max_grade, climb_cost, descent_cost) and penalty map with which `edge_ticks_at` recomputes a step's duration, and
    `avail`, the (rows, cols, W64) mask if it was passed as an array (else None).  `cost` is the arrival as float64 (inf
    where unreachable), so that `route` works on the field."""

    def __init__(self, arrival, pred, window, lengths, radius_m=1737400.0, lat=None, lon=None, D=None, ticks_per_cost=5.0,
                 ticks_per_epoch=3600, n_epochs=None, max_grade=math.inf, climb_cost=0.0, descent_cost=0.0, penalty=None,
                 avail=None):
        self.arrival = np.asarray(arrival, np.uint64)
        cost = np.where(self.arrival == NEVER, np.inf, self.arrival.astype(np.float64))
        super().__init__(cost, pred, window, lengths, radius_m, lat, lon, D)
        self.ticks_per_cost, self.ticks_per_epoch = float(ticks_per_cost), int(ticks_per_epoch)
        self.n_epochs = None if n_epochs is None else int(n_epochs)
        self.max_grade, self.climb_cost, self.descent_cost = float(max_grade), float(climb_cost), float(descent_cost)
        self.penalty = None if penalty is None else np.asarray(penalty, np.float32)
        self.avail = None if avail is None else np.asarray(avail, np.uint64)

    def edge_weight(self, i, j, k):
        """float32 w(u -> v) for v = (i, j) and u its neighbour in direction k, in section 3.13's order (+inf: not driven)."""
        if self.D is None:
            raise ValueError("the field holds no D")
        f32 = np.float32
        rows, cols = self.arrival.shape
        ui, uj = i + int(DI[k]), j + int(DJ[k])
        if self.window["wrap"]:
            uj %= cols
        L = f32(self.step_length(i, k))
        with np.errstate(over="ignore", invalid="ignore"):
            dh = (self.D[i, j] - self.D[ui, uj]) * f32(self.radius_m)
            if abs(dh / L) > f32(self.max_grade):
                return f32(np.inf)
            c = (L + f32(self.climb_cost) * max(dh, f32(0))) + f32(self.descent_cost) * max(-dh, f32(0))
            m = f32(1) if self.penalty is None else f32(0.5) * (self.penalty[ui, uj] + self.penalty[i, j])
            return f32(c * m)

    def edge_ticks_at(self, i, j, k):
        return edge_ticks(self.edge_weight(i, j, k), self.ticks_per_cost)


def timed_route(field, target):
    """`route`'s dict for a TimedField (cost = the arrival ticks as float64), plus per node arrive_tick (the field's
    arrival), depart_tick and wait_ticks (uint64): the wait before the step to the next node is
    A[next] - q - A[this] with q the step's duration recomputed on the host (TimedField.edge_ticks_at); the target departs
    when it arrives.  Also longest_wait_ticks, total_wait_ticks and drive_ticks (the sum of the q).  Raises RouteError in
    `route`'s cases, and if a step's duration does not fit between its two arrivals."""
    r = route(field, target)
    ii, jj = r["i"], r["j"]
    n = len(ii)
    arrive = [int(field.arrival[ii[s], jj[s]]) for s in range(n)]
    wait, depart, drive = [0] * n, list(arrive), 0
    for s in range(n - 1):
        i, j = int(ii[s + 1]), int(jj[s + 1])
        q = field.edge_ticks_at(i, j, int(field.pred[i, j]))
        if q is None or arrive[s + 1] - q < arrive[s]:
            raise RouteError(f"the step into node ({i}, {j}) does not fit between its two arrivals")
        wait[s] = arrive[s + 1] - q - arrive[s]
        depart[s] = arrive[s] + wait[s]
        drive += q
    r["arrive_tick"] = np.array(arrive, np.uint64)
    r["depart_tick"] = np.array(depart, np.uint64)
    r["wait_ticks"] = np.array(wait, np.uint64)
    r["longest_wait_ticks"] = max(wait)
    r["total_wait_ticks"] = sum(wait)
    r["drive_ticks"] = drive
    return r


def timed_route_csv(r, path, ticks_per_hour=None):
    """Write a timed route as CSV, one node per line; with ticks_per_hour the three times are hours, else ticks."""
    s = 1.0 if ticks_per_hour is None else 1.0 / float(ticks_per_hour)
    unit = "ticks" if ticks_per_hour is None else "h"
    with open(path, "w") as f:
        f.write(f"i,j,lat_deg,lon_deg,height_m,length_m,arrive_{unit},depart_{unit},wait_{unit}\n")
        for k in range(len(r["i"])):
            f.write(",".join([str(int(r["i"][k])), str(int(r["j"][k]))] +
                             [repr(float(r[c][k])) for c in ("lat", "lon", "height_m", "length_m")] +
                             [repr(float(r[c][k]) * s) for c in ("arrive_tick", "depart_tick", "wait_ticks")]) + "\n")


def drive_mask(rt, window, times, height_m=0.0, min_sun=0.5, min_earth=None, n_az=256, n_bis=14, observer=None,
               chunk=4096):
    """The drive mask of every node of a window: a DeviceBuffer of rows x cols x W64 uint64 words (W64 = mask_words(len(
    times))), ready for MoonRT.traverse_timed(avail=, n_epochs=len(times)).  Bit k of a node's row: at times[k] (ISO strings
    or datetimes, as ephemeris.sun_epochs takes them) the share of the Sun's disc above the node's horizon is >= min_sun
    and, with min_earth, the Earth's is >= min_earth.  Per chunk of nodes: MoonRT.horizon (from height_m above the ground
    when it is not 0), then MoonRT.horizon_mask against ephemeris.sun_epochs or sun_earth_epochs, both on the device.
    Masks of several constraints combine by AND (download, np.bitwise_and, pass the array as avail)."""
    from . import ephemeris
    from .renderer import DeviceBuffer
    w = window_dict(window)
    lat, lon, _ = rt.traverse_nodes(w)
    la, lo = (a.ravel() for a in np.meshgrid(lat, lon, indexing="ij"))
    if min_earth is None:
        ea, eb = ephemeris.sun_epochs(times, observer=observer), None
    else:
        ea, eb = ephemeris.sun_earth_epochs(times, observer=observer)
    m = len(ea)
    W64 = mask_words(m)
    n = la.size
    out = DeviceBuffer(max(n * W64 * 8, 8), rt.config()["device"])
    chunk = max(1, int(chunk))
    hz = DeviceBuffer(min(chunk, n) * int(n_az) * 4, rt.config()["device"])
    for a in range(0, n, chunk):
        b = min(a + chunk, n)
        rt.horizon(la[a:b], lo[a:b], n_az=n_az, n_bis=n_bis, out=hz, height_m=height_m if height_m else None)
        rt.horizon_mask(la[a:b], lo[a:b], hz, ea, eb, min_a=min_sun, min_b=1.0 if min_earth is None else min_earth,
                        n_az=n_az, out=out, out_offset=a * W64 * 8)
    hz.free()
    return out
