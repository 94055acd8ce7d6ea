"""Least-cost rover traverses over the terrain: the field MoonRT.traverse returns, route extraction
from its predecessors, and penalty maps built from the other terrain stages' outputs.

A penalty P multiplies an edge's effort by the mean of its two end nodes' penalties; +inf makes a node impassable.  The
library accepts P finite in [1e-3, 1e6] or +inf."""
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
