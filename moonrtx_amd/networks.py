"""Site networks on availability masks: which two sites together are never dark, and which few.

Everything here stands on MoonRT.mask_pairs (mrtx_mask_pairs): rows of bits in horizon_mask's layout -- Sun on the panel, Earth
in view, both, relay coverage, or any mask packed with traverse.pack_mask -- combined pair by pair on the device.  site_pairs
gives every site its best partner within a distance band, greedy_sites grows a set one site at a time against the union so
far.  Medians, exhaustive searches over more than two sites and link budgets are not here."""
import math
from fractions import Fraction

import numpy as np

from . import _lib
from .regions import COORD_MAX


def point_positions(lat_deg, lon_deg, radius_m=1737400.0, unit_m=0.01, heights_m=None):
    """(n, 3) int32: the positions of n points (degrees) in units of unit_m metres, regions.node_positions' formula for a point
    list: rint((radius_m + h) (cos lat cos lon, cos lat sin lon, sin lat) / unit_m) in float64, h = heights_m (a scalar or one
    per point, metres above the sphere) or 0.  ValueError when a coordinate leaves +-2^29: choose a larger unit."""
    lat = np.radians(np.atleast_1d(np.asarray(lat_deg, np.float64)).ravel())
    lon = np.radians(np.atleast_1d(np.asarray(lon_deg, np.float64)).ravel())
    if lat.shape != lon.shape:
        raise ValueError("lat_deg and lon_deg must have the same number of points")
    if not (radius_m > 0.0 and unit_m > 0.0 and math.isfinite(radius_m) and math.isfinite(unit_m)):
        raise ValueError("radius_m and unit_m must be finite and > 0")
    r = np.full(lat.shape, float(radius_m))
    if heights_m is not None:
        h = np.asarray(heights_m, np.float64)
        if h.shape not in ((), lat.shape) or not np.all(np.isfinite(h)):
            raise ValueError("heights_m must be a finite scalar or one per point")
        r = r + h
    p = np.stack([r * np.cos(lat) * np.cos(lon), r * np.cos(lat) * np.sin(lon), r * np.sin(lat)], -1)
    q = np.rint(p / float(unit_m))
    if not np.all(np.abs(q) <= COORD_MAX):
        raise ValueError(f"a coordinate of {np.abs(p).max():g} m leaves +-2^29 units of {unit_m:g} m: choose a larger unit")
    return q.astype(np.int32)


def site_mask(rt, lat_deg, lon_deg, times, height_m=0.0, min_sun=0.5, min_earth=None, n_az=256, n_bis=14, observer=None,
              chunk=4096):
    """The availability mask of n points as one DeviceBuffer of n x W64 uint64 words, ready for site_pairs and greedy_sites
    (n_rows = n): traverse.drive_mask for a point list.  Bit k of a point's row: at times[k] the share of the Sun's disc
    above its horizon is >= min_sun (None: the Sun is not asked for) and, with min_earth, the Earth's is >= min_earth.  Per
    chunk of points MoonRT.horizon (from height_m above the ground when it is not 0), then MoonRT.horizon_mask."""
    from . import ephemeris
    from .renderer import DeviceBuffer
    from .traverse import mask_words
    la, lo = rt._points(lat_deg, lon_deg)
    if min_sun is None and min_earth is None:
        raise ValueError("give min_sun, min_earth or both")
    if min_sun is None:
        ea, eb, min_a, min_b = ephemeris.earth_epochs(times, observer=observer), None, min_earth, 1.0
    elif min_earth is None:
        ea, eb, min_a, min_b = ephemeris.sun_epochs(times, observer=observer), None, min_sun, 1.0
    else:
        (ea, eb), min_a, min_b = ephemeris.sun_earth_epochs(times, observer=observer), min_sun, min_earth
    w64, n = mask_words(len(ea)), la.size
    device = rt.config()["device"]
    out = DeviceBuffer(max(n * w64 * 8, 8), device)
    chunk = max(1, int(chunk))
    hz = DeviceBuffer(min(chunk, n) * int(n_az) * 4, device)
    try:
        for a in range(0, n, chunk):
            b = min(a + chunk, n)
            rt.horizon(la[a:b], lo[a:b], n_az=n_az, n_bis=n_bis, out=hz, height_m=height_m if height_m else None)
            rt.horizon_mask(la[a:b], lo[a:b], hz, ea, eb, min_a=min_a, min_b=min_b, n_az=n_az, out=out, out_offset=a * w64 * 8)
    finally:
        hz.free()
    return out


def distance_d2(dist_m, unit_m, up):
    """A distance in metres as an integer squared distance in units of unit_m: (dist_m / unit_m)^2 with both floats taken as the
    exact binary fractions they are, rounded up to the next integer (up) or down, capped at 2^64 - 1."""
    if not (math.isfinite(dist_m) and dist_m >= 0.0 and math.isfinite(unit_m) and unit_m > 0.0):
        raise ValueError("a distance must be finite and >= 0, unit_m finite and > 0")
    q = Fraction(dist_m) / Fraction(unit_m)
    q *= q
    return min(math.ceil(q) if up else math.floor(q), 2 ** 64 - 1)


def _rank_order(records, rank, index):
    """The order of the records under the rank, ties by `index` ascending."""
    c, g = records["count"].astype(np.int64), records["gap"].astype(np.int64)
    keys = (index, g, -c) if rank == "count" else (index, -c, g)
    return np.lexsort(keys)


TOP_DTYPE = np.dtype([("a", "<i4"), ("b", "<i4"), ("count", "<u4"), ("gap", "<u4"), ("gap_first", "<i4"), ("gain", "<i8")])


class SitePairs:
    """What site_pairs returns: best (n,) PAIR_DTYPE, every site's best partner and their joint record; own (n,) PAIR_DTYPE, each
    row's own record; gain (n,) int64, the joint count less the better of the two sites' own counts (0 without a partner);
    n_epochs and rank."""

    def __init__(self, best, own, n_epochs, rank):
        self.best, self.own, self.n_epochs, self.rank = best, own, int(n_epochs), rank
        has = best["partner"] >= 0
        partner_own = own["count"][np.where(has, best["partner"], 0)].astype(np.int64)
        alone = np.maximum(own["count"].astype(np.int64), partner_own)
        self.gain = np.where(has, best["count"].astype(np.int64) - alone, 0)

    def top(self, k):
        """The k best distinct unordered pairs among the sites' best partners, first under the rank and then by (a, b) with
        a < b: (<= k,) TOP_DTYPE."""
        has = np.flatnonzero(self.best["partner"] >= 0)
        lo = np.minimum(has, self.best["partner"][has]).astype(np.int64)
        hi = np.maximum(has, self.best["partner"][has]).astype(np.int64)
        n = max(len(self.best), 1)
        order = _rank_order(self.best[has], self.rank, lo * n + hi)
        out, seen = [], set()
        for i in order:
            key = (int(lo[i]), int(hi[i]))
            if key in seen:
                continue
            seen.add(key)
            r = self.best[has[i]]
            out.append((key[0], key[1], r["count"], r["gap"], r["gap_first"], self.gain[has[i]]))
            if len(out) == int(k):
                break
        return np.array(out, TOP_DTYPE)


def site_pairs(rt, mask, n_epochs, positions=None, unit_m=1.0, min_dist_m=0, max_dist_m=None, op="any", rank="count",
               n_rows=None, stats=None):
    """Every site's best partner (MoonRT.mask_pairs, mode "best") and every site's own record (mode "rows") over the rows of
    `mask` ((n, W64) uint64 or a DeviceBuffer with n_rows=).  positions: (n, 3) integers in units of unit_m metres
    (point_positions) or a DeviceBuffer of int32; with them only partners at min_dist_m <= distance <= max_dist_m count.  The
    distances are converted to integer d2 once: d2_min = ceil((min_dist_m / unit_m)^2) and d2_max = floor((max_dist_m /
    unit_m)^2) with the floats taken as the exact binary fractions they are (distance_d2), max_dist_m = None: no upper bound;
    the device then compares exact integers, both ends inclusive.  Returns a SitePairs."""
    d2_min, d2_max = 0, 2 ** 64 - 1
    if positions is not None:
        d2_min = distance_d2(float(min_dist_m), float(unit_m), True)
        if max_dist_m is not None:
            d2_max = distance_d2(float(max_dist_m), float(unit_m), False)
    elif min_dist_m or max_dist_m is not None:
        raise ValueError("a distance band needs positions")
    best = rt.mask_pairs(mask, n_epochs, op=op, mode="best", rank=rank, positions_a=positions, d2_min=d2_min, d2_max=d2_max,
                         n_rows=n_rows, stats=stats)
    own = rt.mask_pairs(mask, n_epochs, mode="rows", n_rows=n_rows, stats=stats)
    return SitePairs(best, own, n_epochs, rank)


class GreedySites:
    """What greedy_sites returns: sites, the chosen row indices in the order they were chosen; records (len(sites),) PAIR_DTYPE,
    the union's record after each step (partner = -1); n_epochs.  complete: the union holds every epoch."""

    def __init__(self, sites, records, n_epochs):
        self.sites = np.asarray(sites, np.int64)
        self.records = np.array(records, _lib.PAIR_DTYPE)
        self.n_epochs = int(n_epochs)

    @property
    def complete(self):
        return len(self.records) > 0 and int(self.records["count"][-1]) == self.n_epochs


def _mask_row(mask, i, w64):
    """Row i of a mask table, an array or a DeviceBuffer."""
    if isinstance(mask, np.ndarray) or not hasattr(mask, "ptr"):
        return np.ascontiguousarray(mask, np.uint64).reshape(-1, w64)[i].copy()
    row = np.empty(w64, np.uint64)
    rc = _lib.load().mrtx_dev_download(mask.device, row.ctypes.data, mask.ptr + 8 * w64 * int(i), row.nbytes)
    if rc != 0:
        raise RuntimeError(f"device download failed (code {rc})")
    return row


def greedy_sites(rt, mask, n_epochs, k, positions=None, within_m=None, rank="count", unit_m=1.0, n_rows=None, stats=None):
    """A set of up to k <= 64 sites grown one at a time: each step is a MoonRT.mask_pairs call in mode "rows" with base = the
    union of the rows chosen so far, and the host takes the first row under the rank ("count": largest count, then smallest
    gap, then least index; "gap": smallest gap, then largest count, then least index) among the rows not yet chosen.  With
    within_m, from the second site on only rows within that distance of a chosen site are taken: positions, an (n, 3) integer
    array in units of unit_m metres, compared as d2 <= floor((within_m / unit_m)^2) in integers.  Stops early when the union
    holds every epoch, or when no row is left.  Returns a GreedySites."""
    k = int(k)
    if k < 1 or k > 64:
        raise ValueError("k must lie in 1 .. 64")
    if rank not in ("count", "gap"):
        raise ValueError('rank must be "count" or "gap"')
    m = int(n_epochs)
    w64 = (m + 63) // 64
    pos = d2_within = None
    if within_m is not None:
        if positions is None or hasattr(positions, "ptr"):
            raise ValueError("within_m needs positions as an (n, 3) integer array")
        pos = np.asarray(positions).astype(np.int64)
        d2_within = distance_d2(float(within_m), float(unit_m), False)
    base = None
    sites, records = [], []
    near = None
    for _ in range(k):
        rec = rt.mask_pairs(mask, m, mode="rows", base=base, n_rows=n_rows, stats=stats)
        free = np.ones(len(rec), bool)
        free[sites] = False
        if near is not None:
            free &= near
        cand = np.flatnonzero(free)
        if cand.size == 0:
            break
        pick = int(cand[_rank_order(rec[cand], rank, cand)[0]])
        sites.append(pick)
        records.append(rec[pick])
        row = _mask_row(mask, pick, w64)
        base = row if base is None else base | row
        if pos is not None:
            d = pos - pos[pick]
            d2 = (d * d).sum(-1)                    # at most 3 x 2^60: int64 holds it
            close = np.array([int(v) <= d2_within for v in d2], bool)
            near = close if near is None else near | close
        if int(rec["count"][pick]) == m:
            break
    return GreedySites(sites, records, m)
