"""Terrain depressions (DESIGN.md sections 3.24, 3.25): integer heights, the fill map, the basin records and the tree of bowls."""
import numpy as np

from ._lib import FILL_NONE, FILL_ZMAX

# MrtxBasin, field for field (48 bytes)
BASIN_DTYPE = np.dtype([("weight", "<u8"), ("volume", "<u8"), ("count", "<u4"), ("level_min", "<i4"), ("level_max", "<i4"),
                        ("depth_max", "<i4"), ("deepest_at", "<i4"), ("pour_at", "<i4"), ("pour_level", "<i4"),
                        ("reserved", "<u4")])
assert BASIN_DTYPE.itemsize == 48

# MrtxBowl, field for field (64 bytes)
BOWL_DTYPE = np.dtype([("weight", "<u8"), ("volume", "<u8"), ("count", "<u4"), ("own_count", "<u4"), ("floor_at", "<i4"),
                       ("floor_level", "<i4"), ("born_at", "<i4"), ("born_level", "<i4"), ("spill_at", "<i4"),
                       ("spill_level", "<i4"), ("parent", "<i4"), ("n_children", "<u4"), ("n_leaves", "<u4"), ("reserved", "<u4")])
assert BOWL_DTYPE.itemsize == 64


def quantise_heights(heights_m, unit_m=0.01):
    """Heights in metres as int32 counts of unit_m: float64 rint (half to even) of heights_m / unit_m.  Raises ValueError on a
    height that is not finite or lies beyond +-2^30 units."""
    unit_m = float(unit_m)
    if not (np.isfinite(unit_m) and unit_m > 0.0):
        raise ValueError("unit_m must be finite and > 0")
    q = np.rint(np.asarray(heights_m, np.float64) / unit_m)
    if not np.isfinite(q).all():
        raise ValueError("a height is not finite")
    if q.size and (q.min() < -FILL_ZMAX or q.max() > FILL_ZMAX):
        raise ValueError("a height leaves +-2^30 units: choose a larger unit_m")
    return q.astype(np.int32)


def depth_of(fill, z):
    """int32 depths of any fill table: (int64)fill - z held in 0 .. INT32_MAX, as mrtx_fill_basins takes them."""
    d = np.asarray(fill, np.int64) - np.asarray(z, np.int64)
    return np.clip(d, 0, 2 ** 31 - 1).astype(np.int32)


class FillMap:
    """z and fill (rows, cols) int32 in units of unit_m (None: the caller's own unit); connectivity and wrap of the fill."""

    def __init__(self, z, fill, unit_m=None, connectivity=8, wrap=False):
        self.z = np.ascontiguousarray(z, np.int32)
        self.fill = np.ascontiguousarray(fill, np.int32)
        if self.z.ndim != 2 or self.z.shape != self.fill.shape:
            raise ValueError("z and fill must be (rows, cols) alike")
        self.unit_m = None if unit_m is None else float(unit_m)
        self.connectivity = int(connectivity)
        self.wrap = bool(wrap)

    def depth(self):
        """(rows, cols) int32: fill - z, 0 outside every depression."""
        return depth_of(self.fill, self.z)

    def _unit(self):
        if self.unit_m is None:
            raise ValueError("the map has no unit: make it with unit_m")
        return self.unit_m

    def depth_m(self):
        """(rows, cols) float64 depths in metres."""
        return self.depth().astype(np.float64) * self._unit()

    def mask(self, min_depth_m=0):
        """(rows, cols) uint8: 1 where the node lies in a depression deeper than min_depth_m (0: depth > 0)."""
        d = self.depth()
        if not min_depth_m:
            return (d > 0).astype(np.uint8)
        return (d.astype(np.float64) * self._unit() > float(min_depth_m)).astype(np.uint8)

    def catalogue(self, rt, row_weights=None, min_depth_m=0, stats=None):
        """(RegionMap, (n,) BASIN_DTYPE): the connected components of mask(min_depth_m), labelled by rt.regions at the fill's
        connectivity and wrap, and their basin records (rt.basins).  With min_depth_m = 0 every record has level_min ==
        level_max == pour_level."""
        regions = rt.regions(mask=self.mask(min_depth_m), connectivity=self.connectivity, wrap=self.wrap, row_weights=row_weights,
                             stats=stats)
        return regions, rt.basins(regions.labels, regions.n, self, row_weights=row_weights, stats=stats)


class BowlTree:
    """The depression hierarchy of a lattice (mrtx_bowls): records (n,) BOWL_DTYPE numbered so that parent > child, labels
    (rows, cols) int32, the innermost bowl of every node or -1 (None when they were left out), z the heights, in units of
    unit_m (None: the caller's own unit).  invert: the bowls are peaks, the levels summits and key cols."""

    def __init__(self, records, labels, z, unit_m=None, connectivity=8, wrap=False, invert=False):
        self.records = np.ascontiguousarray(records, BOWL_DTYPE)
        self.z = np.ascontiguousarray(z, np.int32)
        self.labels = None if labels is None else np.ascontiguousarray(labels, np.int32)
        if self.z.ndim != 2 or (self.labels is not None and self.labels.shape != self.z.shape):
            raise ValueError("z and labels must be (rows, cols) alike")
        if self.records.ndim != 1:
            raise ValueError("records must be (n,)")
        self.unit_m = None if unit_m is None else float(unit_m)
        self.connectivity = int(connectivity)
        self.wrap = bool(wrap)
        self.invert = bool(invert)

    @property
    def n(self):
        return len(self.records)

    def depth(self):
        """(n,) int64: |spill_level - floor_level|, a bowl's depth or a peak's prominence."""
        return np.abs(self.records["spill_level"].astype(np.int64) - self.records["floor_level"].astype(np.int64))

    def children(self, b):
        """The indices of the direct children of bowl b, ascending."""
        return np.flatnonzero(self.records["parent"] == int(b))

    def roots(self):
        """The indices of the bowls without a parent, ascending."""
        return np.flatnonzero(self.records["parent"] < 0)

    def _up(self):
        parent = self.records["parent"].astype(np.int64)
        return np.where(parent < 0, np.arange(self.n), parent)

    def root_of(self):
        """(n,) int64: the root bowl above each bowl (itself for a root)."""
        r = self._up()
        while True:
            nxt = r[r]
            if (nxt == r).all():
                return r
            r = nxt

    def level(self):
        """(n,) int64: the number of ancestors of each bowl (0 for a root)."""
        lvl = np.zeros(self.n, np.int64)
        parent = self.records["parent"]
        for b in range(self.n - 1, -1, -1):                     # parent > child: a parent's level is final before its children's
            if parent[b] >= 0:
                lvl[b] = lvl[parent[b]] + 1
        return lvl

    def select(self, min_depth_m=0, min_area=0, min_count=0):
        """(n,) bool: the bowls at least min_depth_m deep (needs unit_m unless 0), of weight >= min_area (the unit of the row
        weights) and of count >= min_count.  The zero-depth bowls of a flat go with any min_depth_m > 0."""
        r = self.records
        keep = (r["weight"] >= min_area) & (r["count"] >= min_count)
        if min_depth_m:
            if self.unit_m is None:
                raise ValueError("the tree has no unit: make it with unit_m")
            keep &= self.depth().astype(np.float64) * self.unit_m >= float(min_depth_m)
        return keep

    def target(self, selected, innermost=True):
        """(n,) int64: for each bowl the innermost (or outermost) selected bowl among itself and its ancestors, or -1."""
        sel = np.asarray(selected, bool)
        if sel.shape != (self.n,):
            raise ValueError("selected must be (n,) booleans")
        own = np.where(sel, np.arange(self.n), -1)
        up = self._up()
        if innermost:
            step = np.where(sel, np.arange(self.n), up)         # stop at a selected bowl, else climb
            while True:
                nxt = step[step]
                if (nxt == step).all():
                    break
                step = nxt
            return np.where(sel[step], step, -1) if self.n else own
        best = own
        while True:                                              # best: over 2^k bowls of the chain from b, the one furthest up
            above = best[up]
            new = np.where(above >= 0, above, best)
            nxt = up[up]
            if (new == best).all() and (nxt == up).all():
                return best
            best, up = new, nxt

    def relabel(self, selected, innermost=True):
        """((rows, cols) int32, (k,) int64): every node's innermost (or outermost) selected bowl on its chain as a compact id
        0 .. k - 1, else -1, and the bowl index of each id.  A label table for MoonRT.basins, region_outlines and proximity."""
        if self.labels is None:
            raise ValueError("the tree was made without labels")
        t = self.target(selected, innermost)
        bowl_of = np.unique(t[t >= 0])
        compact = np.full(self.n + 1, -1, np.int32)             # entry n: the nodes outside every bowl
        compact[bowl_of] = np.arange(len(bowl_of), dtype=np.int32)
        per_bowl = np.append(np.where(t >= 0, compact[np.maximum(t, 0)], -1).astype(np.int32), np.int32(-1))
        return per_bowl.take(np.where(self.labels >= 0, self.labels, self.n)), bowl_of

    def fill(self):
        """(rows, cols) int32: max(z, the spill level of the root bowl above the node's label), z outside every bowl: the
        table of mrtx_fill (with invert: min, the fill of the negated heights negated back)."""
        if self.labels is None:
            raise ValueError("the tree was made without labels")
        lv = np.append(self.records["spill_level"][self.root_of()], np.int32(0)).astype(np.int32)
        at = lv.take(np.where(self.labels >= 0, self.labels, self.n))
        out = np.minimum(self.z, at) if self.invert else np.maximum(self.z, at)
        return np.where(self.labels >= 0, out, self.z).astype(np.int32)


__all__ = ["BASIN_DTYPE", "BOWL_DTYPE", "BowlTree", "FILL_NONE", "FILL_ZMAX", "FillMap", "depth_of", "quantise_heights"]
