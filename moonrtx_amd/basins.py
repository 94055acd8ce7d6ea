"""Terrain depressions: integer heights, the fill map and the basin records."""
import numpy as np

from ._lib import FILL_NONE, FILL_ZMAX

# MrtxBasin, field for field (48 bytes)
BASIN_DTYPE = np.dtype([("weight", "<u8"), ("volume", "<u8"), ("count", "<u4"), ("level_min", "<i4"), ("level_max", "<i4"),
                        ("depth_max", "<i4"), ("deepest_at", "<i4"), ("pour_at", "<i4"), ("pour_level", "<i4"),
                        ("reserved", "<u4")])
assert BASIN_DTYPE.itemsize == 48


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


__all__ = ["BASIN_DTYPE", "FILL_NONE", "FILL_ZMAX", "FillMap", "depth_of", "quantise_heights"]
