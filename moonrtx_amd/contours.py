"""Contour lines: what MoonRT.contours returns, and the float64 geometry of its integer lines."""
import numpy as np

from ._lib import CONTOUR_LINE_DTYPE, CONTOUR_MAX_LEVELS, FILL_NONE, FILL_ZMAX

VOID = FILL_NONE                # the height of a node without one


def levels_for(lo, hi, interval, offset=0):
    """The level table of a contour interval: every c = offset + k interval, k an integer, with lo < c <= hi, ascending, as
    int32.  Those are the levels that can cross a lattice whose valid heights span lo .. hi (a node is above c when z >= c).
    All in the integer units of the heights.  ValueError for an interval < 1 or more than 65536 levels."""
    lo, hi, interval, offset = int(lo), int(hi), int(interval), int(offset)
    if interval < 1:
        raise ValueError("interval must be >= 1 unit")
    lo, hi = max(lo, -FILL_ZMAX), min(hi, FILL_ZMAX)
    k0 = (lo - offset) // interval + 1              # the least k with offset + k interval > lo
    k1 = (hi - offset) // interval                  # the greatest with offset + k interval <= hi
    if k1 - k0 + 1 > CONTOUR_MAX_LEVELS:
        raise ValueError(f"{k1 - k0 + 1} levels: a call takes at most {CONTOUR_MAX_LEVELS} (choose a larger interval)")
    return (offset + interval * np.arange(k0, k1 + 1, dtype=np.int64)).astype(np.int32)


class Contours:
    """What MoonRT.contours returns: lines (n,) CONTOUR_LINE_DTYPE in ascending order of their heads; vertices (m,) int32 edge
    ids, line after line, each from its head along the successors with the above side on its right (rows run down, columns
    right); z (rows, cols) int32, the heights (VOID: no node); levels (n_levels,) int32; rows, cols, wrap: the lattice.  Edge
    2 v + 0 joins node v to its east neighbour, edge 2 v + 1 to its south neighbour."""

    def __init__(self, lines, vertices, z, levels, wrap=False):
        self.lines = np.ascontiguousarray(lines, CONTOUR_LINE_DTYPE).reshape(-1)
        self.vertices = np.ascontiguousarray(vertices, np.int32).reshape(-1)
        self.z = np.ascontiguousarray(z, np.int32)
        if self.z.ndim != 2:
            raise ValueError("z must be (rows, cols)")
        self.levels = np.ascontiguousarray(levels, np.int32).reshape(-1)
        self.rows, self.cols, self.wrap = int(self.z.shape[0]), int(self.z.shape[1]), bool(wrap)
        if int(self.lines["n_vertices"].astype(np.int64).sum()) != self.vertices.shape[0]:
            raise ValueError("the lines' n_vertices do not add up to the vertex table")
        self._order = np.argsort(self.lines["level_index"], kind="stable")
        self._sorted = self.lines["level_index"][self._order]

    def __len__(self):
        return int(self.lines.shape[0])

    def line(self, r):
        """(n_vertices,) int32: the edge ids of line r, a view of the vertex table."""
        rec = self.lines[int(r)]
        return self.vertices[int(rec["first"]):int(rec["first"]) + int(rec["n_vertices"])]

    def at(self, level_index):
        """The numbers of the lines of one level, ascending."""
        a, b = np.searchsorted(self._sorted, [int(level_index), int(level_index) + 1])
        return self._order[a:b].astype(np.int64)

    def _ends(self, r):
        """(i, j, k, t) per vertex of line r: the edge's own node, its direction (0 east, 1 south) and the crossing's place
        t in (0, 1) from the own node, float64."""
        e = self.line(r).astype(np.int64)
        c = int(self.lines[int(r)]["level"])
        v, k = e >> 1, e & 1
        i, j = v // self.cols, v % self.cols
        oi, oj = i + k, (j + 1 - k) % self.cols
        z0 = self.z[i, j].astype(np.int64)
        z1 = self.z[oi, oj].astype(np.int64)
        t = (2 * c - 1 - 2 * z0).astype(np.float64) / (2 * (z1 - z0)).astype(np.float64)
        return i, j, k, t

    def _steps(self, j):
        """The column steps in {-1, 0, +1} between consecutive vertices, and from the last back to the first."""
        d = np.roll(j, -1) - j
        if self.wrap:
            d = (d + 1) % self.cols - 1
        return d

    def xy(self, r):
        """(n_vertices, 2) float64 (y, x) of line r in node coordinates: t = (2 c - 1 - 2 z_own) / (2 (z_other - z_own)) from
        the edge's own node towards the other.  Under wrap x is unwrapped along the line by the cumulative sum of the column
        steps, so a line across the seam is continuous and x may leave 0 .. cols."""
        i, j, k, t = self._ends(r)
        if j.size:
            col = j[0] + np.concatenate([[0], np.cumsum(self._steps(j)[:-1])])
        else:
            col = j
        y = i.astype(np.float64) + np.where(k == 1, t, 0.0)
        x = col.astype(np.float64) + np.where(k == 0, t, 0.0)
        return np.stack([y, x], -1)

    def wind(self, r):
        """For a closed line: the net column steps round the line over cols, -1, 0 or +1 (0 without wrap).  ValueError for an
        open line."""
        if not self.lines[int(r)]["closed"]:
            raise ValueError(f"line {int(r)} is open")
        e = self.line(r).astype(np.int64)
        return int(self._steps((e >> 1) % self.cols).sum()) // self.cols

    def latlon(self, r, window, dem_hw):
        """(n_vertices, 2) float64 (lat, lon) degrees of line r, for a window (row0, col0, rows, cols[, stride[, wrap]]) of an
        (H, W) DEM with the nodes at texel centres: lat = 90 - (row0 + y stride + 1 / 2) 180 / H, lon = -180 + (col0 + x stride
        + 1 / 2) 360 / W.  lon is continuous along a line: the unwrapped x of a line across the seam gives longitudes beyond
        +-180, which the caller may reduce."""
        from .traverse import window_dict
        w = window_dict(window)
        H, W = (int(v) for v in dem_hw)
        if w["stride"] < 1 or H < 1 or W < 1:
            raise ValueError("empty window or DEM")
        p = self.xy(r)
        lat = 90.0 - (w["row0"] + p[:, 0] * w["stride"] + 0.5) * (180.0 / H)
        lon = -180.0 + (w["col0"] + p[:, 1] * w["stride"] + 0.5) * (360.0 / W)
        return np.stack([lat, lon], -1)


__all__ = ["CONTOUR_LINE_DTYPE", "Contours", "VOID", "levels_for"]
