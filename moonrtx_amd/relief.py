"""Terrain relief: the map MoonRT.relief returns -- slope, roughness and the gradient of the
least-squares plane under a footprint -- and the split of a window into row bands of constant footprint when the footprint is
given in metres."""
import ctypes as C
import math

import numpy as np

from . import _lib
from .traverse import window_dict

R_MAX = 32          # the largest footprint half-height the library accepts, lattice nodes
BOX_MAX = 1024      # the largest half-height of a landing ellipse's box, map nodes


def relief_window(w, ri=1, rj=1, radius_m=1737400.0, rows=None):
    """The MrtxRelief of a window dict (rows = (first, count): only those rows of it)."""
    i0, n = (0, w["rows"]) if rows is None else rows
    return _lib.MrtxRelief(w["row0"] + i0 * w["stride"], w["col0"], n, w["cols"], w["stride"], int(ri), int(rj), 0,
                           float(radius_m))


def scales(lib, t, dem_shape):
    """(rows, 2) float64 (kx, ky) of an MrtxRelief from mrtx_relief_scales; ValueError on a refused window."""
    out = np.empty((max(t.rows, 1), 2), np.float64)
    rc = lib.mrtx_relief_scales(C.byref(t), int(dem_shape[0]), int(dem_shape[1]), out.ctypes.data)
    if rc != 0:
        raise ValueError(f"mrtx_relief_scales refused the window or the footprint ({rc})")
    return out


def _nodes(half_m, spacing_m):
    return np.maximum(1, np.floor(np.asarray(half_m / spacing_m, np.float64) + 0.5).astype(np.int64))


def footprint_bands(lib, window, footprint_m, radius_m, dem_shape):
    """(ri, bands) of a footprint footprint_m metres across on a window: ri = max(1, round(footprint_m / 2 / L_ns)) from the
    N-S spacing of the lattice rows, and bands = [(first row, row count, rj)] that cover the window's rows in order, rj =
    max(1, round(footprint_m / 2 / L_ew)) constant over each (L_ew shrinks with cos(lat)).  ValueError, naming a stride that
    fits, when a row needs more than 32 nodes."""
    w = window_dict(window)
    f = float(footprint_m)
    if not (f > 0.0 and math.isfinite(f)):
        raise ValueError("footprint_m must be finite and > 0")
    k = scales(lib, relief_window(w, radius_m=radius_m), dem_shape)
    half_ns, half_ew = 0.5 * f * k[:, 1] / radius_m, 0.5 * f * k[:, 0] / radius_m      # half the footprint, in lattice nodes
    ri, rj = int(_nodes(half_ns[0], 1.0)), _nodes(half_ew, 1.0)
    worst = max(float(half_ns[0]), float(half_ew.max()))
    if ri > R_MAX or int(rj.max()) > R_MAX:
        s = w["stride"]
        fit = s + 1
        while math.floor(worst * s / fit + 0.5) > R_MAX:
            fit += 1
        raise ValueError(f"a {f:g} m footprint needs {max(ri, int(rj.max()))} lattice nodes either side at stride {s}, more than "
                         f"{R_MAX}: a stride of {fit} would fit")
    cuts = [0] + [int(i) for i in np.flatnonzero(np.diff(rj)) + 1] + [w["rows"]]
    return ri, [(a, b - a, int(rj[a])) for a, b in zip(cuts[:-1], cuts[1:])]


class ReliefMap:
    """What MoonRT.relief returns: grade (rise over run), rms_m (metres), ge and gn (the gradient to the east and to the
    north), each (rows, cols) float32; the window, radius_m, ri and the bands [(first row, row count, rj)] it was computed
    in; closes_circle: the window's columns go once round the DEM.  NaN where the footprint leaves the DEM's rows."""

    def __init__(self, table, window, radius_m, ri, bands, closes_circle=False, lat=None, lon=None):
        t = np.asarray(table, np.float32)
        self.window = window_dict(window)
        if t.shape != (self.window["rows"], self.window["cols"], 4):
            raise ValueError("the table must be (rows, cols, 4) float32")
        self.table = t
        self.grade, self.rms_m, self.ge, self.gn = (t[..., k] for k in range(4))
        self.radius_m, self.ri, self.bands = float(radius_m), int(ri), list(bands)
        self.closes_circle = bool(closes_circle)
        self.lat, self.lon = lat, lon

    @property
    def slope_deg(self):
        return np.degrees(np.arctan(self.grade.astype(np.float64)))

    @property
    def aspect_deg(self):
        """The azimuth of steepest descent, degrees from north through east; NaN on level ground."""
        ge, gn = self.ge.astype(np.float64), self.gn.astype(np.float64)
        az = np.degrees(np.arctan2(-ge, -gn)) % 360.0
        return np.where((ge == 0.0) & (gn == 0.0), np.nan, az)
