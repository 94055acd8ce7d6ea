"""The terrain half of MoonRT: Sun illumination, horizons, power, occultation, passes, regolith temperatures, line of sight,
traverses and relief -- the Python side of csrc/mrtx_terrain_api.hip.  MoonRT (renderer.py) inherits these methods."""
import ctypes as C
import math

import numpy as np

from . import _lib
from ._calls import Calls, MoonRTError
from ._lib import MrtxPowerModel, MrtxStats


def _device_buffer():
    """DeviceBuffer as renderer.py exports it, looked up at call time as sunlight.py does: `renderer.DeviceBuffer` stays the one
    name a host test replaces to fake device memory for the terrain methods and their callers alike."""
    from . import renderer
    return renderer.DeviceBuffer


class TerrainCalls(Calls):
    # ---- Sun illumination of the terrain
    @staticmethod
    def sun_samples(n):
        """The (u2, u3) float32 table of n Sun samples the illumination stage uses, (n, 2)."""
        out = np.empty((int(n), 2), np.float32)
        if _lib.load().mrtx_illum_sun_samples(int(n), out.ctypes.data) != 0:
            raise ValueError("n_sun must be 1, 2, 4, ..., 64")
        return out

    @staticmethod
    def grid_nodes(lat=(90.0, -90.0), lon=(-180.0, 180.0), shape=(180, 360)):
        """float64 (lat, lon) in degrees of the nodes of a map, the centres of its cells, computed as the library computes
        them -- a point list at these coordinates gives the map's values bit for bit."""
        (la_n, la_s), (lo_w, lo_e), (h, w) = (float(lat[0]), float(lat[1])), (float(lon[0]), float(lon[1])), shape
        dlat, dlon = (la_n - la_s) / h, (lo_e - lo_w) / w
        return la_n - (np.arange(h) + 0.5) * dlat, lo_w + (np.arange(w) + 0.5) * dlon

    def illumination_map(self, lat=(90.0, -90.0), lon=(-180.0, 180.0), shape=(180, 360), n_sun=16, rows=None, stats=None,
                         band_bytes=256 << 20):
        """(rows, w, 4) float32 map of (lit, irr, mu, D) over lat = (north, south), lon = (west, east) in degrees with
        shape = (h, w) cells; rows = (first, end) computes that band only (default: all).  Bands of at most band_bytes go
        through one device buffer.  `stats`, if a dict, receives the summed counters of the launches."""
        h, w = int(shape[0]), int(shape[1])
        r0, r1 = (0, h) if rows is None else (int(rows[0]), int(rows[1]))
        g = _lib.MrtxIllumGrid(float(lat[0]), float(lat[1]), float(lon[0]), float(lon[1]), h, w, r0, r1, int(n_sun), 0)
        return self._band_map("mrtx_illum_grid", g, np.empty((max(r1 - r0, 0), w, 4), np.float32), 16, band_bytes, stats)

    def _band_map(self, name, g, out, node_bytes, band_bytes, stats):
        """Rows [g.row_begin, g.row_end) of a map of node_bytes per node into `out` through the grid call `name`: in one call
        straight into `out` when they fit in band_bytes, else in bands of that size through one device buffer."""
        r0, r1, w = g.row_begin, g.row_end, g.w
        step = max(1, int(band_bytes) // (node_bytes * max(w, 1)))
        call = getattr(self._lib, name)
        if r1 - r0 <= step:      # one band: straight into the host array
            st = MrtxStats()
            self._check(call(self._ctx, C.byref(g), None, out.ctypes.data, C.byref(st)), name)
            self._add_stats(stats, st)
            return out
        buf = _device_buffer()(node_bytes * step * w, self.config()["device"])
        try:
            for a in range(r0, r1, step):
                g.row_begin, g.row_end = a, min(a + step, r1)
                st = MrtxStats()
                self._check(call(self._ctx, C.byref(g), buf.ptr, None, C.byref(st)), name)
                self._add_stats(stats, st)
                out[a - r0:g.row_end - r0] = buf.download(np.float32, (g.row_end - a,) + out.shape[1:])
        finally:
            buf.free()
        return out

    def illumination_at(self, lat_deg, lon_deg, n_sun=16, stats=None):
        """(N, 4) float32 (lit, irr, mu, D) at N selenographic points (degrees): the status bar's Sun altitude
        (renderer_status.py:121-157) on the real terrain."""
        la, lo = self._points(lat_deg, lon_deg)
        pts = np.ascontiguousarray(np.stack([la, lo], -1))
        out = np.empty((la.size, 4), np.float32)
        st = MrtxStats()
        self._check(self._lib.mrtx_illum_points(self._ctx, pts.ctypes.data, la.size, int(n_sun), out.ctypes.data, C.byref(st)),
                    "mrtx_illum_points")
        self._add_stats(stats, st)
        return out

    def illumination_series(self, lat_deg, lon_deg, epochs, n_sun=16, first=None, count=None, stats=None, chunk_bytes=256 << 20):
        """(N, count, 4) float32 (lit, irr, mu, D) at N points over many dates: entry (p, j) is what
        illumination_at gives at point p after the light and Moon frame of epoch first[p] + j were set, bit for bit.
        `epochs`: the (m, 14) float64 array of ephemeris.sun_epochs, or a sequence of SceneDesc.  first = None: every point
        reads epochs [0, count) (count defaults to m); otherwise N window starts and count is required.  Calls hold at most
        chunk_bytes of output each (points split between calls); `stats`, if a dict, receives the summed counters."""
        la, lo = self._points(lat_deg, lon_deg)
        ep = self._epochs(epochs)
        if first is None:
            count = ep.shape[0] if count is None else int(count)
        else:
            if count is None:
                raise ValueError("count is required with first")
            first = np.ascontiguousarray(np.atleast_1d(np.asarray(first)).ravel(), np.int32)
            if first.shape != la.shape:
                raise ValueError("first must hold one window start per point")
            count = int(count)
        out = np.empty((la.size, max(count, 0), 4), np.float32)

        def call(pts, a, b, dh, hh, st):
            return self._lib.mrtx_illum_series(self._ctx, pts, b - a, ep.ctypes.data, ep.shape[0],
                                               None if first is None else first[a:].ctypes.data, count, int(n_sun), None,
                                               out[a:].ctypes.data, st)
        self._point_calls("mrtx_illum_series", call, la, lo, max(count, 1), chunk_bytes, stats, out_bytes=16, empty_call=False)
        return out

    @staticmethod
    def _points(lat_deg, lon_deg):
        la = np.atleast_1d(np.asarray(lat_deg, np.float64)).ravel()
        lo = np.atleast_1d(np.asarray(lon_deg, np.float64)).ravel()
        if la.shape != lo.shape:
            raise ValueError("lat_deg and lon_deg must have the same number of points")
        return la, lo

    @staticmethod
    def _epochs(epochs):
        from .ephemeris import epoch_of_scene
        if not isinstance(epochs, np.ndarray):
            epochs = np.array([epoch_of_scene(e) for e in epochs], np.float64).reshape(-1, 14)
        ep = np.ascontiguousarray(epochs, np.float64)
        if ep.ndim != 2 or ep.shape[1] != 14:
            raise ValueError("epochs must be an (m, 14) array (ephemeris.sun_epochs) or a sequence of SceneDesc")
        return ep

    @staticmethod
    def horizon_azimuths(n_az):
        """Azimuths of the n_az horizon samples, degrees from north through east: a * 360 / n_az."""
        n = int(n_az)
        if n < 4 or n > 4096 or n & (n - 1):
            raise ValueError(f"n_az must be 4, 8, ..., 4096 (got {n_az})")
        return np.arange(n, dtype=np.float64) * (360.0 / n)

    def horizon(self, lat_deg, lon_deg, n_az=256, n_bis=14, stats=None, out=None, chunk_bytes=256 << 20, height_m=None,
                radius_m=1737400.0):
        """(N, n_az) float32: the terrain's horizon elevation, degrees, seen from N points (degrees) at horizon_azimuths(n_az),
        found by n_bis bisection probes that are each an illumination sample's visibility decision.
        out = a DeviceBuffer of at least N * n_az * 4 bytes: the horizons are written there (point-major) and `out` is
        returned.  Calls hold at most chunk_bytes of output each (points split between calls); `stats`, if a dict, receives
        the summed counters.  height_m (one value, or one per point, metres in [0, 1e4]): the horizon seen from a mast top that
        high above each point, line_of_sight's raised end (section 3.15; radius_m = the metres of D = 1); a height of 0 gives
        the ground's horizon bit for bit, None makes the ground-only call."""
        la, lo = self._points(lat_deg, lon_deg)
        n_az = int(n_az)
        hts = None
        if height_m is not None:
            hts = np.asarray(height_m, np.float64)
            if hts.ndim == 0:
                hts = np.full(la.size, float(hts))
            hts = np.ascontiguousarray(hts.ravel())
            if hts.size != la.size:
                raise ValueError("height_m must be one height or one per point")
        if out is not None and out.nbytes < la.size * max(n_az, 0) * 4:
            raise ValueError("the device buffer is smaller than N x n_az float32")
        host = np.empty((la.size, max(n_az, 0)), np.float32) if out is None else None

        def call(pts, a, b, dh, hh, st):
            dev = None if out is None else out.ptr + a * n_az * 4
            hp = None if out is not None else host[a:].ctypes.data
            if hts is None:
                return self._lib.mrtx_horizon_points(self._ctx, pts, b - a, n_az, int(n_bis), dev, hp, st)
            return self._lib.mrtx_horizon_raised(self._ctx, pts, hts[a:].ctypes.data, float(radius_m), b - a, n_az, int(n_bis), dev,
                                                 hp, st)
        self._point_calls("mrtx_horizon_points" if hts is None else "mrtx_horizon_raised", call, la, lo, max(n_az, 1), chunk_bytes,
                          stats)
        return out if out is not None else host

    WINDOW_COLUMNS = ("share_a", "longest_out_a", "share_b", "longest_out_b", "share_both", "longest_both", "first_both",
                      "longest_out_both")

    def horizon_windows(self, lat_deg, lon_deg, horizon, epochs_a, epochs_b, min_a=0.5, min_b=1.0, n_az=None, stats=None,
                        chunk_bytes=256 << 20):
        """Two bodies against the horizons of `horizon`, reduced per point on the device: with f_a,
        f_b horizon_sun's fractions for the epoch tables epochs_a, epochs_b (the same m dates), ok_a = f_a >= min_a,
        ok_b = f_b >= min_b and both = ok_a and ok_b, the (N, 8) float32 columns WINDOW_COLUMNS: the share of epochs with ok_a
        and the longest run of epochs without it, the same for b, the share with both, the longest run with both and the index
        of its first epoch (the earliest such run; -1 if there is none), the longest run without both.  Runs are in epochs.
        `horizon` as for horizon_sun.  No (N, m) table exists anywhere; calls hold at most chunk_bytes of horizons and
        output."""
        la, lo = self._points(lat_deg, lon_deg)
        ea, eb = self._epochs(epochs_a), self._epochs(epochs_b)
        if ea.shape != eb.shape:
            raise ValueError("epochs_a and epochs_b must hold the same number of epochs")
        m = ea.shape[0]
        n_az, hz_at = self._horizon_arg(horizon, la.size, n_az)
        res = np.empty((la.size, 8), np.float32)

        def call(pts, a, b, dh, hh, st):
            return self._lib.mrtx_horizon_windows(self._ctx, pts, b - a, n_az, dh, hh, ea.ctypes.data, eb.ctypes.data, m,
                                                  float(min_a), float(min_b), None, res[a:].ctypes.data, st)
        self._point_calls("mrtx_horizon_windows", call, la, lo, max(int(n_az), 0) + 8, chunk_bytes, stats, hz_at)
        return res

    def horizon_mask(self, lat_deg, lon_deg, horizon, epochs_a, epochs_b=None, min_a=0.5, min_b=1.0, n_az=None, out=None,
                     stats=None, chunk_bytes=256 << 20, out_offset=0):
        """horizon_windows' joint predicate kept as bits (mrtx_horizon_mask): an (N, W64) uint64
        array, W64 = (m + 63) // 64, in which bit k & 63 of word k >> 6 of row p says that at epoch k point p has
        f_a >= min_a and f_b >= min_b (f = horizon_sun's fractions; equality counts as met).  epochs_b = None: ok_a alone.
        The bits past epoch m - 1 are 0.  out = a DeviceBuffer: the words are written there from byte out_offset (a multiple
        of 8) on, point-major, and `out` is returned.  `horizon` as for horizon_sun; calls hold at most chunk_bytes of
        horizons and output.  moonrtx_amd.traverse.unpack_mask turns rows into booleans."""
        la, lo = self._points(lat_deg, lon_deg)
        ea = self._epochs(epochs_a)
        eb = None if epochs_b is None else self._epochs(epochs_b)
        if eb is not None and ea.shape != eb.shape:
            raise ValueError("epochs_a and epochs_b must hold the same number of epochs")
        m = ea.shape[0]
        w64 = (m + 63) // 64
        n_az, hz_at = self._horizon_arg(horizon, la.size, n_az)
        out_offset = int(out_offset)
        if out is not None and (out_offset < 0 or out_offset % 8 or out.nbytes < out_offset + la.size * w64 * 8):
            raise ValueError("the device buffer is smaller than N x W64 uint64 from out_offset (a multiple of 8) on")
        res = np.empty((la.size, w64), np.uint64) if out is None else None

        def call(pts, a, b, dh, hh, st):
            dev = None if out is None else out.ptr + out_offset + a * w64 * 8
            hp = None if out is not None else res[a:].ctypes.data
            return self._lib.mrtx_horizon_mask(self._ctx, pts, b - a, n_az, dh, hh, ea.ctypes.data,
                                               None if eb is None else eb.ctypes.data, m, float(min_a), float(min_b), dev, hp, st)
        self._point_calls("mrtx_horizon_mask", call, la, lo, max(int(n_az), 0) + 2 * max(w64, 1), chunk_bytes, stats, hz_at)
        return out if out is not None else res

    # ---- Joint availability of mask rows
    PAIR_OPS = {"any": _lib.PAIRS_ANY, "both": _lib.PAIRS_BOTH}
    PAIR_MODES = {"rows": _lib.PAIRS_ROWS, "best": _lib.PAIRS_BEST, "table": _lib.PAIRS_TABLE}
    PAIR_RANKS = {"count": _lib.PAIRS_BY_COUNT, "gap": _lib.PAIRS_BY_GAP}

    @staticmethod
    def _mask_rows(mask, w64, n_rows, name):
        """A table of mask rows as (device pointer, host pointer, rows, the array kept alive)."""
        if isinstance(mask, _device_buffer()):
            if n_rows is None:
                raise ValueError(f"{name} is a DeviceBuffer: give its number of rows")
            n = int(n_rows)
            if n < 1 or mask.nbytes < 8 * n * w64:
                raise ValueError(f"the {name} buffer is smaller than its rows x W64 uint64")
            return mask.ptr, None, n, None
        a = np.ascontiguousarray(mask, np.uint64)
        if a.ndim == 1:
            a = a.reshape(1, -1)
        if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] != w64:
            raise ValueError(f"{name} must be (rows, {w64}) uint64 words for its epochs (got {a.shape})")
        if n_rows is not None and int(n_rows) != a.shape[0]:
            raise ValueError(f"{name} holds {a.shape[0]} rows, not {n_rows}")
        return None, a.ctypes.data, a.shape[0], a

    @staticmethod
    def _pair_positions(pos, n, name):
        from .regions import COORD_MAX
        if isinstance(pos, _device_buffer()):
            if pos.nbytes < 12 * n:
                raise ValueError(f"the {name} buffer is smaller than rows x 3 int32")
            return pos.ptr, None, None
        p = np.ascontiguousarray(pos)
        if p.shape != (n, 3) or not np.issubdtype(p.dtype, np.integer):
            raise ValueError(f"{name} must be (rows, 3) integers")
        if p.size and (p.min() < -COORD_MAX or p.max() > COORD_MAX):
            raise ValueError("a coordinate leaves +-2^29: choose a larger unit")
        p = p.astype(np.int32)
        return None, p.ctypes.data, p

    def mask_pairs(self, mask_a, n_epochs, mask_b=None, op="any", mode="best", rank="count", base=None, positions_a=None,
                   positions_b=None, d2_min=0, d2_max=2 ** 64 - 1, out=None, stats=None, n_rows=None, n_rows_b=None,
                   out_offset=0):
        """The joint availability of pairs of mask rows (mrtx_mask_pairs).  mask_a: (n_a, W64) uint64
        rows in horizon_mask's layout over n_epochs epochs, W64 = (n_epochs + 63) // 64, or a DeviceBuffer of them (then
        n_rows= is required); mask_b: a second table (n_rows_b= with a buffer), or None: the rows of mask_a against each
        other, a row never against itself.  The joint row of (a, b) is ((A[a] op B[b]) | base) over the first n_epochs bits:
        op "any" (either site available) or "both"; base an optional (W64,) row or DeviceBuffer.  Of it: count, the set
        bits; gap, the longest run of clear bits; gap_first, the start of the earliest such run (-1 when gap == 0).
        positions_a / positions_b: (rows, 3) integers within +-2^29 (networks.point_positions) or DeviceBuffers of int32;
        with them only pairs with d2_min <= d2 <= d2_max (the exact squared distance, both ends inclusive) are eligible.
          mode "rows"   (n_a,) PAIR_DTYPE of (A[a] | base) itself, partner = -1; no mask_b and no positions
          mode "best"   (n_a,) PAIR_DTYPE: the eligible partner first under rank "count" (largest count, then smallest gap,
                        then least b) or "gap" (smallest gap, then largest count, then least b), and that pair's fields;
                        (-1, 0, 0, -1) without an eligible partner
          mode "table"  (n_a, n_b) PAIR_TABLE_DTYPE, ineligible pairs all ones; at most 2^28 pairs
        out = a DeviceBuffer: the records are written there from byte out_offset (a multiple of 8) on and `out` is returned;
        otherwise the structured array.  `stats`, if a dict, receives kernel_ms, launches and pairs, the eligible pairs
        evaluated.  Needs no DEM."""
        for value, names, what in ((op, self.PAIR_OPS, "op"), (mode, self.PAIR_MODES, "mode"), (rank, self.PAIR_RANKS, "rank")):
            if value not in names:
                raise ValueError(f"{what} must be one of {sorted(names)} (got {value!r})")
        m = int(n_epochs)
        if m < 1 or m > 1 << 24:
            raise ValueError("n_epochs must lie in 1 .. 2^24")
        w64 = (m + 63) // 64
        a_dev, a_host, n_a, keep_a = self._mask_rows(mask_a, w64, n_rows, "mask_a")
        b_dev = b_host = keep_b = None
        n_b = 0
        if mask_b is not None:
            b_dev, b_host, n_b, keep_b = self._mask_rows(mask_b, w64, n_rows_b, "mask_b")
        if mode == "rows" and (mask_b is not None or positions_a is not None or positions_b is not None):
            raise ValueError('mode "rows" takes no mask_b and no positions')
        if (positions_b is not None) != (positions_a is not None and mask_b is not None):
            raise ValueError("give positions_b iff positions_a is given and mask_b is")
        base_dev = base_host = keep_base = None
        if isinstance(base, _device_buffer()):
            if base.nbytes < 8 * w64:
                raise ValueError("the base buffer is smaller than W64 uint64")
            base_dev = base.ptr
        elif base is not None:
            keep_base = np.ascontiguousarray(base, np.uint64).reshape(-1)
            if keep_base.shape != (w64,):
                raise ValueError(f"base must be one row of {w64} uint64 words")
            base_host = keep_base.ctypes.data
        pa = (None, None, None) if positions_a is None else self._pair_positions(positions_a, n_a, "positions_a")
        pb = (None, None, None) if positions_b is None else self._pair_positions(positions_b, n_b, "positions_b")
        d2_min, d2_max = int(d2_min), int(d2_max)
        if not (0 <= d2_min < 1 << 64 and 0 <= d2_max < 1 << 64):
            raise ValueError("d2_min and d2_max must fit uint64")
        cols = n_b if mask_b is not None else n_a
        table = mode == "table"
        if table and n_a * cols > 1 << 28:
            raise ValueError("a table holds at most 2^28 pairs")
        dtype, shape = (_lib.PAIR_TABLE_DTYPE, (n_a, cols)) if table else (_lib.PAIR_DTYPE, (n_a,))
        out_offset = int(out_offset)
        nbytes = dtype.itemsize * n_a * (cols if table else 1)
        if out is not None and (out_offset < 0 or out_offset % 8 or out.nbytes < out_offset + nbytes):
            raise ValueError("the device buffer is smaller than the records from out_offset (a multiple of 8) on")
        res = np.empty(shape, dtype) if out is None else None
        p = _lib.MrtxMaskPairs(n_a, n_b, m, self.PAIR_OPS[op], self.PAIR_MODES[mode], self.PAIR_RANKS[rank], (C.c_int32 * 2)(0, 0),
                               d2_min, d2_max)
        st = MrtxStats()
        pairs = C.c_uint64(0)
        self._check(self._lib.mrtx_mask_pairs(self._ctx, C.byref(p), a_dev, a_host, b_dev, b_host, base_dev, base_host, pa[0], pa[1],
                                              pb[0], pb[1], None if out is None else out.ptr + out_offset,
                                              None if out is not None else res.ctypes.data, C.byref(pairs), C.byref(st)),
                    "mrtx_mask_pairs")
        self._add_stats(stats, st)
        if isinstance(stats, dict):
            stats["pairs"] = stats.get("pairs", 0) + int(pairs.value)
        return out if out is not None else res

    POWER_COLUMNS = ("generated", "net", "storage_need", "drawdown_first", "drawdown_last", "min_charge", "epochs_unmet",
                     "energy_unmet")
    PANELS = {"track": _lib.PANEL_TRACK, "fixed": _lib.PANEL_FIXED, "azimuth": _lib.PANEL_AZIMUTH}

    @staticmethod
    def power_scale(gen_w, load_w):
        """The largest cpw_log2 in [-20, 20] that keeps both tables, as float32 watts times 2^cpw_log2, at or below 2^28 counts
        (DESIGN.md section 3.17); ValueError if even 2^-20 counts per watt does not."""
        top = max(float(np.max(np.asarray(gen_w, np.float64).astype(np.float32), initial=0.0)),
                  float(np.max(np.asarray(load_w, np.float64).astype(np.float32), initial=0.0)))
        if not top > 0.0:
            return 20
        if not math.isfinite(top):
            raise ValueError("gen_w and load_w must be finite")
        mant, exp = math.frexp(top)             # top = mant * 2^exp, mant in [0.5, 1)
        e = (29 if mant == 0.5 else 28) - exp
        if e < -20:
            raise ValueError("gen_w or load_w exceeds 2^28 counts at 2^-20 counts per watt")
        return min(e, 20)

    def power_budget(self, lat_deg, lon_deg, horizon, epochs, gen_w, load_w, panel="track", normal_enu=None, cpw_log2=None,
                     capacity=0, initial=None, mode="summary", n_az=None, stats=None, chunk_bytes=256 << 20):
        """The energy balance of a solar-powered asset at N points against the horizons of `horizon`, in integer counts of
        2^-cpw_log2 W x the epoch spacing.  gen_w[k]: the watts the array delivers facing the whole
        Sun at epoch k; load_w[k]: the watts drawn (one value or one per epoch).  panel: "track" (two-axis), "fixed" (normal
        normal_enu in each point's east, north, up) or "azimuth" (a vertical panel turned toward the Sun).  capacity and
        initial are counts (initial=None: full); cpw_log2=None picks power_scale's.  mode "summary": (N, 8) int64 columns
        POWER_COLUMNS -- the generated and the net energy, the least capacity that starting full never empties, the first and
        last epoch of that drawdown (-1: none), the lowest state of charge, the epochs whose load was not met and the energy
        not delivered; mode "full": (N, m) int32 generated counts G_k.  `horizon` as for horizon_sun; SUMMARY forms no (N, m)
        table anywhere."""
        la, lo = self._points(lat_deg, lon_deg)
        ep = self._epochs(epochs)
        m = ep.shape[0]
        gen = np.ascontiguousarray(np.broadcast_to(np.asarray(gen_w, np.float64), (m,)))
        load = np.ascontiguousarray(np.broadcast_to(np.asarray(load_w, np.float64), (m,)))
        if mode not in ("summary", "full"):
            raise ValueError(f"mode must be 'summary' or 'full' (got {mode!r})")
        if panel not in self.PANELS:
            raise ValueError(f"panel must be one of {sorted(self.PANELS)} (got {panel!r})")
        if (panel == "fixed") != (normal_enu is not None):
            raise ValueError("normal_enu goes with panel='fixed', and only with it")
        md = MrtxPowerModel()
        md.panel = self.PANELS[panel]
        md.normal_enu[:] = [float(x) for x in (normal_enu if normal_enu is not None else (0.0, 0.0, 1.0))]
        md.cpw_log2 = self.power_scale(gen, load) if cpw_log2 is None else int(cpw_log2)
        md.capacity = int(capacity)
        md.initial = int(capacity) if initial is None else int(initial)
        n_az, hz_at = self._horizon_arg(horizon, la.size, n_az)
        full = mode == "full"
        res = np.empty((la.size, m), np.int32) if full else np.empty((la.size, 8), np.int64)

        def call(pts, a, b, dh, hh, st):
            return self._lib.mrtx_power_budget(self._ctx, pts, b - a, n_az, dh, hh, ep.ctypes.data, gen.ctypes.data,
                                               load.ctypes.data, m, C.byref(md), 0 if full else 1, None, res[a:].ctypes.data, st)
        per = max(m, 1) if full else max(int(n_az), 0) + 16
        self._point_calls("mrtx_power_budget", call, la, lo, per, chunk_bytes, stats, hz_at)
        return res

    def horizon_sun(self, lat_deg, lon_deg, horizon, epochs, summary=False, stats=None, n_az=None, chunk_bytes=256 << 20):
        """The Sun against the horizons of `horizon`: per (point, epoch) the fraction of the light's
        disc above the point's horizon.  `horizon`: the (N, n_az) array of MoonRT.horizon, or a DeviceBuffer holding it
        (then n_az is required); `epochs` as for illumination_series.  summary=False: (N, m) float32 fractions;
        summary=True: (N, 4) float32 (mean fraction, share of epochs with any of the disc up, share with all of it up,
        longest run of consecutive epochs with none of it up, in epochs).  FULL calls hold at most chunk_bytes of output."""
        la, lo = self._points(lat_deg, lon_deg)
        ep = self._epochs(epochs)
        m = ep.shape[0]
        n_az, hz_at = self._horizon_arg(horizon, la.size, n_az)
        res = np.empty((la.size, 4 if summary else m), np.float32)

        def call(pts, a, b, dh, hh, st):
            return self._lib.mrtx_horizon_sun(self._ctx, pts, b - a, n_az, dh, hh, ep.ctypes.data, m, 1 if summary else 0, None,
                                              res[a:].ctypes.data, st)
        self._point_calls("mrtx_horizon_sun", call, la, lo, None if summary else max(m, 1), chunk_bytes, stats, hz_at)
        return res

    OCCULTATION_COLUMNS = ("mean", "min", "share_partial", "share_total", "longest_partial", "first_partial", "longest_total",
                           "eclipses")

    def occultation(self, lat_deg, lon_deg, source_epochs, body_epochs, summary=False, stats=None, chunk_bytes=256 << 20):
        """The Earth's occultation of the Sun: per (point, epoch) the share g of the source's disc
        that the body's disc leaves uncovered, seen from the point's vertex.  source_epochs: ephemeris.far_sun_epochs (the Sun
        at its true distance); body_epochs: ephemeris.earth_epochs, for the same m dates.  summary=False: (N, m) float32 g;
        summary=True: the (N, 8) float32 columns OCCULTATION_COLUMNS -- the mean and the least g, the shares of epochs with
        g < 1 and with g == 0, the longest run of epochs with g < 1 and its first epoch (the earliest such run; -1 if none),
        the longest run with g == 0, and the number of separate runs of g < 1 (the eclipses the point saw) -- with no (N, m)
        table anywhere.  The geometric discs only: no atmosphere.  FULL calls hold at most chunk_bytes of output."""
        la, lo = self._points(lat_deg, lon_deg)
        es, eb = self._epochs(source_epochs), self._epochs(body_epochs)
        if es.shape != eb.shape:
            raise ValueError("source_epochs and body_epochs must hold the same number of epochs")
        m = es.shape[0]
        res = np.empty((la.size, 8 if summary else m), np.float32)

        def call(pts, a, b, dh, hh, st):
            return self._lib.mrtx_occultation(self._ctx, pts, b - a, es.ctypes.data, eb.ctypes.data, m, 1 if summary else 0, None,
                                              res[a:].ctypes.data, st)
        self._point_calls("mrtx_occultation", call, la, lo, None if summary else max(m, 1), chunk_bytes, stats)
        return res

    PASS_COLUMNS = _lib.PASS_COLUMNS
    PASS_MODES = {"full": _lib.PASSES_FULL, "summary": _lib.PASSES_SUMMARY, "list": _lib.PASSES_LIST}

    def horizon_passes(self, lat_deg, lon_deg, horizon, positions_m, *, height_m=None, min_elev_deg=0.0, mode="summary",
                       n_az=None, radius_m=1737400.0, stats=None, chunk_bytes=256 << 20):
        """Relay orbiters against the horizons of `horizon` (mrtx_horizon_passes).  positions_m:
        (S, m, 3) or (m, 3) float64 metres in the Moon-fixed frame (orbits.fixed_from_latlon's axes), S <= 256 satellites at the
        same m epochs.  A satellite is in view where its margin g = es - max(horizon at its azimuth, min_elev_deg) is > 0; the
        direction is taken from the mast top height_m above each point (one value or one per point; None: the ground, the same
        bits as 0).  mode "full": (N, S, m, 4) float32 (elevation deg, azimuth deg in [0, 360), range m, g), the antenna
        pointing table; "summary": the (N, 8) float32 columns PASS_COLUMNS -- the share of epochs with a satellite in view, the
        longest outage and the longest contact in epochs, that contact's first epoch (-1: none), the number of contacts, the
        highest elevation in view (-90: none), the mean number in view and the share with two or more -- with no (N, S, m)
        table anywhere; "list": a _lib.PASS_DTYPE array, one record per pass in ascending (point, sat, first), counted in one
        call and filled by a second.  `horizon` as for horizon_sun; calls hold at most chunk_bytes of horizons and output."""
        la, lo = self._points(lat_deg, lon_deg)
        if mode not in self.PASS_MODES:
            raise ValueError(f"mode must be one of {sorted(self.PASS_MODES)} (got {mode!r})")
        pos = np.asarray(positions_m, np.float64)
        if pos.ndim == 2:
            pos = pos[None]
        if pos.ndim != 3 or pos.shape[2] != 3:
            raise ValueError("positions_m must be (S, m, 3) or (m, 3)")
        pos = np.ascontiguousarray(pos)
        S, m = int(pos.shape[0]), int(pos.shape[1])
        hts = None
        if height_m is not None:
            hts = np.ascontiguousarray(np.broadcast_to(np.asarray(height_m, np.float64).ravel(), (la.size,)))
        n_az, hz_at = self._horizon_arg(horizon, la.size, n_az)
        pts = np.ascontiguousarray(np.stack([la, lo], -1))
        k = _lib.MrtxPasses(S, m, self.PASS_MODES[mode], 0, float(radius_m), float(min_elev_deg))
        per = max(S * m, 1)
        # not a _point_calls query: each mode has a step rule of its own (2^27 records, not _chunks' 2^31 outputs), and a list
        # chunk is two calls whose records are renumbered and joined.
        if mode == "full":
            res = np.empty((la.size, S, m, 4), np.float32)
            step = max(1, min(int(chunk_bytes) // (16 * per), (1 << 27) // per))
        elif mode == "summary":
            res = np.empty((la.size, 8), np.float32)
            step = max(1, int(chunk_bytes) // (4 * (max(int(n_az), 0) + 8)))
        else:
            res = []
            step = max(1, min(int(chunk_bytes) // (4 * max(int(n_az), 0) + 12 * S), (1 << 27) // max(S, 1)))
        total = C.c_uint64(0)
        for a in range(0, max(la.size, 1), step):
            b = min(a + step, la.size)
            dh, hh = hz_at(a)
            hp = None if hts is None else hts[a:].ctypes.data
            st = MrtxStats()

            def call(out_ptr, cap):
                self._check(self._lib.mrtx_horizon_passes(self._ctx, C.byref(k), pts[a:].ctypes.data, hp, b - a, n_az, dh, hh,
                                                          pos.ctypes.data, None, out_ptr, cap, C.byref(total), C.byref(st)),
                            "mrtx_horizon_passes")
                self._add_stats(stats, st)
            if mode != "list":
                call(res[a:].ctypes.data, 0)
                continue
            call(None, 0)
            if isinstance(stats, dict):
                stats["count_ms"] = stats.get("count_ms", 0.0) + st.kernel_ms
            part = np.zeros(max(int(total.value), 1), _lib.PASS_DTYPE)
            need = int(total.value)
            call(part.ctypes.data, need)
            if isinstance(stats, dict):
                stats["fill_ms"] = stats.get("fill_ms", 0.0) + st.kernel_ms
            part = part[:need]
            part["point"] += a
            res.append(part)
        return np.concatenate(res) if mode == "list" else res

    @staticmethod
    def thermal_grid(spacing_s=3600.0, spinup_lunations=None, resets=None, F=None):
        """The MrtxThermalModel of the default regolith for epochs `spacing_s` apart: the layer
        tables, n_sub steps per epoch from the stable step at F (default 0.5), spin-up blocks of one lunation.  Defaults:
        thermal.SPINUP_LUNATIONS lunations of spin-up, reset after each of the first thermal.RESETS."""
        from . import thermal
        return thermal.model(spacing_s, thermal.SPINUP_LUNATIONS if spinup_lunations is None else spinup_lunations,
                             thermal.RESETS if resets is None else resets, thermal.F_STEP if F is None else F)

    def surface_temperature(self, lat_deg, lon_deg, horizon, epochs, flux, model=None, mode="summary", stats=None, n_az=None,
                            chunk_bytes=256 << 20):
        """Regolith surface temperatures driven by the Sun against the horizons of `horizon`.
        `horizon`: the (N, n_az) array of MoonRT.horizon, or a DeviceBuffer holding it (then n_az is required); `epochs` as
        for horizon_sun, evenly spaced by model.spacing_s, the first model.n_spin of them spin-up; `flux`: the solar flux
        per epoch, W m^-2 (ephemeris.sun_flux); `model`: thermal_grid() (hourly epochs) unless given.
        mode "summary": (N, 4) float32 (max, min, mean surface temperature, mean bottom-node temperature over the recorded
        epochs); "full": (N, m - n_spin) float32 surface temperatures; "flux": (N, m) float32 absorbed flux, no stepping.
        FULL and FLUX calls hold at most chunk_bytes of output each; `stats`, if a dict, also receives newton_cap_hits."""
        modes = {"full": 0, "summary": 1, "flux": 2}
        if mode not in modes:
            raise ValueError(f"mode must be one of {sorted(modes)} (got {mode!r})")
        la, lo = self._points(lat_deg, lon_deg)
        ep = self._epochs(epochs)
        m = ep.shape[0]
        fl = np.ascontiguousarray(np.asarray(flux, np.float64).ravel())
        if fl.size != m:
            raise ValueError("flux must hold one value per epoch")
        model = self.thermal_grid() if model is None else model
        n_az, hz_at = self._horizon_arg(horizon, la.size, n_az)
        width = {"full": max(m - int(model.n_spin), 1), "summary": 4, "flux": m}[mode]
        res = np.empty((la.size, width), np.float32)

        def call(pts, a, b, dh, hh, st):
            return self._lib.mrtx_thermal(self._ctx, pts, b - a, n_az, dh, hh, ep.ctypes.data, fl.ctypes.data, m, C.byref(model),
                                          modes[mode], None, res[a:].ctypes.data, st)
        self._point_calls("mrtx_thermal", call, la, lo, None if mode == "summary" else width, chunk_bytes, stats, hz_at,
                          {"newton_cap_hits": "reserved"})
        return res

    @staticmethod
    def view_samples(k):
        """The (uh1, uh2) float32 table of the k view directions of view_hits, (k, 2)."""
        out = np.empty((int(k), 2), np.float32)
        if _lib.load().mrtx_view_dir_samples(int(k), out.ctypes.data) != 0:
            raise ValueError("K must be 16, 32, ..., 1024")
        return out

    def view_hits(self, lat_deg, lon_deg, k=64, stats=None, chunk_bytes=256 << 20):
        """What terrain N points see: K fixed cosine-weighted rays per point, each marched as a path's
        continuation ray.  Returns (hits, share): (N, K, 2) float32 (lat, lon) in degrees of each ray's first terrain hit, NaN
        for sky, and (N,) float32 terrain view factors (hits / K).  Calls hold at most chunk_bytes of output each."""
        la, lo = self._points(lat_deg, lon_deg)
        k = int(k)
        hits = np.empty((la.size, max(k, 0), 2), np.float32)
        share = np.empty(la.size, np.float32)
        width = 2 * max(k, 1) + 1

        def call(pts, a, b, dh, hh, st):       # a chunk's hits and shares come in one buffer, taken apart once the call succeeded
            buf = np.empty((b - a) * width, np.float32) if b > a else np.empty(width, np.float32)
            rc = self._lib.mrtx_view_hits(self._ctx, pts, b - a, k, None, buf.ctypes.data, st)
            if rc == 0:
                hits[a:b] = buf[:(b - a) * 2 * k].reshape(b - a, k, 2)
                share[a:b] = buf[(b - a) * 2 * k:(b - a) * width]
            return rc
        self._point_calls("mrtx_view_hits", call, la, lo, width, chunk_bytes, stats, extra={"bounce_rays": "bounce_rays"})
        return hits, share

    def scatter_flux(self, index, exitance, albedo_h, emissivity, n_hits=None, m=None, out=None, stats=None):
        """The gather of DESIGN.md section 3.11: (N, m) float32 Q_sec[p, e] = (1/K) sum over index[p, j] >= 0, in j order, of
        (1 - albedo_h) M_vis + emissivity M_ir of that hit at epoch e.  `index`: (N, K) int32 into the hit list, -1 for sky;
        `exitance`: the (n_hits, m, 2) float32 EXITANCE of surface_temperature_scatter, or a DeviceBuffer holding it (then
        n_hits and m are required).  out = a DeviceBuffer of at least N * m * 4 bytes: Q_sec is written there, `out` returned."""
        ix = np.ascontiguousarray(index, np.int32)
        if ix.ndim != 2:
            raise ValueError("index must be an (N, K) array")
        n, k = ix.shape
        if isinstance(exitance, _device_buffer()):
            if n_hits is None or m is None:
                raise ValueError("n_hits and m are required with a device buffer")
            n_hits, m = int(n_hits), int(m)
            dev, host, length = exitance.ptr, None, exitance.nbytes // 4
        else:
            ex = np.ascontiguousarray(exitance, np.float32)
            if ex.ndim != 3 or ex.shape[2] != 2:
                raise ValueError("exitance must be an (n_hits, m, 2) array")
            n_hits, m = ex.shape[0], ex.shape[1]
            dev, host, length = None, ex.ctypes.data, ex.size
        if out is not None and out.nbytes < n * m * 4:
            raise ValueError("the device buffer is smaller than N x m float32")
        res = np.empty((n, m), np.float32) if out is None else None
        st = MrtxStats()
        self._check(self._lib.mrtx_scatter_flux(self._ctx, ix.ctypes.data, n, k, dev, host, length, n_hits, m, float(albedo_h),
                                                float(emissivity), None if out is None else out.ptr,
                                                None if res is None else res.ctypes.data, C.byref(st)), "mrtx_scatter_flux")
        self._add_stats(stats, st)
        return out if out is not None else res

    def surface_temperature_scatter(self, lat_deg, lon_deg, horizon, epochs, flux, model=None, mode="summary", extra_flux=None,
                                    stats=None, n_az=None, out=None):
        """surface_temperature with the additions of DESIGN.md section 3.11, in one call.  `extra_flux`: None, an (N, m)
        float32 array or a DeviceBuffer holding one, added to Q_abs in every epoch.  Modes as surface_temperature's, plus
        "exitance": (N, m - n_spin, 2) float32 (M_vis, M_ir) per recorded epoch.  out = a DeviceBuffer: the output is written
        there and `out` returned."""
        modes = {"full": 0, "summary": 1, "flux": 2, "exitance": 3}
        head, res, _keep = self._thermal_prologue(modes, mode, lat_deg, lon_deg, horizon, epochs, flux, model, n_az, extra_flux, out)
        st = MrtxStats()
        self._check(self._lib.mrtx_thermal_scatter(*head, None if out is None else out.ptr,
                                                   None if res is None else res.ctypes.data, C.byref(st)), "mrtx_thermal_scatter")
        self._add_stats(stats, st, {"newton_cap_hits": "reserved"})
        return out if out is not None else res

    def _thermal_prologue(self, modes, mode, lat_deg, lon_deg, horizon, epochs, flux, model, n_az, extra_flux, out):
        """What surface_temperature_scatter and thermal_column do before their one call: the mode among `modes`, the points,
        epochs, flux, model, horizons and extra_flux, the output's shape and the check of `out` against it.  Returns (head,
        res, keep): head = the arguments mrtx_thermal_scatter, mrtx_thermal_column and mrtx_thermal_occulted share, from the
        context to the length of extra_flux; res = the host output, None with `out`; keep = the arrays head points into,
        the epochs first."""
        if mode not in modes:
            raise ValueError(f"mode must be one of {sorted(modes)} (got {mode!r})")
        la, lo = self._points(lat_deg, lon_deg)
        ep = self._epochs(epochs)
        m = ep.shape[0]
        fl = np.ascontiguousarray(np.asarray(flux, np.float64).ravel())
        if fl.size != m:
            raise ValueError("flux must hold one value per epoch")
        model = self.thermal_grid() if model is None else model
        n_az, hz_at = self._horizon_arg(horizon, la.size, n_az)
        dh, hh = hz_at(0)
        dx = hx = xf = None
        x_len = 0
        if isinstance(extra_flux, _device_buffer()):
            dx, x_len = extra_flux.ptr, extra_flux.nbytes // 4
        elif extra_flux is not None:
            xf = np.ascontiguousarray(extra_flux, np.float32)
            hx, x_len = xf.ctypes.data, xf.size
        pts = np.ascontiguousarray(np.stack([la, lo], -1))
        rec, nn = max(m - int(model.n_spin), 1), max(int(model.n_nodes), 1)
        shape = {"full": (la.size, rec), "summary": (la.size, 4), "flux": (la.size, m), "exitance": (la.size, rec, 2),
                 "column": (la.size, rec, nn), "volatile": (la.size, nn, 2)}[mode]
        dtype = np.float64 if mode == "volatile" else np.float32
        if out is not None and out.nbytes < int(np.prod(shape)) * np.dtype(dtype).itemsize:
            raise ValueError("the device buffer is smaller than the output")
        res = np.empty(shape, dtype) if out is None else None
        head = (self._ctx, pts.ctypes.data, la.size, n_az, dh, hh, ep.ctypes.data, fl.ctypes.data, m, C.byref(model), modes[mode],
                dx, hx, x_len)
        return head, res, (ep, pts, fl, xf, hz_at)

    @staticmethod
    def thermal_depths(model=None):
        """The node depths z_i of a MrtxThermalModel in metres, (n_nodes,) float64: z_0 = 0 and z_{i+1} = z_i + dz[i] (the
        model of thermal_grid() unless given)."""
        model = TerrainCalls.thermal_grid() if model is None else model
        n = int(model.n_nodes)
        return np.concatenate([[0.0], np.cumsum(np.array(model.dz[:n - 1], np.float64))])

    def thermal_column(self, lat_deg, lon_deg, horizon, epochs, flux, model=None, mode="column", extra_flux=None, species=None,
                       stats=None, n_az=None, out=None, occultation=None):
        """surface_temperature_scatter with the subsurface modes of DESIGN.md section 3.16, in one call.  Its modes ("full",
        "summary", "flux", "exitance") give its bits; "column": (N, m - n_spin, n_nodes) float32, every node's temperature
        after each recorded epoch (node 0 is "full"); "volatile": (N, n_nodes, 2) float64 (E_mean, T_max) per node, the mean
        over the recorded epochs of the free sublimation rate of `species` (a volatiles.Species, an MrtxVolatile or its four
        coefficients; kg m^-2 s^-1) and the node's highest temperature.  thermal_depths(model) gives the nodes' depths.
        out = a DeviceBuffer: the output is written there and `out` returned.  occultation = (source_epochs, body_epochs) as
        for MoonRT.occultation, m rows each: every epoch's disc fraction, spin-up included, is multiplied by that call's g at
        the point (section 3.18); None is the call without it."""
        modes = {"full": 0, "summary": 1, "flux": 2, "exitance": 3, "column": 4, "volatile": 5}
        sp = None
        if mode in modes:               # a mode that is none of them is the prologue's to refuse, as the first thing
            if (mode == "volatile") != (species is not None):
                raise ValueError("species is required in mode 'volatile' and must be None otherwise")
            if species is not None:
                from . import volatiles
                sp = species if isinstance(species, _lib.MrtxVolatile) else volatiles.law(species)
        head, res, keep = self._thermal_prologue(modes, mode, lat_deg, lon_deg, horizon, epochs, flux, model, n_az, extra_flux, out)
        tail = (None if out is None else out.ptr, None if res is None else res.ctypes.data)
        spp = None if sp is None else C.byref(sp)
        st = MrtxStats()
        if occultation is not None:
            os_, ob_ = (self._epochs(e) for e in occultation)
            if os_.shape != keep[0].shape or ob_.shape != keep[0].shape:
                raise ValueError("the occultation tables must hold one row per epoch")
            self._check(self._lib.mrtx_thermal_occulted(*head, spp, os_.ctypes.data, ob_.ctypes.data, *tail, C.byref(st)),
                        "mrtx_thermal_occulted")
        else:
            self._check(self._lib.mrtx_thermal_column(*head, spp, *tail, C.byref(st)), "mrtx_thermal_column")
        self._add_stats(stats, st, {"newton_cap_hits": "reserved"})
        return out if out is not None else res

    # ---- Terrain line of sight
    @staticmethod
    def _observer(observer):
        o = np.asarray(observer, np.float64)
        if o.shape != (3,):
            raise ValueError("observer must be one (lat, lon, height_m) triple")
        return o

    def viewshed(self, observer, lat=(90.0, -90.0), lon=(-180.0, 180.0), shape=(180, 360), target_height_m=0.0, mast_max_m=0.0,
                 n_bis=0, radius_m=1737400.0, rows=None, stats=None, band_bytes=256 << 20):
        """(rows, w) float32 map over the nodes of illumination_map's grid: per node the extra mast height, metres, at which a
        target raised target_height_m there sees the observer (lat, lon, height_m): 0 where it does already, +inf where even
        mast_max_m does not (n_bis = 0: a plain viewshed, 0 or +inf); otherwise the bisection's n_bis probes narrow it to
        mast_max_m / 2^(n_bis - 1).  radius_m = the metres of D = 1 (1737400 * the DEM's radius_scale).  Bands of at most
        band_bytes go through one device buffer; `stats`, if a dict, receives the summed counters."""
        o = self._observer(observer)
        h, w = int(shape[0]), int(shape[1])
        r0, r1 = (0, h) if rows is None else (int(rows[0]), int(rows[1]))
        g = _lib.MrtxSightGrid(o[0], o[1], o[2], float(target_height_m), float(mast_max_m), float(radius_m), float(lat[0]),
                               float(lat[1]), float(lon[0]), float(lon[1]), h, w, r0, r1, int(n_bis), 0)
        return self._band_map("mrtx_sight_grid", g, np.empty((max(r1 - r0, 0), w), np.float32), 4, band_bytes, stats)

    def line_of_sight(self, lat_deg, lon_deg, observer, target_height_m=0.0, mast_max_m=0.0, n_bis=0, radius_m=1737400.0,
                      stats=None, chunk_bytes=256 << 20):
        """(N,) float32 extra mast heights, metres, of N targets (degrees) toward `observer`: one (lat, lon, height_m) triple
        shared by all, or an (N, 3) array, one per target.  As viewshed; a target on a grid node gives that node's value.
        Calls hold at most chunk_bytes of output each (targets split between calls)."""
        la, lo = self._points(lat_deg, lon_deg)
        obs = np.asarray(observer, np.float64)
        if obs.shape == (3,):
            obs = obs.reshape(1, 3)
        elif obs.shape != (la.size, 3):
            raise ValueError("observer must be one (lat, lon, height_m) triple or one per target, (N, 3)")
        obs = np.ascontiguousarray(obs)
        shared = obs.shape[0] == 1
        out = np.empty(la.size, np.float32)

        def call(pts, a, b, dh, hh, st):
            op, no = (obs.ctypes.data, 1) if shared else (obs[a:].ctypes.data, b - a)
            return self._lib.mrtx_sight_points(self._ctx, pts, b - a, op, no, float(target_height_m), float(mast_max_m),
                                               float(radius_m), int(n_bis), None, out[a:].ctypes.data, st)
        self._point_calls("mrtx_sight_points", call, la, lo, 1, chunk_bytes, stats, empty_call=False)
        return out

    # ---- Least-cost traverses
    def _dem_hw(self):
        hw = getattr(self, "_dem_shape", None)
        if hw is None:
            raise MoonRTError("no displacement map: call upload_dem or bind_dem first")
        return hw

    def traverse_nodes(self, window):
        """(lat, lon, grid) of a traverse window (row0, col0, rows, cols[, stride[, wrap]]) on the DEM in place: lat (rows,)
        and lon (cols,) float64 degrees of its nodes, the texel centres (lon in [-180, 180)), and grid = dict(lat=, lon=,
        shape=), the arguments with which illumination_map / viewshed sample the same positions node for node (their
        longitudes continue past 180 where the window does; with stride > 1 a window on the DEM's first or last row puts
        lat beyond +-90, which those calls refuse)."""
        from .traverse import window_dict
        w = window_dict(window)
        H, W = self._dem_hw()
        s = w["stride"]
        lat = 90.0 - (w["row0"] + np.arange(w["rows"]) * s + 0.5) * (180.0 / H)
        lon = -180.0 + ((w["col0"] + np.arange(w["cols"]) * s) % W + 0.5) * (360.0 / W)
        la_n = 90.0 - (w["row0"] + 0.5 - 0.5 * s) * (180.0 / H)
        lo_w = -180.0 + (w["col0"] + 0.5 - 0.5 * s) * (360.0 / W)
        grid = {"lat": (la_n, la_n - w["rows"] * s * (180.0 / H)), "lon": (lo_w, lo_w + w["cols"] * s * (360.0 / W)),
                "shape": (w["rows"], w["cols"])}
        return lat, lon, grid

    def snap_to_nodes(self, window, lat_deg, lon_deg):
        """(N, 2) int32 (i, j) of the window nodes nearest to N points: the row whose centre latitude is nearest, the column
        whose centre longitude is nearest around the circle (halves round up to the larger index); ValueError if one lies
        outside the window."""
        from .traverse import window_dict
        w = window_dict(window)
        H, W = self._dem_hw()
        s = w["stride"]
        la = np.atleast_1d(np.asarray(lat_deg, np.float64))
        lo = np.atleast_1d(np.asarray(lon_deg, np.float64))
        i = np.floor(((90.0 - la) * (H / 180.0) - 0.5 - w["row0"]) / s + 0.5).astype(np.int64)
        cc = ((lo + 180.0) * (W / 360.0) - 0.5 - w["col0"]) % W           # texel columns east of col0
        j = np.floor(cc / s + 0.5).astype(np.int64)
        if w["wrap"]:
            j %= w["cols"]
        else:       # nearer to the window's first column going round the circle the other way
            j = np.where(j >= w["cols"], np.where((W - cc) / s <= 0.5, 0, j), j)
        bad = (i < 0) | (i >= w["rows"]) | (j < 0) | (j >= w["cols"])
        if bad.any():
            k = int(np.argmax(bad))
            raise ValueError(f"point ({la[k]}, {lo[k]}) lies outside the window")
        return np.ascontiguousarray(np.stack([i, j], -1).astype(np.int32))

    # what traverse and traverse_timed share: the sources as nodes, the edge lengths, the penalty argument, the stats
    def _traverse_sources(self, w, sources, nodes):
        """(N, 2) int32 (i, j) from exactly one of `sources` ((lat, lon) degrees, snapped) and `nodes`."""
        if (sources is None) == (nodes is None):
            raise ValueError("give exactly one of sources ((lat, lon) degrees) and nodes ((i, j) indices)")
        if nodes is not None:
            ij = np.asarray(nodes)
            if not np.issubdtype(ij.dtype, np.integer):
                raise ValueError("nodes must be integer (i, j) indices")
            ij = np.ascontiguousarray(ij.reshape(-1, 2) if ij.ndim == 1 else ij, np.int32)
        else:
            ll = np.asarray(sources, np.float64)
            ll = ll.reshape(1, -1) if ll.ndim == 1 else ll
            if ll.ndim != 2 or ll.shape[1] != 2:
                raise ValueError("sources must be (N, 2) (lat, lon) degrees")
            ij = self.snap_to_nodes(w, ll[:, 0], ll[:, 1])
        if ij.ndim != 2 or ij.shape[1] != 2:
            raise ValueError("nodes must be (N, 2) (i, j) indices")
        return ij

    def _traverse_lengths(self, t, H, W):
        lengths = np.empty((max(t.rows, 1), 3), np.float32)
        rc = self._lib.mrtx_traverse_lengths(C.byref(t), H, W, lengths.ctypes.data)
        if rc != 0:
            raise MoonRTError(f"mrtx_traverse_lengths failed ({rc}): bad window or lengths")
        return lengths

    @staticmethod
    def _traverse_penalty(w, penalty):
        """(dev_penalty, host_penalty, the host map or None) of a penalty argument; the map must outlive the call."""
        dev_pen = host_pen = pen = None
        if isinstance(penalty, _device_buffer()):
            if penalty.nbytes < 4 * w["rows"] * w["cols"]:
                raise ValueError("the penalty buffer is smaller than rows x cols float32")
            dev_pen = penalty.ptr
        elif penalty is not None:
            pen = np.ascontiguousarray(penalty, np.float32)
            if pen.shape != (w["rows"], w["cols"]):
                raise ValueError(f"penalty must be a (rows, cols) = {(w['rows'], w['cols'])} map")
            host_pen = pen.ctypes.data
        return dev_pen, host_pen, pen

    @staticmethod
    def _traverse_stats(stats, st, visits):
        if isinstance(stats, dict):
            stats["kernel_ms"] = stats.get("kernel_ms", 0) + st.kernel_ms
            stats["launches"] = stats.get("launches", 0) + st.launches
            stats["tile_visits"] = stats.get("tile_visits", 0) + int(visits.value)

    def traverse(self, window, sources=None, penalty=None, max_slope_deg=20.0, climb_cost=8.0, descent_cost=0.0,
                 radius_m=1737400.0, start_cost=None, stats=None, nodes=None, heights=True):
        """The least-cost field over a window (row0, col0, rows, cols[, stride[, wrap]]) of the DEM's texel lattice
        (mrtx_traverse) from its sources: `sources` = an (N, 2) array of (lat, lon) degrees, each
        snapped to its nearest node (snap_to_nodes), or `nodes` = an (N, 2) array of explicit (i, j) nodes -- exactly one of
        the two; start_cost = N start costs (default 0).  penalty: None, a (rows, cols) float32 map or a DeviceBuffer
        holding one (see moonrtx_amd.traverse for builders).  The effort of a step is its length plus climb_cost per metre
        climbed and descent_cost per metre descended (the defaults: Naismith's rule, 8 m of walking per metre of ascent);
        steps steeper than max_slope_deg are not driven.  radius_m = the metres of D = 1.  Returns a
        moonrtx_amd.traverse.TraverseField; with `heights` it holds the window's node heights (mrtx_traverse_heights), so that
        routes read their heights from the field and not from the context, which may be closed or hold another DEM by then.
        `stats`, if a dict, receives kernel_ms, launches and tile_visits of the traverse."""
        from . import traverse as tv
        w = tv.window_dict(window)
        H, W = self._dem_hw()
        ij = self._traverse_sources(w, sources, nodes)
        cost0 = None if start_cost is None else np.ascontiguousarray(np.broadcast_to(np.asarray(start_cost, np.float64),
                                                                                      (ij.shape[0],)))
        t = self._traverse_window(w, radius_m, tv.max_slope_grade(max_slope_deg), climb_cost, descent_cost)
        lengths = self._traverse_lengths(t, H, W)
        dev_pen, host_pen, pen = self._traverse_penalty(w, penalty)
        cost = np.empty((w["rows"], w["cols"]), np.float64)
        pred = np.empty((w["rows"], w["cols"]), np.uint8)
        visits = C.c_uint64()
        st = MrtxStats()
        self._check(self._lib.mrtx_traverse(self._ctx, C.byref(t), ij.ctypes.data, None if cost0 is None else cost0.ctypes.data,
                                            ij.shape[0], dev_pen, host_pen, None, cost.ctypes.data, None, pred.ctypes.data,
                                            C.byref(visits), C.byref(st)), "mrtx_traverse")
        self._traverse_stats(stats, st, visits)
        lat, lon, _ = self.traverse_nodes(w)
        D = self.traverse_heights(w) if heights else None
        return tv.TraverseField(cost, pred, w, lengths, radius_m, lat, lon, D=D)

    def traverse_timed(self, window, sources=None, nodes=None, start_tick=None, avail=None, n_epochs=None, ticks_per_epoch=3600,
                       ticks_per_cost=5.0, penalty=None, max_slope_deg=20.0, climb_cost=8.0, descent_cost=0.0,
                       radius_m=1737400.0, stats=None):
        """The earliest-arrival field over a traverse window (mrtx_traverse_timed): time in integer
        ticks, an edge of `traverse`'s weight w lasting ceil(w * ticks_per_cost) ticks (at least 1), epoch e covering the
        ticks [e, e + 1) * ticks_per_epoch, and an edge driven only while every epoch it touches is available at both of
        its ends; waiting at a node is free.  window, sources / nodes, penalty and the effort model as for `traverse`;
        start_tick = the sources' start ticks (default 0).  avail: None (always drivable), an (rows, cols, W64) or
        (rows * cols, W64) uint64 array in horizon_mask's layout, or a DeviceBuffer holding one (moonrtx_amd.traverse.
        drive_mask); n_epochs = the epochs it covers (default W64 * 64 for an array, required for a buffer).  Returns a
        moonrtx_amd.traverse.TimedField; `stats`, if a dict, receives kernel_ms, launches and tile_visits."""
        from . import traverse as tv
        w = tv.window_dict(window)
        H, W = self._dem_hw()
        ij = self._traverse_sources(w, sources, nodes)
        tick0 = None if start_tick is None else np.ascontiguousarray(np.broadcast_to(np.asarray(start_tick, np.uint64),
                                                                                      (ij.shape[0],)))
        max_grade = tv.max_slope_grade(max_slope_deg)
        t = self._traverse_window(w, radius_m, max_grade, climb_cost, descent_cost)
        lengths = self._traverse_lengths(t, H, W)
        N = w["rows"] * w["cols"]
        dev_pen, host_pen, pen = self._traverse_penalty(w, penalty)
        dev_av = host_av = av = None
        if isinstance(avail, _device_buffer()):
            if n_epochs is None:
                raise ValueError("n_epochs is required with a device buffer")
            if avail.nbytes < 8 * N * tv.mask_words(n_epochs):
                raise ValueError("the availability buffer is smaller than rows x cols x W64 uint64")
            dev_av = avail.ptr
        elif avail is not None:
            av = np.ascontiguousarray(avail, np.uint64)
            if av.ndim not in (2, 3) or av.size % max(N, 1) or av.shape[:-1] not in ((N,), (w["rows"], w["cols"])):
                raise ValueError("avail must be a (rows, cols, W64) or (rows * cols, W64) uint64 array")
            n_epochs = av.shape[-1] * 64 if n_epochs is None else int(n_epochs)
            if av.shape[-1] != tv.mask_words(n_epochs):
                raise ValueError(f"{n_epochs} epochs take {tv.mask_words(n_epochs)} words per node (got {av.shape[-1]})")
            av = av.reshape(w["rows"], w["cols"], -1)
            host_av = av.ctypes.data
        tt = _lib.MrtxTraverseTimed(float(ticks_per_cost), int(ticks_per_epoch), 0 if avail is None else int(n_epochs), 0)
        arrival = np.empty((w["rows"], w["cols"]), np.uint64)
        pred = np.empty((w["rows"], w["cols"]), np.uint8)
        visits = C.c_uint64()
        st = MrtxStats()
        self._check(self._lib.mrtx_traverse_timed(self._ctx, C.byref(t), C.byref(tt), ij.ctypes.data,
                                                  None if tick0 is None else tick0.ctypes.data, ij.shape[0], dev_pen, host_pen,
                                                  dev_av, host_av, None, arrival.ctypes.data, None, pred.ctypes.data,
                                                  C.byref(visits), C.byref(st)), "mrtx_traverse_timed")
        self._traverse_stats(stats, st, visits)
        lat, lon, _ = self.traverse_nodes(w)
        if dev_pen is not None:
            pen = penalty.download(np.float32, (w["rows"], w["cols"]))
        return tv.TimedField(arrival, pred, w, lengths, radius_m, lat, lon, D=self.traverse_heights(w),
                             ticks_per_cost=ticks_per_cost, ticks_per_epoch=ticks_per_epoch,
                             n_epochs=None if avail is None else n_epochs, max_grade=max_grade, climb_cost=climb_cost,
                             descent_cost=descent_cost, penalty=pen, avail=av)

    @staticmethod
    def _traverse_window(w, radius_m=1737400.0, max_grade=1.0, climb_cost=0.0, descent_cost=0.0):
        return _lib.MrtxTraverse(w["row0"], w["col0"], w["rows"], w["cols"], w["stride"], w["wrap"], float(radius_m),
                                 float(max_grade), float(climb_cost), float(descent_cost), 0)

    def traverse_heights(self, window, stats=None):
        """(rows, cols) float32 D of a traverse window's nodes, copied from the context's DEM (mrtx_traverse_heights):
        (D - 1) x radius_m is a node's height above the sphere in metres."""
        from .traverse import window_dict
        w = window_dict(window)
        D = np.empty((w["rows"], w["cols"]), np.float32)
        st = MrtxStats()
        self._check(self._lib.mrtx_traverse_heights(self._ctx, C.byref(self._traverse_window(w)), None, D.ctypes.data,
                                                    C.byref(st)), "mrtx_traverse_heights")
        self._add_stats(stats, st)
        return D

    # ---- Terrain relief: slope, roughness, landing hazard
    def relief(self, window, footprint_m=None, footprint_nodes=None, radius_m=1737400.0, stats=None):
        """Slope and roughness under a footprint, per node of a window (row0, col0, rows, cols[, stride]) of the DEM's texel
        lattice (mrtx_relief).  Exactly one of footprint_nodes = (ri, rj), the footprint's half-heights
        in lattice nodes (1 .. 32), and footprint_m, its width in metres: then ri follows from the N-S spacing of the rows, and
        the window is split into row bands over which rj = max(1, round(footprint_m / 2 / L_ew)) is constant, one call per
        band (a footprint reads the DEM, not the window, so the bands join exactly).  radius_m = the metres of D = 1.
        Returns a moonrtx_amd.relief.ReliefMap; `stats`, if a dict, receives the summed counters."""
        from . import relief as rl
        w = rl.window_dict(window)
        if w["wrap"]:
            raise ValueError("a relief window is never wrapped: its footprints read across the seam by themselves")
        H, W = self._dem_hw()
        if (footprint_m is None) == (footprint_nodes is None):
            raise ValueError("give exactly one of footprint_m and footprint_nodes = (ri, rj)")
        if footprint_nodes is not None:
            ri, rj = (int(v) for v in footprint_nodes)
            bands = [(0, w["rows"], rj)]
        else:
            ri, bands = rl.footprint_bands(self._lib, w, footprint_m, radius_m, (H, W))
        table = np.empty((w["rows"], w["cols"], 4), np.float32)
        for a, n, rj in bands:
            st = MrtxStats()
            t = rl.relief_window(w, ri, rj, radius_m, rows=(a, n))
            self._check(self._lib.mrtx_relief(self._ctx, C.byref(t), None, table[a:].ctypes.data, C.byref(st)), "mrtx_relief")
            self._add_stats(stats, st)
        lat, lon, _ = self.traverse_nodes(w)
        return rl.ReliefMap(table, w, radius_m, ri, bands, w["cols"] * w["stride"] == W, lat, lon)

    def landing_share(self, relief, max_slope_deg, max_rms_m, ellipse_m=None, ellipse_nodes=None, stats=None):
        """The safe share of a landing ellipse around every node of a ReliefMap (mrtx_relief_share): (rows, cols) float32,
        the fraction of the map's nodes in the (2 Ri + 1) x (2 Rj + 1) box around the node with slope <= max_slope_deg and
        roughness <= max_rms_m (NaN nodes are unsafe; nodes outside the map do not count, and the columns join across +-180
        when the map goes round the circle).  Exactly one of ellipse_nodes = (Ri, Rj), 0 .. 1024, and ellipse_m, the box's
        width in metres, turned into nodes with the map's N-S spacing and the E-W spacing of its middle row."""
        from . import relief as rl
        from .traverse import max_slope_grade
        w = relief.window
        if (ellipse_m is None) == (ellipse_nodes is None):
            raise ValueError("give exactly one of ellipse_m and ellipse_nodes = (Ri, Rj)")
        if ellipse_nodes is not None:
            Ri, Rj = (int(v) for v in ellipse_nodes)
        else:
            k = rl.scales(self._lib, rl.relief_window(w, radius_m=relief.radius_m), self._dem_hw())
            half = 0.5 * float(ellipse_m) / relief.radius_m
            Ri, Rj = int(math.floor(half * k[0, 1] + 0.5)), int(math.floor(half * k[w["rows"] // 2, 0] + 0.5))
        s = _lib.MrtxReliefShare(w["rows"], w["cols"], Ri, Rj, 1 if relief.closes_circle and w["cols"] >= 3 else 0, 0,
                                 max_slope_grade(max_slope_deg), float(max_rms_m))
        table = np.ascontiguousarray(relief.table, np.float32)
        out = np.empty((w["rows"], w["cols"]), np.float32)
        st = MrtxStats()
        self._check(self._lib.mrtx_relief_share(self._ctx, C.byref(s), None, table.ctypes.data, None, out.ctypes.data,
                                                C.byref(st)), "mrtx_relief_share")
        self._add_stats(stats, st)
        return out

    @staticmethod
    def _chunks(n, per, chunk_bytes, out_bytes=4, empty_call=True):
        """The [a, b) point ranges of a point query's calls: each holds at most chunk_bytes and 2^31 outputs, `per` outputs of
        out_bytes per point (per = None: one call for all).  With N = 0 the query makes one call with no points when
        empty_call, which the library refuses (horizon, horizon_sun, surface_temperature, view_hits: an empty query is an
        error), and no call otherwise (illumination_series, line_of_sight: an empty result)."""
        step = max(n, 1) if per is None else max(1, min(int(chunk_bytes) // (out_bytes * per), (1 << 31) // per))
        return [(a, min(a + step, n)) for a in range(0, max(n, 1) if empty_call else n, step)]

    def _point_calls(self, name, call, la, lo, per, chunk_bytes, stats, hz_at=None, extra=None, **chunking):
        """The library calls of a chunked point query, one per range [a, b) of _chunks: call(pts, a, b, dh, hh, st)
        makes the call for the points from a on -- pts = the address of their (lat, lon) pairs, (dh, hh) = hz_at(a), the
        horizons from point a on where the query reads horizons, st = a fresh MrtxStats by reference -- and returns its code;
        the counters of each call, and its own `extra` (_add_stats), are summed into `stats`."""
        pts = np.ascontiguousarray(np.stack([la, lo], -1))
        for a, b in self._chunks(la.size, per, chunk_bytes, **chunking):
            st = MrtxStats()
            dh, hh = hz_at(a) if hz_at is not None else (None, None)
            self._check(call(pts[a:].ctypes.data, a, b, dh, hh, C.byref(st)), name)
            self._add_stats(stats, st, extra)

    @staticmethod
    def _horizon_arg(horizon, n, n_az):
        """(n_az, at) of a `horizon` argument -- the (N, n_az) float32 array of MoonRT.horizon, or a DeviceBuffer holding it
        (then n_az is required) -- with at(a) = the (device, host) pointers of the horizons from point a on."""
        if isinstance(horizon, _device_buffer()):
            if n_az is None:
                raise ValueError("n_az is required with a device buffer")
            n_az = int(n_az)
            if horizon.nbytes < n * n_az * 4:
                raise ValueError("the device buffer is smaller than N x n_az float32")
            return n_az, lambda a: (horizon.ptr + a * n_az * 4, None)
        hz = np.ascontiguousarray(horizon, np.float32)
        if hz.ndim != 2 or hz.shape[0] != n:
            raise ValueError("horizon must be an (N, n_az) array")
        return hz.shape[1], lambda a: (None, hz[a:].ctypes.data)
