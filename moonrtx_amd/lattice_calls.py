"""The lattice half of MoonRT: regions, zonal statistics, shapes, proximity, outlines, polygon rasterisation, contours,
depressions and bowls of per-node tables -- the Python side of csrc/mrtx_lattice_api.hip.  MoonRT (renderer.py) inherits these methods.

Every library call here takes its tables as (device, host) pointer pairs, one of each pair null.  A method is written once:
its inputs come as pairs from _label_arg / _int32_arg / _lattice_arg / _outlet_arg, its outputs are _Tables made on the side
the inputs are on, and `take` turns an output into the array the method returns."""
import ctypes as C
import math

import numpy as np

from . import _lib
from ._calls import Calls, DeviceBuffer, MoonRTError
from ._lib import MrtxStats

_NULL = (None, None)


class _Table:
    """An output table of `shape` records of `dtype`: a numpy array (device = None) or a DeviceBuffer on `device`.  A zeroed
    host table holds at least one record, a device table at least `floor` bytes (default: one item), so that neither is
    ever an empty allocation."""

    def __init__(self, device, dtype, shape, zeros=False, floor=None):
        self.dtype, self.host, self.buf = np.dtype(dtype), None, None
        if device is None:
            self.host = np.zeros((max(shape[0], 1),) + tuple(shape[1:]), dtype) if zeros else np.empty(shape, dtype)
        else:
            nbytes = self.dtype.itemsize * math.prod(shape)
            self.buf = DeviceBuffer(max(nbytes, self.dtype.itemsize if floor is None else floor), device)

    @property
    def pair(self):
        """The table as the (device, host) pointer pair of a library call."""
        return (self.buf.ptr, None) if self.buf is not None else (None, self.host.ctypes.data)

    def take(self, shape):
        """The first shape[0] records as an array: a slice of the host table, a download of the device table."""
        return self.buf.download(self.dtype, shape) if self.buf is not None else self.host[:shape[0]]


class _Tables:
    """The output tables of one method, all on one side (device = None: the host); leaving the block frees every device
    table, whether the method returns or a call was refused."""

    def __init__(self, device):
        self.device, self.made = device, []

    def new(self, dtype, shape, **kw):
        self.made.append(_Table(self.device, dtype, shape, **kw))
        return self.made[-1]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for t in self.made:
            if t.buf is not None:
                t.buf.free()


class LatticeCalls(Calls):
    # ---- Connected regions of a per-node map
    def regions(self, field=None, mask=None, channel=0, lo=-math.inf, hi=math.inf, connectivity=4, wrap=False,
                row_weights=None, stats=None, shape=None, unit_m2=None):
        """The connected regions of a set of lattice nodes (mrtx_regions_label, mrtx_regions_stats).  Exactly one of `field`,
        (rows, cols) or (rows, cols, n_ch) float32: the nodes with lo <= field[..., channel] <= hi, compared as float32 (NaN
        is out), and `mask`, (rows, cols) uint8: the nonzero nodes.  Either may be a numpy array or a DeviceBuffer (then give
        shape = (rows, cols[, n_ch]); labels and catalogue are made in device tables and downloaded).  connectivity 4 or 8;
        wrap joins the last column to the first (cols >= 3).  row_weights: (rows,) uint32 node areas (regions.row_weights),
        or None: every node weighs 1; unit_m2: their unit, remembered by the map.  Needs no DEM.  Returns a
        moonrtx_amd.regions.RegionMap; `stats`, if a dict, receives the summed counters and label_ms / catalogue_ms."""
        from . import regions as rg
        if (field is None) == (mask is None):
            raise ValueError("give exactly one of field and mask")
        src = field if field is not None else mask
        on_device = isinstance(src, DeviceBuffer)
        if on_device:
            if shape is None:
                raise ValueError("a DeviceBuffer needs shape = (rows, cols[, n_ch])")
            shp = tuple(int(v) for v in shape)
        else:
            src = np.ascontiguousarray(src, np.float32 if field is not None else np.uint8)
            shp = src.shape
        if field is not None and len(shp) == 2:
            shp = shp + (1,)
        if len(shp) != (3 if field is not None else 2):
            raise ValueError("field must be (rows, cols) or (rows, cols, n_ch), mask (rows, cols)")
        rows, cols = shp[0], shp[1]
        n_ch = shp[2] if field is not None else 1
        if on_device and src.nbytes < rows * cols * (4 * n_ch if field is not None else 1):
            raise ValueError("the DeviceBuffer is smaller than its shape")
        weights = None
        if row_weights is not None:
            weights = np.ascontiguousarray(row_weights)
            if weights.shape != (rows,) or not np.issubdtype(weights.dtype, np.integer) or \
                    (weights.size and (weights.min() < 0 or weights.max() > rg.WEIGHT_MAX)):
                raise ValueError("row_weights must be (rows,) integers in 0 .. 2^32 - 1")
            weights = weights.astype(np.uint32)
        r = _lib.MrtxRegions(rows, cols, 1 if wrap else 0, int(connectivity), n_ch, int(channel), float(lo), float(hi), 0)
        n = C.c_uint32(0)
        st, st2 = MrtxStats(), MrtxStats()
        wp = weights.ctypes.data if weights is not None else None
        src_pair = (src.ptr, None) if on_device else (None, src.ctypes.data)
        args = src_pair + _NULL if field is not None else _NULL + src_pair
        with _Tables(src.device if on_device else None) as t:
            lab = t.new(np.int32, (rows, cols))
            self._check(self._lib.mrtx_regions_label(self._ctx, C.byref(r), *args, *lab.pair, C.byref(n), C.byref(st)),
                        "mrtx_regions_label")
            rec = t.new(rg.REGION_DTYPE, (n.value,), zeros=True)
            self._check(self._lib.mrtx_regions_stats(self._ctx, rows, cols, r.wrap, *lab.pair, n.value, wp, *rec.pair,
                                                     C.byref(st2)), "mrtx_regions_stats")
            labels = lab.take((rows, cols))
            table = rec.take((n.value,))
        self._add_stats(stats, st)
        self._add_stats(stats, st2)
        if isinstance(stats, dict):
            stats["label_ms"] = stats.get("label_ms", 0.0) + st.kernel_ms
            stats["catalogue_ms"] = stats.get("catalogue_ms", 0.0) + st2.kernel_ms
            stats["label_launches"] = stats.get("label_launches", 0) + st.launches
        return rg.RegionMap(labels, table, wrap, unit_m2)

    # ---- the arguments the lattice calls share
    @staticmethod
    def _label_arg(labels, shape):
        """(device pointer, host pointer, rows, cols, keepalive) of a label table: (rows, cols) int32 or a DeviceBuffer."""
        if isinstance(labels, DeviceBuffer):
            if shape is None:
                raise ValueError("a DeviceBuffer needs shape = (rows, cols)")
            rows, cols = int(shape[0]), int(shape[1])
            if labels.nbytes < 4 * rows * cols:
                raise ValueError("the label DeviceBuffer is smaller than its shape")
            return labels.ptr, None, rows, cols, labels
        a = np.ascontiguousarray(labels, np.int32)
        if a.ndim != 2:
            raise ValueError("labels must be (rows, cols)")
        return None, a.ctypes.data, int(a.shape[0]), int(a.shape[1]), a

    @staticmethod
    def _row_table(table, n, what):
        """(pointer, keepalive) of an optional (n,) table of uint32 weights or side lengths; (None, None) without one."""
        if table is None:
            return None, None
        t = np.ascontiguousarray(table)
        if t.shape != (n,) or not np.issubdtype(t.dtype, np.integer) or (t.size and (t.min() < 0 or t.max() > 2 ** 32 - 1)):
            raise ValueError(f"{what} must be ({n},) integers in 0 .. 2^32 - 1")
        t = t.astype(np.uint32)
        return t.ctypes.data, t

    @staticmethod
    def _int32_arg(table, shape, what):
        """(device pointer, host pointer, keepalive) of a (rows, cols) int32 table: a numpy array or a DeviceBuffer."""
        if isinstance(table, DeviceBuffer):
            if table.nbytes < 4 * shape[0] * shape[1]:
                raise ValueError(f"the {what} DeviceBuffer is smaller than its shape")
            return table.ptr, None, table
        a = np.ascontiguousarray(table)
        if a.shape != tuple(shape) or not np.issubdtype(a.dtype, np.integer):
            raise ValueError(f"{what} must be ({shape[0]}, {shape[1]}) integers")
        if a.size and (a.min() < -2 ** 31 or a.max() > 2 ** 31 - 1):
            raise ValueError(f"{what} leaves int32")
        a = a.astype(np.int32)
        return None, a.ctypes.data, a

    @classmethod
    def _lattice_arg(cls, table, shape, what):
        """(device pointer, host pointer, keepalive, rows, cols) of the lattice a method works on: a (rows, cols) int32 table,
        whose shape is the lattice's, or a DeviceBuffer with shape = (rows, cols)."""
        if isinstance(table, DeviceBuffer):
            if shape is None:
                raise ValueError("a DeviceBuffer needs shape = (rows, cols)")
            rows, cols = int(shape[0]), int(shape[1])
        else:
            h = np.asarray(table)
            if h.ndim != 2:
                raise ValueError(f"{what} must be (rows, cols)")
            rows, cols = int(h.shape[0]), int(h.shape[1])
        return cls._int32_arg(table, (rows, cols), what) + (rows, cols)

    @staticmethod
    def _outlet_arg(outlets, rows, cols):
        """(device pointer, host pointer, keepalive) of an `outlets` argument: None, a (rows, cols) table whose nonzero nodes
        are outlets, or a DeviceBuffer of rows x cols uint8.  It goes to the library as it is, whichever side the heights
        are on."""
        if isinstance(outlets, DeviceBuffer):
            if outlets.nbytes < rows * cols:
                raise ValueError("the outlet DeviceBuffer is smaller than its shape")
            return outlets.ptr, None, outlets
        if outlets is None:
            return None, None, None
        o = np.ascontiguousarray(np.asarray(outlets) != 0, np.uint8)
        if o.shape != (rows, cols):
            raise ValueError("outlets and heights differ in shape")
        return None, o.ctypes.data, o

    def _count_then_fill(self, name, call, counters, n_tables, make, stats, fill_ms=True):
        """The two calls of a method whose output sizes the library alone knows.  call(tables, capacities, st) makes one
        library call with the (device, host) pairs and the capacities of its count-sized tables and returns its code.  The
        first call has no tables and capacities 0 and leaves the counts in `counters`; make(*counts) then makes the tables
        (None: a table left out) for exactly those counts, and the second call fills them.  Returns (counts, tables)."""
        st, st2 = MrtxStats(), MrtxStats()
        self._check(call([_NULL] * n_tables, [0] * len(counters), st), name)
        self._add_stats(stats, st)
        counts = [int(c.value) for c in counters]
        tables = make(*counts)
        self._check(call([t.pair if t is not None else _NULL for t in tables], counts, st2), name)
        self._add_stats(stats, st2)
        if isinstance(stats, dict):
            stats["count_ms"] = stats.get("count_ms", 0.0) + st.kernel_ms
            if fill_ms:
                stats["fill_ms"] = stats.get("fill_ms", 0.0) + st2.kernel_ms
        return counts, tables

    # ---- Zonal statistics and outlines of labelled regions
    def region_statistics(self, labels, n_regions, field, row_weights=None, scale=1.0, hist=None, wrap=False, shape=None,
                          stats=None):
        """What is inside each region of a label table (mrtx_regions_zonal): count, NaN count, exact fixed-point sums (q =
        llrint(x * scale)), area-weighted sums, and the extremes with their places, per region and channel.  labels: (rows,
        cols) int32 or a DeviceBuffer (then give shape = (rows, cols)); field: (rows, cols) or (rows, cols, n_ch) float32 or a
        DeviceBuffer (then shape = (rows, cols, n_ch)); both from one side: with a DeviceBuffer among them the records are
        made in device tables and downloaded.  row_weights: (rows,) uint32 node areas or None.  hist = (channel, n_bins, lo,
        hi): also the weight of every region per value band.  Returns a (n_regions, n_ch) array of regions.ZONAL_DTYPE, and
        with hist the pair (records, (n_regions, n_bins + 2) uint64).  Raises MoonRTError when a weighted sum may have
        wrapped (regions.check_wsum): lower scale then."""
        from . import regions as rg
        n_regions = int(n_regions)
        dev_f = isinstance(field, DeviceBuffer)
        dev_l = isinstance(labels, DeviceBuffer)
        if dev_f != dev_l:
            raise ValueError("labels and field must both be numpy arrays or both DeviceBuffers")
        if dev_f:
            if shape is None or len(shape) != 3:
                raise ValueError("DeviceBuffers need shape = (rows, cols, n_ch)")
            n_ch = int(shape[2])
        else:
            field = np.ascontiguousarray(field, np.float32)
            if field.ndim == 2:
                field = field[:, :, None]
            if field.ndim != 3:
                raise ValueError("field must be (rows, cols) or (rows, cols, n_ch)")
            n_ch = int(field.shape[2])
        lab_d, lab_h, rows, cols, _keep = self._label_arg(labels, shape)
        if dev_f:
            if field.nbytes < 4 * rows * cols * n_ch:
                raise ValueError("the field DeviceBuffer is smaller than its shape")
        elif field.shape[:2] != (rows, cols):
            raise ValueError("field and labels differ in shape")
        wp, _kw = self._row_table(row_weights, rows, "row_weights")
        hist_ch, n_bins, lo, inv_w = 0, 0, 0.0, 1.0
        if hist is not None:
            hist_ch, n_bins, lo, hi = int(hist[0]), int(hist[1]), float(hist[2]), float(hist[3])
            if n_bins < 1 or not hi > lo:
                raise ValueError("hist = (channel, n_bins >= 1, lo, hi > lo)")
            inv_w = n_bins / (hi - lo)
        z = _lib.MrtxZonalSpec(rows, cols, 1 if wrap else 0, n_ch, float(scale), hist_ch, n_bins, lo, inv_w, 0)
        st = MrtxStats()
        width = n_bins + 2
        f_pair = (field.ptr, None) if dev_f else (None, field.ctypes.data)
        with _Tables(field.device if dev_f else None) as t:
            rec = t.new(rg.ZONAL_DTYPE, (n_regions, n_ch), zeros=True)
            hb = t.new(np.uint64, (n_regions, width), zeros=True) if n_bins else None
            self._check(self._lib.mrtx_regions_zonal(self._ctx, C.byref(z), lab_d, lab_h, n_regions, *f_pair, wp, *rec.pair,
                                                     *(hb.pair if hb else _NULL), C.byref(st)), "mrtx_regions_zonal")
            table = rec.take((n_regions, n_ch))
            h = hb.take((n_regions, width)) if hb else None
        self._add_stats(stats, st)
        try:
            rg.check_wsum(table, float(scale))
        except OverflowError as e:
            raise MoonRTError(str(e)) from e
        return (table, h) if n_bins else table

    def region_shapes(self, labels, n_regions, connectivity=4, wrap=False, side_ew=None, side_ns=None, shape=None, stats=None):
        """The outline of each region of a label table (mrtx_regions_shape): perimeter, boundary-side counts, the bit-quad
        counts and the Euler number (components minus holes in the given connectivity).  labels: (rows, cols) int32 or a
        DeviceBuffer (then give shape = (rows, cols)).  side_ew (rows,) and side_ns (rows + 1,) uint32 side lengths
        (regions.side_weights), both or neither: with neither every side counts 1.  Returns (n_regions,) regions.SHAPE_DTYPE."""
        from . import regions as rg
        n_regions = int(n_regions)
        lab_d, lab_h, rows, cols, _keep = self._label_arg(labels, shape)
        if (side_ew is None) != (side_ns is None):
            raise ValueError("give both of side_ew and side_ns or neither")
        ewp, _ke = self._row_table(side_ew, rows, "side_ew")
        nsp, _kn = self._row_table(side_ns, rows + 1, "side_ns")
        st = MrtxStats()
        with _Tables(labels.device if lab_d is not None else None) as t:
            rec = t.new(rg.SHAPE_DTYPE, (n_regions,), zeros=True)
            self._check(self._lib.mrtx_regions_shape(self._ctx, rows, cols, 1 if wrap else 0, int(connectivity), lab_d, lab_h,
                                                     n_regions, ewp, nsp, *rec.pair, C.byref(st)), "mrtx_regions_shape")
            table = rec.take((n_regions,))
        self._add_stats(stats, st)
        return table

    # ---- Proximity maps and the reach of labelled regions
    def proximity(self, labels, positions, to="set", shape=None, stats=None, unit_m=None):
        """Every node's nearest feature node and the exact squared distance to it (mrtx_proximity), between node positions in
        three dimensions: to="set" measures to the nodes with label >= 0, to="outside" to those with label < 0; ties go to
        the least node index.  labels: (rows, cols) int32 or a DeviceBuffer; positions: (rows, cols, 3) int32
        (regions.node_positions), every coordinate within +-2^29, or a DeviceBuffer; both from one side, and with
        DeviceBuffers give shape = (rows, cols): the tables are then made on the device and downloaded.  unit_m: the metres
        of one unit of the positions, for the map's distances in metres.  Returns regions.ProximityMap.  stats gains
        launches, kernel_ms and pairs, the number of distance evaluations."""
        from . import regions as rg
        modes = {"set": _lib.PROX_TO_SET, "outside": _lib.PROX_TO_OUTSIDE}
        if to not in modes:
            raise ValueError('to must be "set" or "outside"')
        dev = isinstance(positions, DeviceBuffer)
        if dev != isinstance(labels, DeviceBuffer):
            raise ValueError("labels and positions must both be numpy arrays or both DeviceBuffers")
        lab_d, lab_h, rows, cols, _keep = self._label_arg(labels, shape)
        p = _lib.MrtxProximity(rows, cols, modes[to], 0)
        st = MrtxStats()
        pairs = C.c_uint64(0)
        if dev:
            if positions.nbytes < 12 * rows * cols:
                raise ValueError("the position DeviceBuffer is smaller than its shape")
            pos_pair = (positions.ptr, None)
        else:
            pos = np.ascontiguousarray(positions)
            if pos.shape != (rows, cols, 3) or not np.issubdtype(pos.dtype, np.integer):
                raise ValueError("positions must be (rows, cols, 3) integers")
            if pos.size and (pos.min() < -rg.COORD_MAX or pos.max() > rg.COORD_MAX):
                raise ValueError("a coordinate leaves +-2^29: choose a larger unit")
            pos = pos.astype(np.int32)
            pos_pair = (None, pos.ctypes.data)
        with _Tables(positions.device if dev else None) as t:
            near = t.new(np.int32, (rows, cols), floor=0)
            d2 = t.new(np.uint64, (rows, cols), floor=0)
            self._check(self._lib.mrtx_proximity(self._ctx, C.byref(p), *pos_pair, lab_d, lab_h, *near.pair, *d2.pair,
                                                 C.byref(pairs), C.byref(st)), "mrtx_proximity")
            nearest = near.take((rows, cols))
            dist2 = d2.take((rows, cols))
        self._add_stats(stats, st)
        if isinstance(stats, dict):
            stats["pairs"] = stats.get("pairs", 0) + int(pairs.value)
        return rg.ProximityMap(nearest, dist2, unit_m)

    def region_reach(self, labels, n_regions, prox, shape=None, stats=None):
        """The extremes of a proximity map over each region of a label table (mrtx_regions_reach): the greatest and least
        dist2 of the region's nodes, the least node index attaining each, and the nearest feature of the closest node.
        labels: (rows, cols) int32 or a DeviceBuffer (then give shape = (rows, cols)); prox: a regions.ProximityMap or a pair
        (dist2, nearest) of arrays.  On a to="outside" map of the regions' own labels d2_max and max_at are the radius and
        the centre of the largest circle in each region; on a to="set" map of another set d2_min, min_at and min_nearest say
        how close each region comes to it.  Returns (n_regions,) regions.REACH_DTYPE."""
        from . import regions as rg
        n_regions = int(n_regions)
        lab_d, lab_h, rows, cols, _keep = self._label_arg(labels, shape)
        d2, near = (prox.dist2, prox.nearest) if isinstance(prox, rg.ProximityMap) else prox
        d2 = np.ascontiguousarray(d2, np.uint64)
        near = np.ascontiguousarray(near, np.int32)
        if d2.shape != (rows, cols) or near.shape != (rows, cols):
            raise ValueError("the proximity map and labels differ in shape")
        table = np.zeros(max(n_regions, 1), rg.REACH_DTYPE)
        st = MrtxStats()
        self._check(self._lib.mrtx_regions_reach(self._ctx, rows, cols, lab_d, lab_h, n_regions, None, d2.ctypes.data, None,
                                                 near.ctypes.data, None, table.ctypes.data, C.byref(st)), "mrtx_regions_reach")
        self._add_stats(stats, st)
        return table[:n_regions]

    # ---- Region outlines
    def region_outlines(self, labels, n_regions, connectivity=4, wrap=False, corners=True, row_weights=None, shape=None,
                        stats=None):
        """The ordered boundary rings of each region of a label table (mrtx_regions_outline): every ring from its least side
        on, the region on its right, holes as rings of their own, x unwrapped along a ring that crosses the seam.  labels:
        (rows, cols) int32 or a DeviceBuffer (then give shape = (rows, cols), and the tables are made on the device and
        downloaded).  corners: only the vertices at which a ring turns (else one per boundary side).  row_weights: (rows,)
        uint32 node areas for MrtxRing.warea, or None.  One call counts, a second fills tables of exactly that size.  Returns
        regions.Outlines."""
        from . import regions as rg
        n_regions = int(n_regions)
        lab_d, lab_h, rows, cols, _keep = self._label_arg(labels, shape)
        wp, _kw = self._row_table(row_weights, rows, "row_weights")
        o = _lib.MrtxOutline(rows, cols, 1 if wrap else 0, int(connectivity), _lib.OUTLINE_CORNERS if corners else _lib.OUTLINE_ALL, 0)
        nr, nv = C.c_uint64(0), C.c_uint64(0)

        def call(tables, caps, st):
            (r_d, r_h), (v_d, v_h) = tables
            return self._lib.mrtx_regions_outline(self._ctx, C.byref(o), lab_d, lab_h, n_regions, wp, r_d, r_h, caps[0], v_d, v_h,
                                                  caps[1], C.byref(nr), C.byref(nv), C.byref(st))
        with _Tables(labels.device if lab_d is not None else None) as t:
            (n_r, n_v), (rb, vb) = self._count_then_fill(
                "mrtx_regions_outline", call, (nr, nv), 2,
                lambda n_r, n_v: (t.new(rg.RING_DTYPE, (n_r,), zeros=True), t.new(np.int32, (n_v, 2), zeros=True, floor=8)), stats)
            rings = rb.take((n_r,))
            vertices = vb.take((n_v, 2))
        return rg.Outlines(rings, vertices, rows, cols, wrap)

    # ---- Polygon rasterisation
    def rasterise(self, polygons, shape, wrap=False, rule="nonzero", order="first", row_weights=None, stats=None):
        """Polygons burnt into a label table (mrtx_rasterise), the inverse of region_outlines: every node of a (rows, cols) =
        shape lattice gets the least (order="first") or the greatest (order="last", the painter's order) index among the
        polygons that cover its centre, or -1.  polygons: a regions.Polygons (Outlines.polygons(), Polygons.from_latlon), or
        the device tables with their counts, (rings DeviceBuffer, n_rings, vertices DeviceBuffer, n_vertices, n_polygons,
        subcell_bits): the outputs are then made on the device and downloaded.  rule: "nonzero" (an outline's hole rings take
        its outer ring's winding back to 0) or "evenodd" (for rings whose orientation is not known).  wrap joins the last
        column to the first (cols >= 3).  row_weights: (rows,) uint32 node areas or None.  Needs no DEM.  Returns (labels (rows,
        cols) int32, cover (n_polygons,) regions.COVER_DTYPE); stats gains launches, kernel_ms and crossings."""
        from . import regions as rg
        rules = {"nonzero": _lib.RASTER_NONZERO, "evenodd": _lib.RASTER_EVENODD}
        orders = {"first": _lib.RASTER_FIRST, "last": _lib.RASTER_LAST}
        if rule not in rules:
            raise ValueError('rule must be "nonzero" or "evenodd"')
        if order not in orders:
            raise ValueError('order must be "first" or "last"')
        rows, cols = int(shape[0]), int(shape[1])
        if isinstance(polygons, rg.Polygons):
            device = None
            n_r, n_v, n_p, s = len(polygons), polygons.vertices.shape[0], polygons.n_polygons, polygons.subcell_bits
            r_pair = (None, polygons.rings.ctypes.data if n_r else None)
            v_pair = (None, polygons.vertices.ctypes.data if n_v else None)
        else:
            rb, n_r, vb, n_v, n_p, s = polygons
            if not isinstance(rb, DeviceBuffer) or not isinstance(vb, DeviceBuffer):
                raise ValueError("polygons must be a regions.Polygons or (rings DeviceBuffer, n_rings, vertices DeviceBuffer, "
                                 "n_vertices, n_polygons, subcell_bits)")
            n_r, n_v, n_p, s = int(n_r), int(n_v), int(n_p), int(s)
            if rb.nbytes < rg.RASTER_RING_DTYPE.itemsize * n_r or vb.nbytes < 8 * n_v:
                raise ValueError("a DeviceBuffer is smaller than its count")
            device = rb.device
            r_pair, v_pair = (rb.ptr if n_r else None, None), (vb.ptr if n_v else None, None)
        wp, _kw = self._row_table(row_weights, rows, "row_weights")
        blk = _lib.MrtxRaster(rows, cols, 1 if wrap else 0, s, rules[rule], orders[order], 0)
        st = MrtxStats()
        crossings = C.c_uint64(0)
        with _Tables(device) as t:
            lab = t.new(np.int32, (rows, cols))
            rec = t.new(rg.COVER_DTYPE, (n_p,), zeros=True)
            self._check(self._lib.mrtx_rasterise(self._ctx, C.byref(blk), *r_pair, n_r, *v_pair, n_v, n_p, wp, *lab.pair,
                                                 *(rec.pair if n_p else _NULL), C.byref(crossings), C.byref(st)), "mrtx_rasterise")
            labels = lab.take((rows, cols))
            cover = rec.take((n_p,))
        self._add_stats(stats, st)
        if isinstance(stats, dict):
            stats["crossings"] = stats.get("crossings", 0) + int(crossings.value)
        return labels, cover

    # ---- Contour lines
    def contours(self, z, levels, wrap=False, shape=None, stats=None):
        """The contour lines of a lattice of integer heights at a table of levels (mrtx_contours): every line an ordered run
        of crossed edges with the above side (z >= level) on its right, closed, or open where it meets the lattice's edge or
        a void node.  z: (rows, cols) int32 within +-2^30 (basins.quantise_heights), contours.VOID where there is no node, or
        a DeviceBuffer (then give shape = (rows, cols); the tables are made on the device and downloaded together with the
        heights).  levels: strictly ascending int32 (contours.levels_for), at most 65536.  One call counts, a second fills
        tables of exactly that size.  Needs no DEM.  Returns contours.Contours; stats gains launches, kernel_ms, count_ms and
        fill_ms."""
        from . import contours as ct
        dev = isinstance(z, DeviceBuffer)
        z_d, z_h, z_keep, rows, cols = self._lattice_arg(z, shape, "z")
        lv = np.asarray(levels)
        if lv.ndim != 1 or not 1 <= lv.size <= _lib.CONTOUR_MAX_LEVELS or not np.issubdtype(lv.dtype, np.integer):
            raise ValueError(f"levels must be 1 .. {_lib.CONTOUR_MAX_LEVELS} integers")
        if lv.min() < -2 ** 31 or lv.max() > 2 ** 31 - 1:
            raise ValueError("levels leave int32")
        lv = np.ascontiguousarray(lv, np.int32)
        k = _lib.MrtxContours(rows, cols, 1 if wrap else 0, int(lv.size), 0)
        nl, nv = C.c_uint64(0), C.c_uint64(0)

        def call(tables, caps, st):
            (l_d, l_h), (v_d, v_h) = tables
            return self._lib.mrtx_contours(self._ctx, C.byref(k), z_d, z_h, lv.ctypes.data, l_d, l_h, caps[0], v_d, v_h, caps[1],
                                           C.byref(nl), C.byref(nv), C.byref(st))
        with _Tables(z.device if dev else None) as t:
            (n_l, n_v), (lb, vb) = self._count_then_fill(
                "mrtx_contours", call, (nl, nv), 2,
                lambda n_l, n_v: (t.new(_lib.CONTOUR_LINE_DTYPE, (n_l,), zeros=True), t.new(np.int32, (n_v,), zeros=True)), stats)
            lines = lb.take((n_l,))
            vertices = vb.take((n_v,))
            heights = z.download(np.int32, (rows, cols)) if dev else z_keep
        return ct.Contours(lines, vertices, heights, lv, wrap)

    # ---- Terrain depressions
    def fill_depressions(self, heights, outlets=None, edge_outlets=True, connectivity=8, wrap=False, shape=None, stats=None,
                         unit_m=None):
        """The level up to which every node of a lattice of integer heights is closed (mrtx_fill): the least, over all paths
        to an outlet, of the greatest height on the path.  heights: (rows, cols) int32 within +-2^30 (basins.quantise_heights)
        or a DeviceBuffer (then give shape = (rows, cols); the fill is made in a device table and downloaded together with
        the heights).  Outlets: with edge_outlets the lattice's border rows and, without wrap, its border columns; and the
        nonzero nodes of `outlets`, (rows, cols) uint8 or a DeviceBuffer, if given.  unit_m: the metres of one unit of
        height, remembered by the map.  Needs no DEM.  Returns a moonrtx_amd.basins.FillMap; stats gains launches, kernel_ms
        and visits."""
        from . import basins as bs
        dev = isinstance(heights, DeviceBuffer)
        z_d, z_h, z_keep, rows, cols = self._lattice_arg(heights, shape, "heights")
        o_d, o_h, _ko = self._outlet_arg(outlets, rows, cols)
        f = _lib.MrtxFill(rows, cols, 1 if wrap else 0, int(connectivity), 1 if edge_outlets else 0, 0)
        st = MrtxStats()
        visits = C.c_uint64(0)
        with _Tables(heights.device if dev else None) as t:
            fb = t.new(np.int32, (rows, cols))
            self._check(self._lib.mrtx_fill(self._ctx, C.byref(f), z_d, z_h, o_d, o_h, *fb.pair, C.byref(visits), C.byref(st)),
                        "mrtx_fill")
            fill = fb.take((rows, cols))
            z = heights.download(np.int32, (rows, cols)) if dev else z_keep
        self._add_stats(stats, st)
        if isinstance(stats, dict):
            stats["visits"] = stats.get("visits", 0) + int(visits.value)
        return bs.FillMap(z, fill, unit_m, int(connectivity), bool(wrap))

    def basins(self, labels, n_regions, fillmap, row_weights=None, connectivity=None, wrap=None, shape=None, stats=None):
        """One record per region of a label table over a fill (mrtx_fill_basins): weight, volume, the extremes of the fill,
        the greatest depth and its place, and the pour point, the neighbour outside the region of least (fill, index).
        labels: (rows, cols) int32, any table, or a DeviceBuffer (then give shape = (rows, cols)); fillmap: a basins.FillMap,
        or a pair (z, fill) of (rows, cols) int32 arrays or DeviceBuffers; connectivity and wrap default to the map's (8 and
        False for a pair).  With a DeviceBuffer among the tables the records are made in a device table and downloaded.
        row_weights: (rows,) uint32 node areas or None.  Returns (n_regions,) basins.BASIN_DTYPE."""
        from . import basins as bs
        n_regions = int(n_regions)
        lab_d, lab_h, rows, cols, _keep = self._label_arg(labels, shape)
        if isinstance(fillmap, bs.FillMap):
            z, fill = fillmap.z, fillmap.fill
            connectivity = fillmap.connectivity if connectivity is None else connectivity
            wrap = fillmap.wrap if wrap is None else wrap
        else:
            z, fill = fillmap
            connectivity = 8 if connectivity is None else connectivity
            wrap = False if wrap is None else wrap
        z_d, z_h, _kz = self._int32_arg(z, (rows, cols), "heights")
        f_d, f_h, _kf = self._int32_arg(fill, (rows, cols), "fill")
        wp, _kw = self._row_table(row_weights, rows, "row_weights")
        st = MrtxStats()
        on_dev = [b for b in (labels, z, fill) if isinstance(b, DeviceBuffer)]
        with _Tables(on_dev[0].device if on_dev else None) as t:
            rec = t.new(bs.BASIN_DTYPE, (n_regions,), zeros=True)
            self._check(self._lib.mrtx_fill_basins(self._ctx, rows, cols, 1 if wrap else 0, int(connectivity), lab_d, lab_h,
                                                   n_regions, z_d, z_h, f_d, f_h, wp, *rec.pair, C.byref(st)),
                        "mrtx_fill_basins")
            table = rec.take((n_regions,))
        self._add_stats(stats, st)
        return table

    # ---- The depression hierarchy
    def bowls(self, heights, outlets=None, edge_outlets=True, connectivity=8, wrap=False, invert=False, row_weights=None,
              labels=True, shape=None, stats=None, unit_m=None):
        """The nested closed bowls of a lattice of integer heights (mrtx_bowls): one record per bowl with its floor, its spill
        point, its parent, weight and volume, and per node the innermost bowl that holds it.  heights, outlets, edge_outlets,
        connectivity, wrap and unit_m as in fill_depressions (a DeviceBuffer needs shape = (rows, cols); the tables are then
        made on the device and downloaded).  invert: the same for -heights, levels reported in the caller's heights: summits,
        key cols and prominences.  row_weights: (rows,) uint32 node areas or None.  labels = False leaves the label table out.
        One call counts, a second fills a table of exactly that size.  Needs no DEM.  Returns a moonrtx_amd.basins.BowlTree;
        stats gains launches, kernel_ms, rounds and bowls."""
        from . import basins as bs
        dev = isinstance(heights, DeviceBuffer)
        z_d, z_h, z_keep, rows, cols = self._lattice_arg(heights, shape, "heights")
        o_d, o_h, _ko = self._outlet_arg(outlets, rows, cols)
        wp, _kw = self._row_table(row_weights, rows, "row_weights")
        blk = _lib.MrtxBowls(rows, cols, 1 if wrap else 0, int(connectivity), 1 if edge_outlets else 0, 1 if invert else 0)
        nb, rounds = C.c_uint64(0), C.c_uint64(0)

        def call(tables, caps, st):
            (r_d, r_h), (l_d, l_h) = tables
            return self._lib.mrtx_bowls(self._ctx, C.byref(blk), z_d, z_h, o_d, o_h, wp, r_d, r_h, caps[0], l_d, l_h, C.byref(nb),
                                        C.byref(rounds), C.byref(st))
        with _Tables(heights.device if dev else None) as t:
            (n,), (rb, lb) = self._count_then_fill(
                "mrtx_bowls", call, (nb,), 2,
                lambda n: (t.new(bs.BOWL_DTYPE, (n,), zeros=True), t.new(np.int32, (rows, cols)) if labels else None),
                stats, fill_ms=False)
            records = rb.take((n,))
            table = lb.take((rows, cols)) if labels else None
            z = heights.download(np.int32, (rows, cols)) if dev else z_keep
        if isinstance(stats, dict):
            stats["rounds"] = stats.get("rounds", 0) + int(rounds.value)
            stats["bowls"] = stats.get("bowls", 0) + n
        return bs.BowlTree(records, table, z, unit_m, int(connectivity), bool(wrap), bool(invert))

    def peaks(self, heights, **kw):
        """bowls(invert=True): every summit with its key col (spill_at, spill_level), its prominence (floor_level -
        spill_level) and its parent peak."""
        kw["invert"] = True
        return self.bowls(heights, **kw)
