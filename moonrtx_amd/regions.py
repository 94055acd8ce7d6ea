"""Connected regions of a per-node terrain map: what MoonRT.regions returns, the per-row node areas
that make a region's area an exact integer sum, and helpers over the catalogue.

A region is a connected component (4- or 8-connected, the columns joined across the seam when the map is wrapped) of the nodes
a predicate selects; its root is its least node index i cols + j, and regions are numbered in ascending order of their roots.
The catalogue is all integers: it does not depend on the order in which the device summed it."""
import math

import numpy as np

# mirrors MrtxRegion (include/moonrt.h), 56 bytes
REGION_DTYPE = np.dtype([("weight", "<u8"), ("sum_i", "<i8"), ("sum_dj", "<i8"), ("count", "<u4"), ("root_i", "<i4"),
                         ("root_j", "<i4"), ("i_min", "<i4"), ("i_max", "<i4"), ("dj_min", "<i4"), ("dj_max", "<i4"),
                         ("reserved", "<u4")])
assert REGION_DTYPE.itemsize == 56

# mirrors MrtxZonal, 56 bytes: one channel of one region
ZONAL_DTYPE = np.dtype([("wcount", "<u8"), ("wsum", "<i8"), ("sum", "<i8"), ("count", "<u4"), ("n_nan", "<u4"),
                        ("n_clipped", "<u4"), ("min", "<f4"), ("max", "<f4"), ("min_at", "<i4"), ("max_at", "<i4"),
                        ("reserved", "<u4")])
assert ZONAL_DTYPE.itemsize == 56
# mirrors MrtxRegionShape, 32 bytes
SHAPE_DTYPE = np.dtype([("perimeter", "<u8"), ("sides_ns", "<u4"), ("sides_ew", "<u4"), ("q1", "<u4"), ("q3", "<u4"),
                        ("qd", "<u4"), ("euler", "<i4")])
assert SHAPE_DTYPE.itemsize == 32
# mirrors MrtxRegionReach, 32 bytes
REACH_DTYPE = np.dtype([("d2_max", "<u8"), ("d2_min", "<u8"), ("max_at", "<i4"), ("min_at", "<i4"), ("min_nearest", "<i4"),
                        ("count", "<u4")])
assert REACH_DTYPE.itemsize == 32
# mirrors MrtxRing, 48 bytes
RING_DTYPE = np.dtype([("area", "<i8"), ("warea", "<i8"), ("first", "<u8"), ("n_sides", "<u4"), ("n_vertices", "<u4"),
                       ("label", "<i4"), ("head", "<i4"), ("wind", "<i4"), ("reserved", "<u4")])
assert RING_DTYPE.itemsize == 48
# mirrors MrtxRasterRing, 24 bytes
RASTER_RING_DTYPE = np.dtype([("first", "<u8"), ("n_vertices", "<u4"), ("polygon", "<i4"), ("wind", "<i4"), ("reserved", "<u4")])
assert RASTER_RING_DTYPE.itemsize == 24
# mirrors MrtxPolygonCover, 40 bytes
COVER_DTYPE = np.dtype([("weight", "<u8"), ("owned_weight", "<u8"), ("count", "<u4"), ("owned", "<u4"), ("i_min", "<i4"),
                        ("i_max", "<i4"), ("first_at", "<i4"), ("reserved", "<u4")])
assert COVER_DTYPE.itemsize == 40

WEIGHT_MAX = 2 ** 32 - 1
# every coordinate of a node position lies in -COORD_MAX .. COORD_MAX (mrtx_proximity)
COORD_MAX = 2 ** 29
NO_FEATURE = np.uint64(2 ** 64 - 1)
# every vertex coordinate of a polygon lies in -RASTER_COORD_MAX .. RASTER_COORD_MAX (mrtx_rasterise), in units of 2^-s of a cell
RASTER_COORD_MAX = 2 ** 24
RASTER_MAX_SUBCELL = 8


def row_weights(window, dem_hw, radius_m=1737400.0, unit_m2=1.0):
    """(rows,) uint32: the area of one lattice cell of every row of a window (row0, col0, rows, cols[, stride[, wrap]]) of an
    (H, W) DEM, in units of unit_m2 square metres, rounded to the nearest integer.  A cell is stride 2 pi / W wide in
    longitude; in latitude it reaches half a row spacing (stride pi / H / 2) either side of the latitude of the row's texel
    centres, pi / 2 - (row + 1 / 2) pi / H, clipped to the poles.  float64 spherical area radius_m^2 dlon (sin a - sin b).
    ValueError for a weight that rounds to zero or does not fit 32 bits: choose another unit."""
    from .traverse import window_dict
    w = window_dict(window)
    H, W = (int(v) for v in dem_hw)
    if not (radius_m > 0.0 and unit_m2 > 0.0 and math.isfinite(radius_m) and math.isfinite(unit_m2)):
        raise ValueError("radius_m and unit_m2 must be finite and > 0")
    if w["rows"] < 1 or w["stride"] < 1 or H < 1 or W < 1:
        raise ValueError("empty window or DEM")
    if w["row0"] < 0 or w["row0"] + (w["rows"] - 1) * w["stride"] >= H:
        raise ValueError(f"the window's rows leave the DEM's {H} rows")
    row = w["row0"] + np.arange(w["rows"], dtype=np.float64) * w["stride"]
    lat = 0.5 * math.pi - (row + 0.5) * (math.pi / H)
    half = 0.5 * w["stride"] * math.pi / H
    north = np.minimum(lat + half, 0.5 * math.pi)
    south = np.maximum(lat - half, -0.5 * math.pi)
    area = float(radius_m) ** 2 * (w["stride"] * 2.0 * math.pi / W) * (np.sin(north) - np.sin(south))
    q = np.rint(area / float(unit_m2))
    if not np.all(q >= 1.0):
        k = int(np.argmin(q))
        raise ValueError(f"row {k}: a node's area {area[k]:g} m^2 rounds to zero units of {unit_m2:g} m^2: use a smaller unit")
    if not np.all(q <= WEIGHT_MAX):
        k = int(np.argmax(q))
        raise ValueError(f"row {k}: a node's area {area[k]:g} m^2 does not fit 32 bits in units of {unit_m2:g} m^2: use a larger unit")
    return q.astype(np.uint32)


def side_weights(window, dem_hw, radius_m=1737400.0, unit_m=1.0):
    """(side_ew (rows,), side_ns (rows + 1,)) uint32: the lengths of the sides of a lattice cell of every row of a window, in
    units of unit_m metres, rounded to the nearest integer, by row_weights' row convention: a cell reaches half a row spacing
    either side of its row's latitude, clipped to the poles.  side_ew[i] is the meridian arc radius_m (north - south) of row
    i's cells; side_ns[i] the arc of the parallel between rows i - 1 and i, radius_m cos(lat) dlon (entry 0: the north edge of
    row 0; entry rows: the south edge of the last row).  ValueError for a length that rounds to zero (a side on a pole) or
    does not fit 32 bits: choose another unit or window."""
    from .traverse import window_dict
    w = window_dict(window)
    H, W = (int(v) for v in dem_hw)
    if not (radius_m > 0.0 and unit_m > 0.0 and math.isfinite(radius_m) and math.isfinite(unit_m)):
        raise ValueError("radius_m and unit_m must be finite and > 0")
    if w["rows"] < 1 or w["stride"] < 1 or H < 1 or W < 1:
        raise ValueError("empty window or DEM")
    if w["row0"] < 0 or w["row0"] + (w["rows"] - 1) * w["stride"] >= H:
        raise ValueError(f"the window's rows leave the DEM's {H} rows")
    row = w["row0"] + np.arange(w["rows"], dtype=np.float64) * w["stride"]
    lat = 0.5 * math.pi - (row + 0.5) * (math.pi / H)
    half = 0.5 * w["stride"] * math.pi / H
    north = np.minimum(lat + half, 0.5 * math.pi)
    south = np.maximum(lat - half, -0.5 * math.pi)
    dlon = w["stride"] * 2.0 * math.pi / W
    ew = float(radius_m) * (north - south)
    ns = float(radius_m) * dlon * np.cos(np.concatenate([north, south[-1:]]))
    out = []
    for name, length in (("side_ew", ew), ("side_ns", ns)):
        q = np.rint(length / float(unit_m))
        if not np.all(q >= 1.0):
            k = int(np.argmin(q))
            raise ValueError(f"{name}[{k}]: a side of {length[k]:g} m rounds to zero units of {unit_m:g} m: use a smaller unit")
        if not np.all(q <= WEIGHT_MAX):
            k = int(np.argmax(q))
            raise ValueError(f"{name}[{k}]: a side of {length[k]:g} m does not fit 32 bits in units of {unit_m:g} m: use a larger unit")
        out.append(q.astype(np.uint32))
    return out[0], out[1]


def fixed_point(x, scale):
    """q of a float32 value as mrtx_regions_zonal forms it, a Python integer: rint(float64(x) * scale), and +-2^31 with the
    product's sign when |float64(x) * scale| >= 2^31."""
    p = float(np.float64(np.float32(x)) * np.float64(scale))
    if abs(p) >= 2.0 ** 31:
        return -2 ** 31 if p < 0.0 else 2 ** 31
    return int(np.rint(p))


def check_wsum(z, scale):
    """OverflowError when a record's weighted sum may have wrapped: max(|q(min)|, |q(max)|) * wcount >= 2^63, in Python
    integers from the record itself.  Every |q| of the record is at most that maximum, so a wsum that passes did not wrap."""
    z = np.asarray(z)
    flat = z.reshape(-1)
    for k in np.flatnonzero(flat["count"] > 0):
        r = flat[k]
        bound = max(abs(fixed_point(r["min"], scale)), abs(fixed_point(r["max"], scale))) * int(r["wcount"])
        if bound >= 2 ** 63:
            raise OverflowError(f"record {int(k)}: |q| up to 2^{math.log2(max(bound // int(r['wcount']), 1)):.1f} times a weight "
                                f"of {int(r['wcount'])} may exceed 63 bits, so wsum may have wrapped: lower scale")


def zonal_mean(z, scale):
    """float64 mean of every record: sum / count / scale (NaN where count == 0)."""
    z = np.asarray(z)
    cnt = z["count"].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(cnt > 0, z["sum"].astype(np.float64) / cnt / float(scale), np.nan)


def zonal_area_mean(z, scale):
    """float64 weighted mean of every record: wsum / wcount / scale (NaN where wcount == 0)."""
    z = np.asarray(z)
    w = z["wcount"].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(w > 0, z["wsum"].astype(np.float64) / w / float(scale), np.nan)


def holes(shape, table=None, cols=None, wrap=False):
    """(holes, may_wind): holes = 1 - euler of every region of a SHAPE_DTYPE table, right for a connected region that does not
    wind round the seam; may_wind marks the regions of a wrapped map whose dj extent spans all cols columns (table: the
    catalogue, REGION_DTYPE), which may wind and then read one hole more."""
    shape = np.asarray(shape)
    h = 1 - shape["euler"].astype(np.int64)
    wind = np.zeros(h.shape, bool)
    if wrap and table is not None:
        if cols is None:
            raise ValueError("give cols with a wrapped map's table")
        t = np.asarray(table)
        wind = (t["dj_max"].astype(np.int64) - t["dj_min"].astype(np.int64) + 1 >= int(cols)) & (t["count"] > 0)
    return h, wind


def node_positions(window, dem_hw, radius_m=1737400.0, unit_m=0.01, heights_m=None):
    """(rows, cols, 3) int32: the positions of the nodes of a window (row0, col0, rows, cols[, stride[, wrap]]) of an (H, W)
    DEM in units of unit_m metres, for MoonRT.proximity: rint((radius_m + h) (cos lat cos lon, cos lat sin lon, sin lat) /
    unit_m) in float64, h = heights_m (a scalar or (rows, cols) metres above the sphere) or 0.  lat and lon are the texel
    centres of MoonRT.traverse_nodes and row_weights, in radians: lat = pi / 2 - (row + 1 / 2) pi / H of row = row0 + i
    stride, lon = -pi + (col + 1 / 2) 2 pi / W of col = (col0 + j stride) mod W.  ValueError when a coordinate leaves
    +-2^29: choose a larger unit."""
    from .traverse import window_dict
    w = window_dict(window)
    H, W = (int(v) for v in dem_hw)
    if not (radius_m > 0.0 and unit_m > 0.0 and math.isfinite(radius_m) and math.isfinite(unit_m)):
        raise ValueError("radius_m and unit_m must be finite and > 0")
    if w["rows"] < 1 or w["cols"] < 1 or w["stride"] < 1 or H < 1 or W < 1:
        raise ValueError("empty window or DEM")
    if w["row0"] < 0 or w["row0"] + (w["rows"] - 1) * w["stride"] >= H:
        raise ValueError(f"the window's rows leave the DEM's {H} rows")
    row = w["row0"] + np.arange(w["rows"], dtype=np.float64) * w["stride"]
    col = ((w["col0"] + np.arange(w["cols"], dtype=np.int64) * w["stride"]) % W).astype(np.float64)
    lat = (0.5 * math.pi - (row + 0.5) * (math.pi / H))[:, None]
    lon = (-math.pi + (col + 0.5) * (2.0 * math.pi / W))[None, :]
    r = np.full((w["rows"], w["cols"]), float(radius_m))
    if heights_m is not None:
        h = np.asarray(heights_m, np.float64)
        if h.shape not in ((), (w["rows"], w["cols"])) or not np.all(np.isfinite(h)):
            raise ValueError("heights_m must be a finite scalar or (rows, cols)")
        r = r + h
    p = np.stack([r * np.cos(lat) * np.cos(lon), r * np.cos(lat) * np.sin(lon), r * np.sin(lat) * np.ones_like(lon)], -1)
    q = np.rint(p / float(unit_m))
    if not np.all(np.abs(q) <= COORD_MAX):
        raise ValueError(f"a coordinate of {np.abs(p).max():g} m leaves +-2^29 units of {unit_m:g} m: choose a larger unit")
    return q.astype(np.int32)


class Outlines:
    """What MoonRT.region_outlines returns: rings (n,) RING_DTYPE in ascending order of their heads;
    vertices (m, 2) int32 (y, x) corner coordinates, ring after ring, each ring from its head on with the region on its right
    (rows run down, columns right), x unwrapped along a ring that crosses the seam; rows, cols, wrap: the lattice.

    holes() counts a label's hole rings (wind == 0 and area < 0).  Unlike regions.holes, which reads 1 - euler and is one too
    many for a region that winds round the seam, this count is right for winding regions too: a winding ring counts neither
    as an outer ring nor as a hole."""

    def __init__(self, rings, vertices, rows, cols, wrap=False):
        self.rings = np.ascontiguousarray(rings, RING_DTYPE).reshape(-1)
        self.vertices = np.ascontiguousarray(vertices, np.int32).reshape(-1, 2)
        self.rows, self.cols, self.wrap = int(rows), int(cols), bool(wrap)
        if int(self.rings["n_vertices"].astype(np.int64).sum()) != self.vertices.shape[0]:
            raise ValueError("the rings' n_vertices do not add up to the vertex table")

    def __len__(self):
        return int(self.rings.shape[0])

    def ring(self, r):
        """(n_vertices, 2) int32: the vertices of ring r, a view of the vertex table."""
        rec = self.rings[int(r)]
        return self.vertices[int(rec["first"]):int(rec["first"]) + int(rec["n_vertices"])]

    def role(self, r):
        """"outer" (wind == 0, area > 0), "hole" (wind == 0, area < 0) or "winding" (wind != 0: the ring goes round the window)."""
        rec = self.rings[int(r)]
        if rec["wind"] != 0:
            return "winding"
        return "outer" if rec["area"] > 0 else "hole"

    def of(self, label):
        """The numbers of a label's rings: outer rings first, then winding rings, then holes, each in ring order."""
        idx = np.flatnonzero(self.rings["label"] == int(label))
        order = {"outer": 0, "winding": 1, "hole": 2}
        return np.array(sorted(idx, key=lambda r: (order[self.role(r)], r)), np.int64)

    def holes(self, n_regions=None):
        """(n_regions,) int64: per label the number of hole rings (n_regions: one more than the greatest label when not given)."""
        lab = self.rings["label"].astype(np.int64)
        n = int(n_regions) if n_regions is not None else (int(lab.max()) + 1 if lab.size else 0)
        hole = (self.rings["wind"] == 0) & (self.rings["area"] < 0)
        return np.bincount(lab[hole], minlength=n).astype(np.int64)

    def corner_latlon(self, window, dem_hw):
        """(m, 2) float64 (lat, lon) degrees of every vertex, for a window (row0, col0, rows, cols[, stride[, wrap]]) of an
        (H, W) DEM.  Corners sit on the cell edges of row_weights / side_weights' convention, half a row or column spacing off
        the texel-centre nodes: lat = 90 - (row0 + (y - 1 / 2) stride + 1 / 2) 180 / H clipped to the poles, lon = -180 +
        (col0 + (x - 1 / 2) stride + 1 / 2) 360 / W.  lon is continuous along a ring: the unwrapped x of a ring across the seam
        gives longitudes beyond +-180, which the caller may reduce."""
        from .traverse import window_dict
        w = window_dict(window)
        H, W = (int(v) for v in dem_hw)
        if w["stride"] < 1 or H < 1 or W < 1:
            raise ValueError("empty window or DEM")
        y = self.vertices[:, 0].astype(np.float64)
        x = self.vertices[:, 1].astype(np.float64)
        lat = 90.0 - (w["row0"] + (y - 0.5) * w["stride"] + 0.5) * (180.0 / H)
        lon = -180.0 + (w["col0"] + (x - 0.5) * w["stride"] + 0.5) * (360.0 / W)
        return np.stack([np.clip(lat, -90.0, 90.0), lon], -1)

    def polygons(self, n_regions=None):
        """The rings as the Polygons of MoonRT.rasterise, label as polygon, in the outlines' own coordinates (subcell_bits 0):
        rasterising them gives back the label table (n_regions: one more than the greatest label when not given)."""
        lab = self.rings["label"].astype(np.int64)
        n = int(n_regions) if n_regions is not None else (int(lab.max()) + 1 if lab.size else 0)
        rings = np.zeros(len(self), RASTER_RING_DTYPE)
        for name, src in (("first", "first"), ("n_vertices", "n_vertices"), ("polygon", "label"), ("wind", "wind")):
            rings[name] = self.rings[src]
        return Polygons(rings, self.vertices, n, 0)


class Polygons:
    """What MoonRT.rasterise burns into a label table: rings (n,) RASTER_RING_DTYPE, each a run of the
    vertex table that belongs to a polygon; vertices (m, 2) int32 (y, x) corner coordinates in units of 2^-subcell_bits of a
    cell, x unwrapped along a ring; n_polygons; subcell_bits 0 .. 8.  A ring closes from its last vertex to its first, wind
    times round a wrapped window."""

    def __init__(self, rings, vertices, n_polygons, subcell_bits=0):
        self.rings = np.ascontiguousarray(rings, RASTER_RING_DTYPE).reshape(-1)
        self.vertices = np.ascontiguousarray(vertices, np.int32).reshape(-1, 2)
        self.n_polygons, self.subcell_bits = int(n_polygons), int(subcell_bits)
        if not 0 <= self.subcell_bits <= RASTER_MAX_SUBCELL:
            raise ValueError("subcell_bits must lie in 0 .. 8")
        if self.n_polygons < 0:
            raise ValueError("n_polygons must be >= 0")
        if int(self.rings["n_vertices"].astype(np.int64).sum()) != self.vertices.shape[0]:
            raise ValueError("the rings' n_vertices do not add up to the vertex table")

    def __len__(self):
        return int(self.rings.shape[0])

    def ring(self, r):
        """(n_vertices, 2) int32: the vertices of ring r, a view of the vertex table."""
        rec = self.rings[int(r)]
        return self.vertices[int(rec["first"]):int(rec["first"]) + int(rec["n_vertices"])]

    @classmethod
    def from_rings(cls, rings, n_polygons=None, subcell_bits=0):
        """From [(polygon, (n, 2) integer (y, x) vertices[, wind])], ring after ring."""
        recs = np.zeros(len(rings), RASTER_RING_DTYPE)
        verts, at = [], 0
        for k, ring in enumerate(rings):
            v = np.asarray(ring[1], np.int64).reshape(-1, 2)
            recs[k] = (at, len(v), int(ring[0]), int(ring[2]) if len(ring) > 2 else 0, 0)
            verts.append(v)
            at += len(v)
        n = int(n_polygons) if n_polygons is not None else (int(recs["polygon"].max()) + 1 if len(recs) else 0)
        table = np.concatenate(verts) if verts else np.zeros((0, 2), np.int64)
        if table.size and np.abs(table).max() > 2 ** 31 - 1:
            raise ValueError("a coordinate leaves int32")
        return cls(recs, table.astype(np.int32), n, subcell_bits)

    @classmethod
    def from_latlon(cls, window, dem_hw, polygons, subcell_bits=4):
        """The inverse of Outlines.corner_latlon: polygons is a sequence of polygons, each a sequence of rings, each (n, 2)
        (lat, lon) degrees, for a window (row0, col0, rows, cols[, stride[, wrap]]) of an (H, W) DEM.  y = ((90 - lat) H / 180 -
        1 / 2 - row0) / stride + 1 / 2 and x = ((lon + 180) W / 360 - 1 / 2 - col0) / stride + 1 / 2 in float64, each quantised
        as floor(v 2^s + 1 / 2).  Longitude is kept continuous along a ring: every vertex takes the longitude nearest to its
        predecessor's (steps of less than 180 degrees), so a ring across the seam stays unwrapped; a ring that comes back to
        its first vertex a whole turn on winds round the window (wrap only).  A repeated closing vertex is dropped.
        ValueError when a coordinate leaves +-2^24 units: lower subcell_bits."""
        from .traverse import window_dict
        w = window_dict(window)
        H, W = (int(v) for v in dem_hw)
        s = int(subcell_bits)
        if not 0 <= s <= RASTER_MAX_SUBCELL:
            raise ValueError("subcell_bits must lie in 0 .. 8")
        if w["stride"] < 1 or H < 1 or W < 1:
            raise ValueError("empty window or DEM")
        out = []
        for p, poly in enumerate(polygons):
            for ring in poly:
                ll = np.asarray(ring, np.float64).reshape(-1, 2)
                if not len(ll) or not np.all(np.isfinite(ll)):
                    raise ValueError(f"polygon {p}: a ring needs at least one finite (lat, lon) vertex")
                lon = ll[:, 1].copy()
                for k in range(1, len(lon)):
                    lon[k] = lon[k - 1] + ((lon[k] - lon[k - 1] + 180.0) % 360.0 - 180.0)
                n, wind = len(ll), 0
                if n > 1 and ll[-1, 0] == ll[0, 0]:
                    turns = (lon[-1] - lon[0]) / 360.0
                    if turns == round(turns):                   # the first vertex again, perhaps a whole turn on
                        n, wind = n - 1, int(round(turns))
                if wind and not w["wrap"]:
                    raise ValueError(f"polygon {p}: a ring goes round the globe, the window does not")
                y = ((90.0 - ll[:n, 0]) * (H / 180.0) - 0.5 - w["row0"]) / w["stride"] + 0.5
                x = ((lon[:n] + 180.0) * (W / 360.0) - 0.5 - w["col0"]) / w["stride"] + 0.5
                q = np.floor(np.stack([y, x], -1) * float(2 ** s) + 0.5)
                if np.abs(q).max() > RASTER_COORD_MAX:
                    raise ValueError(f"polygon {p}: a coordinate leaves +-2^24 units of 2^-{s} of a cell: lower subcell_bits")
                out.append((p, q.astype(np.int64), wind))
        return cls.from_rings(out, len(polygons), s)


class ProximityMap:
    """What MoonRT.proximity returns: nearest (rows, cols) int32, the node index of every node's
    nearest feature (-1: there is none); dist2 (rows, cols) uint64, the exact squared distance to it in squared units of the
    positions (2^64 - 1: none); unit_m, the metres of one unit of the positions, or None when they are not metres."""

    def __init__(self, nearest, dist2, unit_m=None):
        self.nearest = np.ascontiguousarray(nearest, np.int32)
        self.dist2 = np.ascontiguousarray(dist2, np.uint64)
        if self.nearest.ndim != 2 or self.dist2.shape != self.nearest.shape:
            raise ValueError("nearest and dist2 must be (rows, cols) alike")
        self.unit_m = None if unit_m is None else float(unit_m)

    def _unit(self):
        if self.unit_m is None:
            raise ValueError("the map has no unit: give unit_m")
        return self.unit_m

    def chord_m(self):
        """(rows, cols) float64: the straight-line distance sqrt(dist2) unit_m to the nearest feature, inf where there is none."""
        u = self._unit()
        return np.where(self.nearest < 0, np.inf, np.sqrt(self.dist2.astype(np.float64)) * u)

    def arc_m(self, radius_m=1737400.0):
        """(rows, cols) float64: the great-circle distance 2 R asin(chord / 2 R) on a sphere of radius_m of two points that
        lie on it (a chord longer than the diameter reads as the half circle); inf where there is no feature."""
        c = self.chord_m()
        none = ~np.isfinite(c)
        x = np.minimum(np.where(none, 0.0, c) / (2.0 * float(radius_m)), 1.0)
        return np.where(none, np.inf, 2.0 * float(radius_m) * np.arcsin(x))

    def nearest_label(self, labels):
        """(rows, cols) int32: the label of every node's nearest feature, the Voronoi allocation of the nodes to the regions
        of `labels`; -1 where nearest is -1."""
        lab = np.ascontiguousarray(labels, np.int32)
        if lab.shape != self.nearest.shape:
            raise ValueError("labels and the map differ in shape")
        return np.where(self.nearest < 0, -1, lab.reshape(-1)[np.maximum(self.nearest, 0)]).astype(np.int32)

    def within(self, distance_m):
        """(rows, cols) bool: the buffer chord_m() <= distance_m, compared in integers: dist2 <= floor((distance_m /
        unit_m)^2), the quotient and the square in float64, the comparison exact.  A node without a feature is never
        within, nor is any node for a negative or NaN distance."""
        t = float(distance_m) / self._unit()
        if not t >= 0.0:
            return np.zeros(self.dist2.shape, bool)
        sq = t * t
        limit = 2 ** 64 - 2 if sq >= 2.0 ** 64 else min(int(math.floor(sq)), 2 ** 64 - 2)
        return self.dist2 <= np.uint64(limit)


class RegionMap:
    """labels (rows, cols) int32, the region's number or -1; table (n,) REGION_DTYPE; n; wrap; unit_m2 = the square metres of
    one unit of weight when the map was made with row weights of a known unit (else None: a weight is a node count or the
    caller's own unit)."""

    def __init__(self, labels, table, wrap=False, unit_m2=None):
        self.labels = np.ascontiguousarray(labels, np.int32)
        self.table = np.ascontiguousarray(table, REGION_DTYPE).reshape(-1)
        if self.labels.ndim != 2:
            raise ValueError("labels must be (rows, cols)")
        self.n = int(self.table.shape[0])
        self.wrap = bool(wrap)
        self.unit_m2 = None if unit_m2 is None else float(unit_m2)

    def area_m2(self, unit_m2=None):
        """(n,) float64 areas: weight x unit_m2 (the map's own unit when none is given)."""
        u = self.unit_m2 if unit_m2 is None else float(unit_m2)
        if u is None:
            raise ValueError("the map has no unit: give unit_m2")
        return self.table["weight"].astype(np.float64) * u

    def centroids(self, lat, lon):
        """(n, 2) float64 (lat, lon) degrees of the regions' node-count centroids, from the node axes lat (rows,) and lon
        (cols,) (MoonRT.traverse_nodes): row sum_i / count, column root_j + sum_dj / count, so a region that straddles the
        seam of a wrapped map has its centroid on the seam and not half a circle away.  lon comes back in [-180, 180)."""
        lat, lon = np.asarray(lat, np.float64), np.asarray(lon, np.float64)
        rows, cols = self.labels.shape
        if lat.shape != (rows,) or lon.shape != (cols,):
            raise ValueError("lat must be (rows,) and lon (cols,)")
        t = self.table
        cnt = np.maximum(t["count"].astype(np.float64), 1.0)
        dlat = lat[1] - lat[0] if rows > 1 else 0.0
        dlon = ((lon[1] - lon[0] + 180.0) % 360.0 - 180.0) if cols > 1 else 0.0
        la = lat[0] + (t["sum_i"] / cnt) * dlat
        lo = lon[np.clip(t["root_j"], 0, cols - 1)] + (t["sum_dj"] / cnt) * dlon
        return np.stack([la, (lo + 180.0) % 360.0 - 180.0], -1)

    def zonal(self, rt, field, row_weights=None, scale=1.0, hist=None, stats=None):
        """MoonRT.region_statistics of a (rows, cols[, n_ch]) float32 field over this map's regions."""
        return rt.region_statistics(self.labels, self.n, field, row_weights=row_weights, scale=scale, hist=hist, wrap=self.wrap,
                                    stats=stats)

    def shapes(self, rt, connectivity=4, side_ew=None, side_ns=None, stats=None):
        """MoonRT.region_shapes of this map's regions."""
        return rt.region_shapes(self.labels, self.n, connectivity=connectivity, wrap=self.wrap, side_ew=side_ew, side_ns=side_ns,
                                stats=stats)

    def holes(self, shape):
        """regions.holes of a shape table of this map: (holes, may_wind)."""
        return holes(shape, self.table, self.labels.shape[1], self.wrap)

    def outlines(self, rt, connectivity=4, corners=True, row_weights=None, stats=None):
        """MoonRT.region_outlines of this map's regions: an Outlines."""
        return rt.region_outlines(self.labels, self.n, connectivity=connectivity, wrap=self.wrap, corners=corners,
                                  row_weights=row_weights, stats=stats)

    def proximity(self, rt, positions, to="set", unit_m=None, stats=None):
        """MoonRT.proximity of this map's labels: every node's nearest node of any region (to="set") or nearest node outside
        every region (to="outside"), over (rows, cols, 3) int32 positions (node_positions)."""
        return rt.proximity(self.labels, positions, to=to, unit_m=unit_m, stats=stats)

    def reach(self, rt, prox, stats=None):
        """MoonRT.region_reach of a ProximityMap over this map's regions: (n,) REACH_DTYPE."""
        return rt.region_reach(self.labels, self.n, prox, stats=stats)

    def inscribed(self, rt, positions, unit_m=0.01, stats=None):
        """(radius_m (n,) float64, centre_node (n,) int32): the largest circle that fits in each region, from the distances to
        the nearest node outside every region: its centre is the region's node farthest from one (the least index among
        equals) and its radius that chord, sqrt(d2_max) unit_m.  inf and the region's least node when no node of the window
        lies outside a region.  Nodes beyond the window's edge are not "outside": a region that touches the edge (the i_min
        / i_max and dj_min / dj_max extents of the catalogue tell which) may read a circle that leaves the window."""
        prox = self.proximity(rt, positions, to="outside", unit_m=unit_m, stats=stats)
        r = self.reach(rt, prox, stats=stats)
        none = r["d2_max"] == NO_FEATURE
        return np.where(none, np.inf, np.sqrt(r["d2_max"].astype(np.float64)) * float(unit_m)), r["max_at"].copy()

    def largest(self, k=1):
        """The numbers of the k regions of greatest weight, greatest first (equal weights: the lower number first)."""
        order = np.lexsort((np.arange(self.n), -self.table["weight"].astype(np.float64)))
        return order[:max(int(k), 0)]

    def filter(self, min_count=0, min_area=0.0):
        """A new RegionMap of the regions with count >= min_count and area >= min_area (square metres when the map has a
        unit, else units of weight), renumbered in their old order; the nodes of the others get -1."""
        t = self.table
        area = t["weight"].astype(np.float64) * (self.unit_m2 if self.unit_m2 is not None else 1.0)
        keep = (t["count"] >= min_count) & (area >= min_area)
        new = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
        lut = np.concatenate([new, np.array([-1], np.int32)])       # label -1 reads the last entry
        return RegionMap(lut[self.labels], t[keep], self.wrap, self.unit_m2)
