"""An independent model of the polygon rasterisation, straight from the rule: every edge against every
column centre it spans, the height of the crossing as a fractions.Fraction in the vertices' own units (not the kernels' doubled
integers), Python integers for every sum.  It shares no code with the package."""
import math
from fractions import Fraction

import numpy as np

RING = np.dtype([("first", "<u8"), ("n_vertices", "<u4"), ("polygon", "<i4"), ("wind", "<i4"), ("reserved", "<u4")])
COVER = np.dtype([("weight", "<u8"), ("owned_weight", "<u8"), ("count", "<u4"), ("owned", "<u4"), ("i_min", "<i4"),
                  ("i_max", "<i4"), ("first_at", "<i4"), ("reserved", "<u4")])
NONZERO, EVENODD = 0, 1
FIRST, LAST = 0, 1


def crossings(rings, vertices, rows, cols, wrap=False, s=0):
    """[(polygon, column, first row clipped to 0 .. rows, sign)] of every hit of an edge on a column centre inside the lattice."""
    unit = 2 ** s                                   # units per cell
    V = np.asarray(vertices).reshape(-1, 2).tolist()
    out = []
    for g in np.asarray(rings).reshape(-1).tolist():
        first, n, polygon, wind = int(g[0]), int(g[1]), int(g[2]), int(g[3])
        pts = [tuple(V[first + k]) for k in range(n)]
        pts.append((pts[0][0], pts[0][1] + wind * cols * unit))
        for (y0, x0), (y1, x1) in zip(pts[:-1], pts[1:]):
            if x0 == x1:
                continue
            lo, hi = min(x0, x1), max(x0, x1)
            ju = math.ceil(Fraction(lo, unit) - Fraction(1, 2))         # the first centre (ju + 1/2) unit at or after lo
            while (2 * ju + 1) * unit < 2 * hi:                          # ... and before hi
                xc = Fraction(2 * ju + 1, 2) * unit
                ys = y0 + (xc - x0) * Fraction(y1 - y0, x1 - x0)
                i0 = math.ceil(ys / unit - Fraction(1, 2))              # the rows whose centre (i + 1/2) unit is at or below
                if wrap or 0 <= ju < cols:
                    out.append((polygon, ju % cols, min(max(i0, 0), rows), 1 if x1 > x0 else -1))
                ju += 1
    return out


def raster(rings, vertices, n_polygons, rows, cols, wrap=False, s=0, rule=NONZERO, order=FIRST, row_weight=None, hits=None):
    """(labels (rows, cols) int32, cover (n_polygons,) COVER, the number of crossings); hits: what crossings() gave for the same
    polygons and lattice, to save working it out again."""
    if hits is None:
        hits = crossings(rings, vertices, rows, cols, wrap, s)
    per = {}
    for p, j, i0, sg in hits:
        per.setdefault(p, []).append((j, i0, sg))
    labels = np.full((rows, cols), -1, np.int32)
    covered = {}
    for p in sorted(per):
        used = sorted({j for j, _, _ in per[p]})
        at = {j: k for k, j in enumerate(used)}
        d = np.zeros((rows + 1, len(used)), np.int64)
        for j, i0, sg in per[p]:
            d[i0, at[j]] += sg
        w = np.cumsum(d, axis=0)[:rows]
        c = (w % 2 != 0) if rule == EVENODD else (w != 0)
        ii, kk = np.nonzero(c)
        if ii.size:
            jj = np.asarray(used, np.int64)[kk]
            covered[p] = (ii, jj)
            if order == LAST:
                labels[ii, jj] = p
            else:
                free = labels[ii, jj] < 0
                labels[ii[free], jj[free]] = p
    cover = np.zeros(n_polygons, COVER)
    cover["i_min"] = cover["i_max"] = cover["first_at"] = -1
    weight = [1] * rows if row_weight is None else [int(v) for v in row_weight]
    for p, (ii, jj) in covered.items():
        own = labels[ii, jj] == p
        cover[p] = (sum(weight[i] for i in ii.tolist()), sum(weight[i] for i in ii[own].tolist()), ii.size, int(own.sum()),
                    int(ii.min()), int(ii.max()), int((ii * cols + jj).min()), 0)
    return labels, cover, len(hits)


def rings_of_outlines(outline_rings):
    """The RING records of an outline_model.trace ring table, label as polygon."""
    out = np.zeros(len(outline_rings), RING)
    out["first"], out["n_vertices"] = outline_rings["first"], outline_rings["n_vertices"]
    out["polygon"], out["wind"] = outline_rings["label"], outline_rings["wind"]
    return out


def polygons(rings, s=0):
    """(RING records, (m, 2) int32 vertices) from [(polygon, [(y, x), ...][, wind])], ring after ring."""
    recs, verts = np.zeros(len(rings), RING), []
    for k, ring in enumerate(rings):
        recs[k] = (len(verts), len(ring[1]), ring[0], ring[2] if len(ring) > 2 else 0, 0)
        verts.extend((int(y), int(x)) for y, x in ring[1])
    return recs, np.array(verts, np.int32).reshape(-1, 2)
