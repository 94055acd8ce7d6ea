"""What the host and the GPU tests of mrtx_rasterise share: the raw call, the list of refusals and the built polygons."""
import ctypes as C
import math

import numpy as np

from moonrtx_amd import _lib
from moonrtx_amd import regions as rg


def block(rows=8, cols=9, wrap=0, s=0, rule=0, order=0, reserved=0):
    return _lib.MrtxRaster(rows, cols, wrap, s, rule, order, reserved)


def raster_call(lib, ctx, r, rings=None, dev_rings=None, n_rings=None, vertices=None, dev_vertices=None, n_vertices=None,
                n_polygons=1, weights=None, labels=None, dev_labels=None, cover=None, dev_cover=None, crossings=None, block=True,
                st=None):
    """mrtx_rasterise with numpy arrays for the host tables and integers for the device tables."""
    ptr = lambda a: None if a is None else a.ctypes.data
    n_rings = (len(rings) if rings is not None else 0) if n_rings is None else n_rings
    n_vertices = (len(vertices) if vertices is not None else 0) if n_vertices is None else n_vertices
    return lib.mrtx_rasterise(ctx, C.byref(r) if block else None, dev_rings, ptr(rings), n_rings, dev_vertices, ptr(vertices),
                              n_vertices, n_polygons, ptr(weights), dev_labels, ptr(labels), dev_cover, ptr(cover),
                              C.byref(crossings) if crossings is not None else None, C.byref(st) if st is not None else None)


def refusal_tables():
    """(rings (2,), vertices (8, 2), labels (8, 9), cover (1,)): the host tables of the refusal cases; the outputs zeroed."""
    rings = np.zeros(2, rg.RASTER_RING_DTYPE)
    rings["first"], rings["n_vertices"] = (0, 4), 4
    vertices = np.array([[1, 1], [1, 5], [5, 5], [5, 1], [2, 2], [2, 3], [3, 3], [3, 2]], np.int32)
    return rings, vertices, np.zeros((8, 9), np.int32), np.zeros(1, rg.COVER_DTYPE)


def refusal_cases(rings, vertices, labels, cover, dev):
    """[(a pattern of the refusal's text, keyword arguments of raster_call)]; dev: the address of 8192 bytes of device memory, or
    any 16-byte aligned number where no device is present: no case gets as far as reading it."""
    F = dict(rings=rings, vertices=vertices, labels=labels, cover=cover)
    D = dict(dev_rings=dev, n_rings=2, dev_vertices=dev + 64, n_vertices=8, dev_labels=dev + 512, dev_cover=dev + 1024)
    return [
        ("null raster block", dict(F, r=block(), block=False)),
        ("reserved must be 0", dict(F, r=block(reserved=1))),
        ("empty lattice", dict(F, r=block(rows=0))),
        ("empty lattice", dict(F, r=block(cols=-3))),
        ("at most 2\\^31 nodes", dict(F, r=block(rows=65536, cols=32769))),
        ("at most 2\\^28 nodes", dict(F, r=block(rows=16384, cols=16385))),
        ("wrap must be 0 or 1", dict(F, r=block(wrap=2))),
        ("cols >= 3", dict(F, r=block(cols=2, wrap=1))),
        ("subcell_bits must lie in 0 .. 8", dict(F, r=block(s=-1))),
        ("subcell_bits must lie in 0 .. 8", dict(F, r=block(s=9))),
        ("rule must be MRTX_RASTER_NONZERO or MRTX_RASTER_EVENODD", dict(F, r=block(rule=2))),
        ("order must be MRTX_RASTER_FIRST or MRTX_RASTER_LAST", dict(F, r=block(order=-1))),
        ("exactly one of dev_rings and host_rings", dict(F, r=block(), rings=None, n_rings=2)),
        ("exactly one of dev_rings and host_rings", dict(F, r=block(), dev_rings=dev)),
        ("at most one of dev_rings and host_rings", dict(F, r=block(), dev_rings=dev, n_rings=0)),
        ("exactly one of dev_vertices and host_vertices", dict(F, r=block(), vertices=None, n_vertices=8)),
        ("exactly one of dev_vertices and host_vertices", dict(F, r=block(), dev_vertices=dev)),
        ("at most one of dev_vertices and host_vertices", dict(F, r=block(), dev_vertices=dev, n_vertices=0)),
        ("fewer than 2\\^31 rings and vertices", dict(F, r=block(), n_rings=2 ** 31)),
        ("fewer than 2\\^31 rings and vertices", dict(F, r=block(), n_vertices=2 ** 40)),
        ("exactly one of dev_labels and host_labels", dict(F, r=block(), labels=None)),
        ("exactly one of dev_labels and host_labels", dict(F, r=block(), dev_labels=dev)),
        ("exactly one of dev_cover and host_cover", dict(F, r=block(), cover=None)),
        ("exactly one of dev_cover and host_cover", dict(F, r=block(), dev_cover=dev)),
        ("at most one of dev_cover and host_cover", dict(F, r=block(), dev_cover=dev, n_polygons=0)),
        ("at most 2\\^28 bins", dict(F, r=block(rows=1, cols=6401), n_polygons=2 ** 28 // 101 + 1)),
        ("dev_rings must be 8-byte aligned", dict(D, r=block(), dev_rings=dev + 4)),
        ("dev_vertices must be 4-byte aligned", dict(D, r=block(), dev_vertices=dev + 66)),
        ("dev_labels must be 4-byte aligned", dict(D, r=block(), dev_labels=dev + 514)),
        ("dev_cover must be 8-byte aligned", dict(D, r=block(), dev_cover=dev + 1028)),
        ("must not overlap", dict(D, r=block(), dev_labels=dev + 40)),              # the labels on the rings
        ("must not overlap", dict(D, r=block(), dev_labels=dev + 64 + 60)),         # ... on the vertices
        ("must not overlap", dict(D, r=block(), dev_cover=dev + 512 + 280)),        # the cover records on the labels
        ("must not overlap", dict(D, r=block(), dev_cover=dev + 16)),               # ... on the rings
    ]


def assert_refused(lib, ctx, text, kw, labels, cover):
    """One refusal: the code, the text, the count and the statistics as they were, the host outputs untouched."""
    import re
    kw = dict(kw)
    crossings = C.c_uint64(5)
    st = _lib.MrtxStats()
    st.launches, st.kernel_ms = 0xABCD, -7.0
    assert raster_call(lib, ctx, crossings=crossings, st=st, **kw) == -1, text
    msg = lib.mrtx_last_error(ctx).decode()
    assert re.search(text, msg), (text, msg)
    assert crossings.value == 5 and st.launches == 0xABCD and st.kernel_ms == -7.0, text
    assert (labels == 0).all() and (cover.view(np.uint8) == 0).all(), text


# ---- the built polygons: name -> (rings [(polygon, [(y, x) ...][, wind])], n_polygons, rows, cols, wrap, subcell_bits)
def _rect(y0, x0, y1, x1, u=1):
    """Clockwise on the screen (rows run down): the interior on the right, as an outline's outer ring."""
    return [(y0 * u, x0 * u), (y0 * u, x1 * u), (y1 * u, x1 * u), (y1 * u, x0 * u)]


def _mirror(points, cols, u):
    return [(y, cols * u - x) for y, x in points]


def geometry_cases():
    out = {}
    # two triangles sharing the diagonal through the node centres (i + 1/2, i + 1/2): every node belongs to exactly one
    u = 2
    out["two_triangles"] = ([(0, [(0, 0), (0, 8 * u), (8 * u, 8 * u)]), (1, [(0, 0), (8 * u, 8 * u), (8 * u, 0)])], 2, 8, 8, False, 1)
    # a diamond with its four vertices on the centres of nodes (0, 3), (3, 6), (6, 3), (3, 0)
    out["vertex_on_a_centre"] = ([(0, [(1, 7), (7, 13), (13, 7), (7, 1)])], 1, 7, 7, False, 1)
    # horizontal and vertical edges through node centres: from the centre of (0, 0) to that of (5, 6)
    out["edges_through_centres"] = ([(0, [(2, 2), (2, 26), (22, 26), (22, 2)])], 1, 7, 8, False, 2)
    # a pentagram: its inner pentagon has winding 2, covered under NONZERO and not under EVENODD
    u = 8
    star = [(round((10 - 9.3 * math.cos(2 * math.pi * k / 5)) * u), round((10 + 9.3 * math.sin(2 * math.pi * k / 5)) * u)) for k in (0, 2, 4, 1, 3)]
    out["pentagram"] = ([(0, star)], 1, 20, 20, False, 3)
    # rings that cover nothing: there and back, and one vertex; and polygon 2, which has no ring
    out["zero_area_and_one_vertex"] = ([(0, [(5, 3), (37, 81)]), (1, [(33, 33)]), (3, [(8, 8), (8, 40), (40, 40), (40, 8)])], 4, 12, 12, False, 2)
    # partly outside (every side of the lattice), wholly outside, and larger than the lattice
    u = 16
    out["outside"] = ([(0, _rect(-3, -2, 4, 5, u)), (1, _rect(7, 8, 14, 30, u)), (2, _rect(-9, 3, -2, 7, u)), (3, _rect(3, 14, 6, 20, u)),
                       (4, _rect(12, 2, 15, 5, u)), (5, [(-40 * u, 6 * u), (5 * u + 3, 60 * u), (50 * u, 6 * u + 5), (5 * u, -50 * u)])],
                      6, 10, 12, False, 4)
    out["larger_than_the_lattice"] = ([(0, _rect(-100, -100, 100, 100, 256))], 1, 9, 11, False, 8)
    # overlapping polygons: FIRST against LAST, owned against count; an anticlockwise one among them
    u = 32
    out["overlapping"] = ([(0, _rect(1, 1, 9, 9, u)), (1, _rect(4, 4, 12, 14, u)), (2, _rect(5, 5, 7, 7, u)[::-1]),
                           (1, _rect(5, 6, 8, 8, u)[::-1]), (3, [(2 * u + 5, 10 * u), (11 * u, 15 * u + 7), (13 * u, 2 * u + 1)])], 4, 14, 16, False, 5)
    # the same oblique shapes at every sub-cell resolution: the two triangles and the pentagram side by side, a quarter of a
    # unit off the cell corners where s allows it
    for s in range(1, 9):
        u, off = 2 ** s, 2 ** s // 4
        star = [(round((10 - 9.3 * math.cos(2 * math.pi * k / 5)) * u) + off, round((19 + 9.3 * math.sin(2 * math.pi * k / 5)) * u) - off)
                for k in (0, 2, 4, 1, 3)]
        out[f"oblique_s{s}"] = ([(0, [(0, 0), (0, 8 * u), (8 * u, 8 * u)]), (1, [(0, 0), (8 * u, 8 * u), (8 * u, 0)]), (2, star)], 3, 20, 30, False, s)
    # ---- layout edges
    for cols in (63, 64, 65, 129):
        u = 4
        out[f"width_{cols}"] = ([(0, [(u, 0), (3 * u, cols * u), (19 * u, cols * u - 3), (20 * u, 2)]), (1, _rect(5, cols - 7, 25, cols + 9, u))],
                                2, 22, cols, False, 2)
    out["edge_on_a_strip_boundary"] = ([(0, _rect(2, 64, 9, 128, 2)), (1, _rect(1, 60, 5, 64, 2)), (2, _rect(6, 127, 11, 129, 2))], 3, 12, 130, False, 1)
    # across the seam with negative x and with x > cols; and a one-vertex ring all the way round
    u = 2
    out["across_the_seam"] = ([(0, _rect(1, -5, 6, 5, u)), (1, _rect(8, 65, 12, 77, u)), (2, [(14 * u, 3 * u)], 1), (2, [(15 * u, 9 * u)], -1),
                               (3, [(2 * u + 1, -30 * u), (9 * u, -68 * u + 1), (5 * u, -75 * u)])], 4, 17, 70, True, 1)
    # an edge three and a half times as long as the window is wide: it hits every column three or four times
    u = 4
    out["edge_longer_than_cols"] = ([(0, [(0, 0), (9 * u, 35 * u), (9 * u + 2, 0)]), (1, [(2 * u, -21 * u - 1), (7 * u, 46 * u + 3), (8 * u, 5 * u)])],
                                    2, 11, 10, True, 2)
    # a comb: forty bars of one polygon inside one strip, 120 crossings each, far more than one LDS chunk holds
    out["comb"] = ([(0, _rect(2 * k, 1, 2 * k + 1, 61)) for k in range(40)] + [(1, _rect(0, 30, 80, 90))], 2, 80, 100, False, 0)
    # seventy polygons on 33 strips: more bins than one chunk of the scan
    u = 2
    out["many_bins"] = ([(p, _rect(p % 7 * 5, 30 * p, p % 7 * 5 + 4 + p % 3, 30 * p + 45, u)) for p in range(70)], 70, 40, 2100, False, 1)
    # rings whose crossings all clip to row 0: one above the lattice, one that reaches into it
    out["clipped_to_row_0"] = ([(0, _rect(-9, 1, -2, 8, 8)), (1, [(-70, 10), (-3, 90), (-1, 20)]), (2, _rect(-4, 10, 3, 14, 8))], 3, 6, 16, False, 3)
    return out


def mirrored(case):
    rings, n, rows, cols, wrap, s = case
    return [(r[0], _mirror(r[1], cols, 2 ** s)) + ((-r[2],) if len(r) > 2 else ()) for r in rings], n, rows, cols, wrap, s


GEOMETRY = ["two_triangles", "vertex_on_a_centre", "edges_through_centres", "pentagram", "zero_area_and_one_vertex", "outside",
            "larger_than_the_lattice", "overlapping", "oblique_s1", "oblique_s2", "oblique_s3", "oblique_s4", "oblique_s5", "oblique_s6",
            "oblique_s7", "oblique_s8", "width_63", "width_64", "width_65", "width_129", "edge_on_a_strip_boundary",
            "across_the_seam", "edge_longer_than_cols", "comb", "many_bins", "clipped_to_row_0"]


def weights_for(rows):
    """distinct per row and near 2^32, so that the weights need 64 bits"""
    return (2 ** 32 - 1 - 3 * np.arange(rows)).astype(np.uint32)
