"""An independent model of the region outlines, straight from the definitions: a plain Python tracer
that loops over the nodes in index order and follows successors with a visited set.  Records and vertices are built with
Python integers.  It shares no code with the package.

Cell corners of node (i, j): NW (i, j), NE (i, j + 1), SE (i + 1, j + 1), SW (i + 1, j).  Side k of node v has the id 4 v + k and
the region on its right: 0 north NW -> NE, 1 east NE -> SE, 2 south SE -> SW, 3 west SW -> NW."""
import numpy as np

RING = np.dtype([("area", "<i8"), ("warea", "<i8"), ("first", "<u8"), ("n_sides", "<u4"), ("n_vertices", "<u4"),
                 ("label", "<i4"), ("head", "<i4"), ("wind", "<i4"), ("reserved", "<u4")])
ALL, CORNERS = 0, 1

T = ((0, 1), (1, 0), (0, -1), (-1, 0))      # travel direction of side k
D = ((-1, 0), (0, 1), (1, 0), (0, -1))      # outward direction of side k
START = ((0, 0), (0, 1), (1, 1), (1, 0))    # the start corner of side k, from the node's NW corner


def trace(labels, connectivity=4, wrap=False, mode=CORNERS, row_weight=None):
    """(rings (n,) RING, vertices (m, 2) int32) of a (rows, cols) label table; labels < 0 carry no region."""
    assert connectivity in (4, 8) and mode in (ALL, CORNERS)
    lab = np.asarray(labels).astype(np.int64)
    rows, cols = lab.shape
    assert not wrap or cols >= 3
    L = lab.tolist()
    cw = [0]
    for i in range(rows):
        cw.append(cw[-1] + (1 if row_weight is None else int(row_weight[i])))

    def node(i, j):
        """(i, j) with the column wrapped, or None outside the lattice."""
        if i < 0 or i >= rows:
            return None
        if j < 0 or j >= cols:
            if not wrap:
                return None
            j %= cols
        return i, j

    def carries(p, l):
        return p is not None and L[p[0]][p[1]] == l

    def boundary(i, j, k):
        l = L[i][j]
        return l >= 0 and not carries(node(i + D[k][0], j + D[k][1]), l)

    def successor(i, j, k):
        l = L[i][j]
        a = node(i + T[k][0], j + T[k][1])
        b = node(i + T[k][0] + D[k][0], j + T[k][1] + D[k][1])
        ca, cb = carries(a, l), carries(b, l)
        if ca and cb:
            return b[0], b[1], (k - 1) % 4
        if ca:
            return a[0], a[1], k
        if cb and connectivity == 8:
            return b[0], b[1], (k - 1) % 4
        return i, j, (k + 1) % 4

    seen = set()
    recs, verts = [], []
    for v in range(rows * cols):
        for k in range(4):
            i, j = divmod(v, cols)
            if not boundary(i, j, k) or (i, j, k) in seen:
                continue
            # a new ring, met at its least side id: walk it once
            sides = []
            s = (i, j, k)
            while s not in seen:
                seen.add(s)
                assert boundary(*s), "the successor of a boundary side is a boundary side"
                sides.append(s)
                s = successor(*s)
            assert s == (i, j, k), "the successor map is a permutation: the walk closes at its head"
            n = len(sides)
            area = warea = north = south = 0
            for (a, b, c) in sides:
                if c == 0:
                    area -= a
                    warea -= cw[a]
                    north += 1
                elif c == 2:
                    area += a + 1
                    warea += cw[a + 1]
                    south += 1
            assert (north - south) % cols == 0
            x = j + START[k][1]
            ring_v = []
            for p, (a, b, c) in enumerate(sides):
                turned = c != sides[p - 1][2]
                if mode == ALL or turned:
                    ring_v.append((a + START[c][0], x))
                x += T[c][1]
            if not ring_v:
                ring_v.append((i + START[k][0], j + START[k][1]))
            recs.append((area, warea, len(verts), n, len(ring_v), L[i][j], 4 * v + k, (north - south) // cols, 0))
            verts.extend(ring_v)
    rings = np.array(recs, RING) if recs else np.zeros(0, RING)
    vertices = np.array(verts, np.int32).reshape(-1, 2)
    return rings, vertices
