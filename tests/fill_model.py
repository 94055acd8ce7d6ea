"""A plain model of the terrain depressions, written from the definition: a priority-flood from the
outlets for the fill (the kernels relax tiles to a fixed point instead), and a loop over the regions for the basin records.
Python integers throughout."""
import heapq

import numpy as np

NONE = 2 ** 31 - 1
ZMAX = 2 ** 30
BASIN = np.dtype([("weight", "<u8"), ("volume", "<u8"), ("count", "<u4"), ("level_min", "<i4"), ("level_max", "<i4"),
                  ("depth_max", "<i4"), ("deepest_at", "<i4"), ("pour_at", "<i4"), ("pour_level", "<i4"), ("reserved", "<u4")])

STEPS4 = ((-1, 0), (0, 1), (1, 0), (0, -1))
STEPS8 = STEPS4 + ((-1, 1), (1, 1), (1, -1), (-1, -1))


def neighbours(i, j, rows, cols, conn, wrap):
    """The lattice neighbours of (i, j): no edge crosses the first or the last row; wrap joins the last column to the first."""
    for di, dj in (STEPS8 if conn == 8 else STEPS4):
        a, b = i + di, j + dj
        if a < 0 or a >= rows:
            continue
        if b < 0 or b >= cols:
            if not wrap:
                continue
            b %= cols
        yield a, b


def outlets(rows, cols, wrap, edge_outlets, table=None):
    o = np.zeros((rows, cols), bool)
    if edge_outlets:
        o[0, :] = o[-1, :] = True
        if not wrap:
            o[:, 0] = o[:, -1] = True
    if table is not None:
        o |= np.asarray(table).reshape(rows, cols) != 0
    return o


def fill(z, conn=8, wrap=False, edge_outlets=True, table=None):
    """(rows, cols) int32: the least, over all paths to an outlet, of the greatest height on the path.  Nodes leave the heap
    in ascending fill, so the first time a node is reached its value is final."""
    z = np.asarray(z)
    rows, cols = z.shape
    zz = [[int(v) for v in row] for row in z]
    out = [[NONE] * cols for _ in range(rows)]
    heap = []
    for i, j in zip(*np.nonzero(outlets(rows, cols, wrap, edge_outlets, table))):
        out[i][j] = zz[i][j]
        heap.append((zz[i][j], int(i), int(j)))
    heapq.heapify(heap)
    done = [[False] * cols for _ in range(rows)]
    while heap:
        f, i, j = heapq.heappop(heap)
        if done[i][j]:
            continue
        done[i][j] = True
        for a, b in neighbours(i, j, rows, cols, conn, wrap):
            if done[a][b]:
                continue
            g = max(f, zz[a][b])
            if g < out[a][b]:
                out[a][b] = g
                heapq.heappush(heap, (g, a, b))
    return np.array(out, np.int64).astype(np.int32)


def depth(fill_, z):
    """fill - z held in 0 .. INT32_MAX (the fill of a lattice without outlets is INT32_MAX)."""
    return [[min(max(int(f) - int(h), 0), 2 ** 31 - 1) for f, h in zip(fr, zr)] for fr, zr in zip(np.asarray(fill_), np.asarray(z))]


def basins(labels, n_regions, z, fill_, conn=8, wrap=False, row_weight=None):
    """(n_regions,) BASIN: one region after the other."""
    labels = np.asarray(labels)
    rows, cols = labels.shape
    d = depth(fill_, z)
    fl = np.asarray(fill_).tolist()
    lab = labels.tolist()
    out = np.zeros(n_regions, BASIN)
    flat = labels.reshape(-1)
    order = np.argsort(flat, kind="stable")             # a region's nodes in ascending index, one region after the other
    for r in range(n_regions):
        weight = volume = count = 0
        lmin, lmax, dmax, deepest = 2 ** 31 - 1, -2 ** 31, 0, -1
        pour = None
        for v in order[np.searchsorted(flat, r, "left", order):np.searchsorted(flat, r, "right", order)].tolist():
            i, j = divmod(v, cols)
            w = 1 if row_weight is None else int(row_weight[i])
            f = fl[i][j]
            weight += w
            volume += w * d[i][j]
            count += 1
            lmin, lmax = min(lmin, f), max(lmax, f)
            if deepest < 0 or d[i][j] > dmax:
                dmax, deepest = d[i][j], v
            for a, b in neighbours(i, j, rows, cols, conn, wrap):
                if lab[a][b] != r:
                    key = (fl[a][b], a * cols + b)
                    pour = key if pour is None or key < pour else pour
        out[r] = (weight % 2 ** 64, volume % 2 ** 64, count, lmin, lmax, dmax, deepest, -1 if pour is None else pour[1],
                  2 ** 31 - 1 if pour is None else pour[0], 0)
    return out
