"""An independent model of the regions stage, straight from its definitions: a plain union-find over
the lattice's edges in Python / numpy.  It shares no code with the package.

Lattice rows x cols, node index i cols + j; wrap joins column cols - 1 to column 0; connectivity 4 or 8; no edge crosses the
first or the last row.  A region is a connected component of the set, its root its least node index, regions numbered in
ascending order of root.  The catalogue is all integers."""
import numpy as np

RECORD = np.dtype([("weight", "<u8"), ("sum_i", "<i8"), ("sum_dj", "<i8"), ("count", "<u4"), ("root_i", "<i4"),
                   ("root_j", "<i4"), ("i_min", "<i4"), ("i_max", "<i4"), ("dj_min", "<i4"), ("dj_max", "<i4"),
                   ("reserved", "<u4")])


def predicate(field, ch, lo, hi):
    """(rows, cols) bool: x >= (float)lo && x <= (float)hi for x = field[..., ch] as float32; NaN is out."""
    x = np.asarray(field, np.float32)
    x = x[..., ch] if x.ndim == 3 else x
    with np.errstate(invalid="ignore"):
        return (x >= np.float32(lo)) & (x <= np.float32(hi))


def edges(mask, connectivity, wrap):
    """(E, 2) int64 node indices of the lattice edges whose two ends are both in the set."""
    mask = np.asarray(mask) != 0
    rows, cols = mask.shape
    idx = np.arange(rows * cols, dtype=np.int64).reshape(rows, cols)
    steps = [(0, 1), (1, 0)] if connectivity == 4 else [(0, 1), (1, 0), (1, 1), (1, -1)]
    out = []
    for di, dj in steps:
        for i in range(rows - di):
            j = np.arange(cols)
            nj = j + dj
            if wrap and cols >= 3:
                nj = nj % cols
                ok = np.ones(cols, bool)
            else:
                ok = (nj >= 0) & (nj < cols)
            a, b = idx[i, j[ok]], idx[i + di, nj[ok]]
            both = mask.reshape(-1)[a] & mask.reshape(-1)[b]
            out.append(np.stack([a[both], b[both]], -1))
    return np.concatenate(out) if out else np.zeros((0, 2), np.int64)


def label(mask, connectivity=4, wrap=False):
    """(labels (rows, cols) int32, K)."""
    assert connectivity in (4, 8)
    mask = np.asarray(mask) != 0
    rows, cols = mask.shape
    parent = list(range(rows * cols))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in edges(mask, connectivity, wrap).tolist():
        ra, rb = find(a), find(b)
        if ra < rb:
            parent[rb] = ra
        elif rb < ra:
            parent[ra] = rb
    flat = mask.reshape(-1)
    root = np.array([find(v) if flat[v] else -1 for v in range(rows * cols)], np.int64)
    roots = np.unique(root[root >= 0])              # ascending: the numbering
    labels = np.full(rows * cols, -1, np.int32)
    labels[root >= 0] = np.searchsorted(roots, root[root >= 0]).astype(np.int32)
    return labels.reshape(rows, cols), int(roots.size)


def catalogue(labels, n, wrap=False, row_weight=None):
    """(n,) RECORD of a label table; a number that no node carries gives count 0, root (-1, -1), extents 0."""
    labels = np.asarray(labels, np.int64)
    rows, cols = labels.shape
    # per region: weight, sum_i, sum_dj, count, root_i, root_j, i_min, i_max, dj_min, dj_max as Python integers
    recs = [[0, 0, 0, 0, -1, -1, 0, 0, 0, 0] for _ in range(n)]
    rowsl = labels.tolist()
    for i in range(rows):
        w = 1 if row_weight is None else int(row_weight[i])
        for j, l in enumerate(rowsl[i]):
            if l < 0:
                continue
            r = recs[l]
            if r[3] == 0:                           # row-major order: the first node met is the root
                r[4], r[5] = i, j
                dj = 0
                r[6] = r[7] = i
            else:
                dj = j - r[5]
                if wrap:
                    dj = ((dj + cols // 2) % cols) - cols // 2
                r[6], r[7] = min(r[6], i), max(r[7], i)
                r[8], r[9] = min(r[8], dj), max(r[9], dj)
            r[0] += w
            r[1] += i
            r[2] += dj
            r[3] += 1
    t = np.zeros(n, RECORD)
    for k, name in enumerate(RECORD.names[:10]):
        t[name] = [r[k] for r in recs]
    return t
