"""A plain numpy model of the proximity maps and the reach of labelled regions: brute force over every
(node, feature) pair in int64, and a loop over the regions.  The feature axis ascends in node index and numpy's argmin returns
the first minimum, which is the tie rule: the least node index among the features at the least distance."""
import numpy as np

COORD_MAX = 2 ** 29
D2_MAX = 3 * 2 ** 60
assert D2_MAX <= np.iinfo(np.int64).max          # every d2 fits int64
NONE = np.uint64(2 ** 64 - 1)

REACH = np.dtype([("d2_max", "<u8"), ("d2_min", "<u8"), ("max_at", "<i4"), ("min_at", "<i4"), ("min_nearest", "<i4"),
                  ("count", "<u4")])


def proximity(labels, positions, outside=False, chunk=512):
    """(nearest (rows, cols) int32, dist2 (rows, cols) uint64) of labels (rows, cols) and positions (rows, cols, 3)."""
    lab = np.asarray(labels)
    rows, cols = lab.shape
    pos = np.asarray(positions).astype(np.int64).reshape(rows * cols, 3)
    assert np.abs(pos).max(initial=0) <= COORD_MAX
    flat = lab.reshape(-1)
    feat = np.flatnonzero(flat < 0 if outside else flat >= 0)      # ascending node index
    nearest = np.full(rows * cols, -1, np.int32)
    dist2 = np.full(rows * cols, NONE, np.uint64)
    if feat.size:
        fp = pos[feat]
        for a in range(0, rows * cols, chunk):
            d = pos[a:a + chunk, None, :] - fp[None, :, :]
            d2 = (d * d).sum(-1)                                    # int64, at most 3 x 2^60
            k = np.argmin(d2, axis=1)                               # the first of equal minima
            nearest[a:a + chunk] = feat[k]
            dist2[a:a + chunk] = d2[np.arange(d2.shape[0]), k].astype(np.uint64)
    return nearest.reshape(rows, cols), dist2.reshape(rows, cols)


def reach(labels, n_regions, dist2, nearest):
    """(n_regions,) REACH records of a dist2 / nearest pair over a label table, region by region."""
    flat = np.asarray(labels).reshape(-1)
    d2 = np.asarray(dist2, np.uint64).reshape(-1)
    near = np.asarray(nearest, np.int32).reshape(-1)
    out = np.zeros(n_regions, REACH)
    for r in range(n_regions):
        nodes = np.flatnonzero(flat == r)
        rec = out[r]
        rec["count"] = nodes.size
        if nodes.size == 0:
            rec["d2_max"], rec["d2_min"], rec["max_at"], rec["min_at"], rec["min_nearest"] = 0, NONE, -1, -1, -1
            continue
        vals = [int(v) for v in d2[nodes]]
        hi, lo = max(vals), min(vals)
        rec["d2_max"], rec["d2_min"] = hi, lo
        rec["max_at"] = nodes[vals.index(hi)]                      # nodes ascend: the least index among equals
        rec["min_at"] = nodes[vals.index(lo)]
        rec["min_nearest"] = near[rec["min_at"]]
    return out
