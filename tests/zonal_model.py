"""An independent model of the zonal statistics and outlines of labelled regions: plain Python and
numpy, nothing shared with the package.  Sums are Python integers per node, folded to 64 bits at the end; the fixed point is
np.rint(float64(x) * scale); the extremes are taken by the total-order key of the float32 bits; the perimeter comes from
neighbour comparison and the bit quads from every 2 x 2 window in turn.  Two further routes to a region's topology: the holes
counted as components of its complement in the dual connectivity on a padded lattice, and the Euler number as V - E + F."""
import numpy as np

ZONAL = np.dtype([("wcount", "<u8"), ("wsum", "<i8"), ("sum", "<i8"), ("count", "<u4"), ("n_nan", "<u4"), ("n_clipped", "<u4"),
                  ("min", "<f4"), ("max", "<f4"), ("min_at", "<i4"), ("max_at", "<i4"), ("reserved", "<u4")])
SHAPE = np.dtype([("perimeter", "<u8"), ("sides_ns", "<u4"), ("sides_ew", "<u4"), ("q1", "<u4"), ("q3", "<u4"), ("qd", "<u4"),
                  ("euler", "<i4")])


def order_key(x):
    """The uint32 key of float32 values whose unsigned order is the total order of the bit patterns (-0.0 before +0.0)."""
    b = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return np.where(b & 0x80000000, (~b) & 0xFFFFFFFF, b | 0x80000000).astype(np.uint64)


def fixed(x, scale):
    """(q as a list of Python ints, clipped as a bool array) of float32 values that are not NaN."""
    p = np.asarray(x, np.float32).astype(np.float64) * np.float64(scale)
    clipped = np.abs(p) >= 2.0 ** 31
    with np.errstate(invalid="ignore"):
        r = np.rint(np.where(clipped, 0.0, p))
    q = [(-2 ** 31 if pp < 0 else 2 ** 31) if c else int(v) for v, c, pp in zip(r.tolist(), clipped.tolist(), p.tolist())]
    return q, clipped


def _i64(v):
    v &= 2 ** 64 - 1
    return v - 2 ** 64 if v >= 2 ** 63 else v


def zonal(labels, n, field, scale, weights=None):
    """(n, n_ch) ZONAL records of field (rows, cols, n_ch) float32 over labels (rows, cols); entries outside 0 .. n - 1 are
    in no region."""
    labels = np.asarray(labels)
    rows, cols = labels.shape
    field = np.asarray(field, np.float32).reshape(rows, cols, -1)
    n_ch = field.shape[2]
    out = np.zeros((n, n_ch), ZONAL)
    out["min"], out["max"], out["min_at"], out["max_at"] = np.inf, -np.inf, -1, -1
    lab = labels.reshape(-1)
    w_node = np.repeat(np.ones(rows, np.uint64) if weights is None else np.asarray(weights, np.uint64), cols).tolist()
    for ch in range(n_ch):
        x = field[:, :, ch].reshape(-1)
        nan = np.isnan(x)
        key = order_key(x).tolist()
        q, clipped = fixed(np.where(nan, np.float32(0), x), scale)
        acc = [dict(wcount=0, wsum=0, sum=0, count=0, n_nan=0, n_clipped=0, kmin=None, kmax=None) for _ in range(n)]
        for node in np.flatnonzero((lab >= 0) & (lab < n)).tolist():
            a = acc[lab[node]]
            if nan[node]:
                a["n_nan"] += 1
                continue
            a["count"] += 1
            a["wcount"] += w_node[node]
            a["sum"] += q[node]
            a["wsum"] += w_node[node] * q[node]
            a["n_clipped"] += bool(clipped[node])
            if a["kmin"] is None or key[node] < a["kmin"][0]:          # strictly: the least index among equals stays
                a["kmin"] = (key[node], node)
            if a["kmax"] is None or key[node] > a["kmax"][0]:
                a["kmax"] = (key[node], node)
        for r, a in enumerate(acc):
            o = out[r, ch]
            o["wcount"], o["wsum"], o["sum"] = a["wcount"] % 2 ** 64, _i64(a["wsum"]), _i64(a["sum"])
            o["count"], o["n_nan"], o["n_clipped"] = a["count"], a["n_nan"], a["n_clipped"]
            if a["count"]:
                o["min"], o["min_at"] = x[a["kmin"][1]], a["kmin"][1]
                o["max"], o["max_at"] = x[a["kmax"][1]], a["kmax"][1]
    return out


def wsum_exact(labels, r, field_ch, scale, weights):
    """The unwrapped Python-integer sum of weight * q over region r."""
    labels = np.asarray(labels)
    x = np.asarray(field_ch, np.float32)
    sel = (labels == r) & ~np.isnan(x)
    q, _ = fixed(x[sel], scale)
    w = np.broadcast_to(np.asarray(weights, np.uint64)[:, None], labels.shape)[sel].tolist()
    return sum(a * b for a, b in zip(w, q))


def histogram(labels, n, field_ch, n_bins, lo, inv_w, weights=None):
    """(n, n_bins + 2) uint64: column 0 below, column n_bins + 1 at or above the top, t = (float64(x) - lo) * inv_w."""
    labels = np.asarray(labels)
    rows, cols = labels.shape
    x = np.asarray(field_ch, np.float32).reshape(rows, cols)
    t = (x.astype(np.float64) - np.float64(lo)) * np.float64(inv_w)
    out = [[0] * (n_bins + 2) for _ in range(n)]
    for i in range(rows):
        w = 1 if weights is None else int(weights[i])
        for j in range(cols):
            l = int(labels[i, j])
            if l < 0 or l >= n or np.isnan(x[i, j]):
                continue
            tt = t[i, j]
            col = 0 if tt < 0 else n_bins + 1 if tt >= n_bins else 1 + int(np.floor(tt))
            out[l][col] += w
    return np.array([[v % 2 ** 64 for v in row] for row in out], np.uint64).reshape(n, n_bins + 2)


def _at(labels, i, j, wrap):
    rows, cols = labels.shape
    if i < 0 or i >= rows:
        return -1
    if j < 0 or j >= cols:
        if not wrap:
            return -1
        j %= cols
    return int(labels[i, j])


def shape(labels, n, connectivity, wrap=False, side_ew=None, side_ns=None):
    """(n,) SHAPE records: boundary sides by neighbour comparison, bit quads window by window."""
    labels = np.asarray(labels)
    rows, cols = labels.shape
    acc = [dict(perimeter=0, sides_ns=0, sides_ew=0, q1=0, q3=0, qd=0) for _ in range(n)]
    ew = [1] * rows if side_ew is None else [int(v) for v in side_ew]
    ns = [1] * (rows + 1) if side_ns is None else [int(v) for v in side_ns]
    for i in range(rows):
        for j in range(cols):
            l = int(labels[i, j])
            if l < 0 or l >= n:
                continue
            a = acc[l]
            for di, dj, length, kind in ((-1, 0, ns[i], "sides_ns"), (1, 0, ns[i + 1], "sides_ns"), (0, -1, ew[i], "sides_ew"),
                                         (0, 1, ew[i], "sides_ew")):
                if _at(labels, i + di, j + dj, wrap) != l:
                    a[kind] += 1
                    a["perimeter"] += length
    for i in range(rows + 1):
        for j in range(cols if wrap else cols + 1):
            quad = (_at(labels, i - 1, j - 1, wrap), _at(labels, i - 1, j, wrap), _at(labels, i, j - 1, wrap), _at(labels, i, j, wrap))
            for l in set(quad):
                if l < 0 or l >= n:
                    continue
                pat = tuple(v == l for v in quad)
                k = sum(pat)
                if k == 1:
                    acc[l]["q1"] += 1
                elif k == 3:
                    acc[l]["q3"] += 1
                elif pat in ((True, False, False, True), (False, True, True, False)):
                    acc[l]["qd"] += 1
    out = np.zeros(n, SHAPE)
    for r, a in enumerate(acc):
        e4 = a["q1"] - a["q3"] + (2 if connectivity == 4 else -2) * a["qd"]
        assert e4 % 4 == 0, (r, a)
        out[r] = (a["perimeter"] % 2 ** 64, a["sides_ns"], a["sides_ew"], a["q1"], a["q3"], a["qd"], e4 // 4)
    return out


def _components(mask, connectivity, wrap=False):
    """The number of connected components of a boolean mask (a flood fill with an explicit stack)."""
    mask = np.asarray(mask, bool)
    rows, cols = mask.shape
    seen = np.zeros(mask.shape, bool)
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if connectivity == 8 else [])
    count = 0
    for i0, j0 in np.argwhere(mask).tolist():
        if seen[i0, j0]:
            continue
        count += 1
        seen[i0, j0] = True
        stack = [(i0, j0)]
        while stack:
            i, j = stack.pop()
            for di, dj in steps:
                a, b = i + di, j + dj
                if a < 0 or a >= rows:
                    continue
                if b < 0 or b >= cols:
                    if not wrap:
                        continue
                    b %= cols
                if mask[a, b] and not seen[a, b]:
                    seen[a, b] = True
                    stack.append((a, b))
    return count


def components(labels, r, connectivity, wrap=False):
    return _components(np.asarray(labels) == r, connectivity, wrap)


def holes(labels, r, connectivity):
    """The holes of region r of an unwrapped map: the components of its complement in the dual connectivity on a lattice
    padded by one node all round, less the one outside."""
    m = np.pad(np.asarray(labels) == r, 1)
    return _components(~m, 8 if connectivity == 4 else 4) - 1


def euler_vef(labels, r, connectivity, wrap=False):
    """V - E + F of region r.  4-connected: the nodes are vertices, adjacent pairs edges and full 2 x 2 blocks faces.
    8-connected: every node is a closed unit square; its distinct corners, sides and the squares themselves."""
    m = np.asarray(labels) == r
    rows, cols = m.shape
    wc = (lambda j: j % cols) if wrap else (lambda j: j)
    cells = np.argwhere(m).tolist()
    if connectivity == 4:
        def has(i, j):
            if i >= rows:
                return False
            if j >= cols:
                if not wrap:
                    return False
                j %= cols
            return bool(m[i, j])
        V = len(cells)
        E = sum(has(i, j + 1) for i, j in cells) + sum(has(i + 1, j) for i, j in cells)
        F = sum(has(i, j + 1) and has(i + 1, j) and has(i + 1, j + 1) for i, j in cells)
        return V - E + F
    corners, hor, ver = set(), set(), set()
    for i, j in cells:
        corners.update({(i, wc(j)), (i, wc(j + 1)), (i + 1, wc(j)), (i + 1, wc(j + 1))})
        hor.update({(i, j), (i + 1, j)})                    # the sides along row lines, named by their west corner
        ver.update({(i, wc(j)), (i, wc(j + 1))})            # the sides along column lines, named by their north corner
    return len(corners) - len(hor) - len(ver) + len(cells)
