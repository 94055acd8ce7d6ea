"""Terrain relief on the CPU, TEST INFRASTRUCTURE: the float64 left folds of the plane fit in numpy,
vectorised over the nodes and looping over the footprint only, in exactly the spec's operation order; and the safe share of a
landing ellipse from integer counts.  The metric scales come from the library's host helper mrtx_relief_scales, as the
kernel's do."""
import ctypes as C

import numpy as np

from moonrtx_amd import _lib


def make_window(row0, col0, rows, cols, stride=1, ri=1, rj=1, radius_m=1737400.0):
    return _lib.MrtxRelief(row0, col0, rows, cols, stride, ri, rj, 0, radius_m)


def scales(t, dem_shape):
    """(rows, 2) float64 (kx, ky) from mrtx_relief_scales; raises on a refused window."""
    lib = _lib.load()
    out = np.empty((t.rows, 2), np.float64)
    rc = lib.mrtx_relief_scales(C.byref(t), int(dem_shape[0]), int(dem_shape[1]), out.ctypes.data)
    if rc != 0:
        raise ValueError(f"mrtx_relief_scales refused the window ({rc})")
    return out


def q_sum(r):
    """sum of d^2 over d = -r .. r, an exact integer"""
    return r * (r + 1) * (2 * r + 1) // 3


def relief(dem, t, k=None):
    """(rows, cols, 4) float32 (grade, rms_m, ge, gn) of an MrtxRelief window over `dem`; k: the (rows, 2) scales (default:
    from the library for dem's shape)."""
    dem = np.asarray(dem, np.float32)
    return _relief(dem, t, scales(t, dem.shape) if k is None else k, 0, dem.shape[0])


def relief_crop(crop, crop_row0, full_shape, t):
    """As relief() for a window of a (H, W) DEM of which only the rows from crop_row0 on are at hand (all W columns)."""
    return _relief(np.asarray(crop, np.float32), t, scales(t, full_shape), crop_row0, full_shape[0])


def _relief(dem, t, k, crop_row0, H):
    W = dem.shape[1]
    ri, rj, s = t.ri, t.rj, t.stride
    rows_idx = t.row0 + np.arange(t.rows) * s                         # DEM rows of the window's rows
    valid = (rows_idx - ri * s >= 0) & (rows_idx + ri * s < H)
    cols_idx = t.col0 + np.arange(t.cols) * s
    n = (2 * ri + 1) * (2 * rj + 1)
    inv_n = 1.0 / n
    inv_xj = 1.0 / ((2 * ri + 1) * q_sum(rj))
    inv_xi = 1.0 / ((2 * rj + 1) * q_sum(ri))
    # the row pass once per lattice row the window's footprints touch (rows outside the DEM read a clipped row: only NaN
    # nodes use them), then the column pass on slices of it: the same folds, node for node
    lat_rows = t.row0 + np.arange(-ri, t.rows + ri) * s - crop_row0
    rr = np.clip(lat_rows, 0, dem.shape[0] - 1)
    r0 = r1 = r2 = None
    for dj in range(-rj, rj + 1):
        cc = (cols_idx + dj * s) % W
        z = dem[np.ix_(rr, cc)].astype(np.float64) - 1.0
        if r0 is None:
            r0, r1, r2 = z, float(dj) * z, z * z
        else:
            r0 = r0 + z
            r1 = r1 + float(dj) * z
            r2 = r2 + z * z
    S0 = Sj = Si = S2 = None
    for di in range(-ri, ri + 1):
        sl = slice(di + ri, di + ri + t.rows)
        if S0 is None:
            S0, Sj, Si, S2 = r0[sl], r1[sl], float(di) * r0[sl], r2[sl]
        else:
            S0 = S0 + r0[sl]
            Sj = Sj + r1[sl]
            Si = Si + float(di) * r0[sl]
            S2 = S2 + r2[sl]
    c = S0 * inv_n
    aj = Sj * inv_xj
    ai = Si * inv_xi
    E = np.fmax(((S2 - c * S0) - aj * Sj) - ai * Si, 0.0)
    ge = aj * k[:, 0:1]
    gn = -(ai * k[:, 1:2])
    out = np.empty((t.rows, t.cols, 4), np.float32)
    out[..., 0] = np.sqrt((ge * ge + gn * gn).astype(np.float32))
    out[..., 1] = np.sqrt((E * inv_n).astype(np.float32)) * np.float32(t.radius_m)
    out[..., 2] = ge.astype(np.float32)
    out[..., 3] = gn.astype(np.float32)
    out[~valid] = np.nan
    return out


def fetches(t, dem_h):
    """The texels the definition reads: (2 ri + 1)(2 rj + 1) per node that is not NaN."""
    rows_idx = t.row0 + np.arange(t.rows) * t.stride
    valid = (rows_idx - t.ri * t.stride >= 0) & (rows_idx + t.ri * t.stride < dem_h)
    return int(valid.sum()) * t.cols * (2 * t.ri + 1) * (2 * t.rj + 1)


def safe_mask(table, grade_max, rms_max):
    """The predicate of the share, thresholds compared as float32; NaN is unsafe."""
    with np.errstate(invalid="ignore"):
        return (table[..., 0] <= np.float32(grade_max)) & (table[..., 1] <= np.float32(rms_max))


def share(table, Ri, Rj, wrap, grade_max, rms_max):
    """(rows, cols) float32 (float)safe / (float)total from integer counts: separable sums of shifted copies."""
    ok = safe_mask(np.asarray(table, np.float32), grade_max, rms_max).astype(np.int64)
    rows, cols = ok.shape

    def box(a):
        # along the columns
        if wrap and 2 * Rj + 1 >= cols:
            h = np.repeat(a.sum(1, keepdims=True), cols, 1)
        else:
            c = np.concatenate([np.zeros((rows, 1), np.int64), np.cumsum(a, 1)], 1)
            if wrap:
                c = np.concatenate([c, c[:, 1:] + c[:, -1:]], 1)           # two laps of the circle
                j = np.arange(cols)
                lo, hi = j - Rj, j + Rj + 1
                shift = np.where(lo < 0, cols, 0)
                h = c[:, hi + shift] - c[:, lo + shift]
            else:
                j = np.arange(cols)
                h = c[:, np.minimum(j + Rj + 1, cols)] - c[:, np.maximum(j - Rj, 0)]
        # down the rows
        r = np.concatenate([np.zeros((1, cols), np.int64), np.cumsum(h, 0)], 0)
        i = np.arange(rows)
        return r[np.minimum(i + Ri + 1, rows)] - r[np.maximum(i - Ri, 0)]

    safe, total = box(ok), box(np.ones_like(ok))
    return safe.astype(np.float32) / total.astype(np.float32)


def share_brute(table, Ri, Rj, wrap, grade_max, rms_max):
    """The same by counting the distinct nodes of every box one by one (small maps only)."""
    ok = safe_mask(np.asarray(table, np.float32), grade_max, rms_max)
    rows, cols = ok.shape
    out = np.empty((rows, cols), np.float32)
    for i in range(rows):
        for j in range(cols):
            nodes = set()
            for di in range(-Ri, Ri + 1):
                for dj in range(-Rj, Rj + 1):
                    a, b = i + di, j + dj
                    if wrap:
                        b %= cols
                    if 0 <= a < rows and 0 <= b < cols:
                        nodes.add((a, b))
            safe = sum(1 for n in nodes if ok[n])
            out[i, j] = np.float32(safe) / np.float32(len(nodes))
    return out
