"""The least-cost traverse on the CPU, TEST INFRASTRUCTURE: float32 edge weights vectorised in numpy in
exactly the spec's operation order, a heapq Dijkstra summing in float64, and the predecessor rule.  The lengths come from the
library's host helper mrtx_traverse_lengths, as the kernels' do."""
import ctypes as C
import heapq
import math

import numpy as np

from moonrtx_amd import _lib

DI = (-1, -1, 0, 1, 1, 1, 0, -1)      # N, NE, E, SE, S, SW, W, NW: the step from v to u
DJ = (0, 1, 1, 1, 0, -1, -1, -1)


def make_window(row0, col0, rows, cols, stride=1, wrap=0, radius_m=1737400.0, max_grade=math.tan(math.radians(20.0)),
                climb_cost=8.0, descent_cost=0.0):
    return _lib.MrtxTraverse(row0, col0, rows, cols, stride, wrap, radius_m, max_grade, climb_cost, descent_cost, 0)


def lengths(t, dem_shape):
    """(rows, 3) float32 (L_ew, L_ns, L_dg) from mrtx_traverse_lengths; raises on a refused window."""
    lib = _lib.load()
    out = np.empty((t.rows, 3), np.float32)
    rc = lib.mrtx_traverse_lengths(C.byref(t), int(dem_shape[0]), int(dem_shape[1]), out.ctypes.data)
    if rc != 0:
        raise ValueError(f"mrtx_traverse_lengths refused the window ({rc})")
    return out


def window_D(dem, t):
    """(rows, cols) float32 heights of the window's nodes: texels (row0 + i stride, (col0 + j stride) mod W)."""
    H, W = dem.shape
    r = t.row0 + np.arange(t.rows) * t.stride
    c = (t.col0 + np.arange(t.cols) * t.stride) % W
    return np.asarray(dem, np.float32)[np.ix_(r, c)]


def weights(D, P, L, t):
    """(8, rows, cols) float32: wt[k, i, j] = w(u -> v) for v = (i, j) and u = v + step k, +inf where u is no node or the
    edge is not driven.  float32 throughout, in the spec's order."""
    rows, cols = D.shape
    f32 = np.float32
    Rm, gmax, a_up, a_dn = f32(t.radius_m), f32(t.max_grade), f32(t.climb_cost), f32(t.descent_cost)
    out = np.full((8, rows, cols), np.inf, np.float32)
    ii, jj = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(8):
            ui, uj = ii + DI[k], jj + DJ[k]
            if t.wrap:
                uj = uj % cols
            ok = (ui >= 0) & (ui < rows) & (uj >= 0) & (uj < cols)
            vi, vj = ii[ok], jj[ok]
            ui, uj = ui[ok], uj[ok]
            if DI[k] == 0:
                Lk = L[vi, 0]
            else:
                Lk = L[np.minimum(vi, ui), 1 if DJ[k] == 0 else 2]
            Dv, Du = D[vi, vj], D[ui, uj]
            dh = (Dv - Du) * Rm
            g = dh / Lk
            c = (Lk + a_up * np.maximum(dh, f32(0))) + a_dn * np.maximum(-dh, f32(0))
            if P is None:
                m = f32(1)
            else:
                m = f32(0.5) * (P[ui, uj] + P[vi, vj])
            w = (c * m).astype(np.float32)
            w[np.abs(g) > gmax] = np.inf
            out[k][vi, vj] = w
    return out


def reduce_sources(src_ij, src_cost=None):
    best = {}
    for n, (i, j) in enumerate(np.asarray(src_ij).reshape(-1, 2)):
        c = 0.0 if src_cost is None else float(src_cost[n]) + 0.0
        key = (int(i), int(j))
        best[key] = min(best.get(key, math.inf), c)
    return best


def dijkstra(wt, sources, wrap):
    """float64 costs: heapq Dijkstra over the 8-neighbour lattice, d[v] = min(src[v], min_u d[u] + (double)w(u -> v))."""
    _, rows, cols = wt.shape
    d = np.full((rows, cols), np.inf)
    heap = []
    for (i, j), c in sources.items():
        if c < d[i, j]:
            d[i, j] = c
            heapq.heappush(heap, (c, i, j))
    # out-edges of u: to v = u - step k, using wt[k, v]
    wl = wt.astype(np.float64).tolist()
    dl = d.tolist()
    done = [[False] * cols for _ in range(rows)]
    while heap:
        du, ui, uj = heapq.heappop(heap)
        if done[ui][uj] or du > dl[ui][uj]:
            continue
        done[ui][uj] = True
        for k in range(8):
            vi, vj = ui - DI[k], uj - DJ[k]
            if wrap:
                vj %= cols
            if not (0 <= vi < rows and 0 <= vj < cols):
                continue
            w = wl[k][vi][vj]
            if w == math.inf:
                continue
            nd = du + w
            if nd < dl[vi][vj]:
                dl[vi][vj] = nd
                heapq.heappush(heap, (nd, vi, vj))
    return np.array(dl, np.float64)


def predecessors(d, wt, sources, wrap):
    rows, cols = d.shape
    pred = np.where(np.isinf(d), 255, 254).astype(np.uint8)
    found = np.zeros((rows, cols), bool)
    ii, jj = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    for k in range(8):
        ui, uj = ii + DI[k], jj + DJ[k]
        if wrap:
            uj = uj % cols
        ok = (ui >= 0) & (ui < rows) & (uj >= 0) & (uj < cols)
        du = np.full((rows, cols), np.inf)
        du[ok] = d[ui[ok], uj[ok]]
        w = wt[k].astype(np.float64)
        hit = ok & ~found & np.isfinite(d) & (du < d) & np.isfinite(w) & (du + w == d)
        pred[hit] = k
        found |= hit
    for (i, j), c in sources.items():
        if d[i, j] == c:
            pred[i, j] = 8
    return pred


def field(dem, t, src_ij, src_cost=None, penalty=None):
    """(cost, pred) of the model for a DEM, an MrtxTraverse window, sources and an optional penalty map."""
    L = lengths(t, dem.shape)
    D = window_D(dem, t)
    P = None if penalty is None else np.asarray(penalty, np.float32)
    wt = weights(D, P, L, t)
    src = reduce_sources(src_ij, src_cost)
    d = dijkstra(wt, src, t.wrap)
    return d, predecessors(d, wt, src, t.wrap)
