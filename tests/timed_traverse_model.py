"""The timed traverse on the CPU, TEST INFRASTRUCTURE: float32 edge weights from traverse_model, the
durations q by the spec's rule, a word-free start() over a Python list of booleans, a heapq Dijkstra over Python ints and the
predecessor rule.  Also start_trace() (start() with a record of what it did), a brute-force start(), a randomly ordered
label-correcting loop and the synthetic masks of the GPU tests."""
import collections
import heapq
import math

import numpy as np

import traverse_model as tm
from traverse_model import DI, DJ

NEVER = 0xFFFFFFFFFFFFFFFF


def durations(wt, ticks_per_cost):
    """(8, rows, cols) nested lists: q of every incoming edge, None where it is not driven."""
    x = wt.astype(np.float64) * float(ticks_per_cost)
    drive = np.isfinite(wt) & (x <= 2147483648.0)
    q = np.where(drive, np.where(x <= 1.0, 1.0, np.ceil(np.where(drive, x, 0.0))), 0.0).astype(np.int64)
    out = q.astype(object)
    out[~drive] = None
    return out.tolist()


def start(ok, a, q, tpe):
    """The least tick t >= a such that every epoch t // tpe .. (t + q - 1) // tpe is True in the list `ok` (epochs past its
    end are unavailable), or None.  ok = None: always available."""
    if ok is None:
        return a
    n = len(ok)
    t = a
    while True:
        e = t // tpe
        while e < n and not ok[e]:
            e += 1
        if e >= n:
            return None
        if e > t // tpe:
            t = e * tpe
        last = (t + q - 1) // tpe
        z = e
        while z < n and z <= last and ok[z]:
            z += 1
        if z > last:
            return t
        t = (z + 1) * tpe


Trace = collections.namedtuple("Trace", "t restarts boundaries skipped_zero_word past_table attempts")


def start_trace(ok, a, q, tpe):
    """start()'s result and what happened on the way, as a Trace:
      t                  start(ok, a, q, tpe)
      restarts           how often the search went on behind a blocking epoch
      boundaries         the 64-epoch word boundaries between the first and the last epoch of the accepted drive (0 if none)
      skipped_zero_word  a whole word of 64 unavailable epochs lay between an epoch the search looked from and the available
                         epoch it found
      past_table         t is None because the last tick of the drive falls past the table (no later start fits either)
      attempts           (first epoch, last epoch, blocking epoch or None) of every drive that was tried
    Word-free like start(): words appear only as e // 64 in the bookkeeping."""
    if ok is None:
        return Trace(a, 0, 0, False, False, [])
    n = len(ok)
    t = a
    restarts, skipped, attempts = 0, False, []
    while True:
        e0 = t // tpe
        e = e0
        while e < n and not ok[e]:
            e += 1
        if e >= n:
            return Trace(None, restarts, 0, skipped, False, attempts)
        if e // 64 - e0 // 64 >= 2:
            skipped = True
        if e > e0:
            t = e * tpe
        last = (t + q - 1) // tpe
        if last >= n:
            attempts.append((e, last, None))
            return Trace(None, restarts, 0, skipped, True, attempts)
        z = e
        while z <= last and ok[z]:
            z += 1
        if z > last:
            attempts.append((e, last, None))
            return Trace(t, restarts, last // 64 - e // 64, skipped, False, attempts)
        attempts.append((e, last, z))
        restarts += 1
        t = (z + 1) * tpe


def start_brute(ok, a, q, tpe):
    """start() tick by tick."""
    n = len(ok)
    for t in range(a, n * tpe):
        if all(e < n and ok[e] for e in range(t // tpe, (t + q - 1) // tpe + 1)):
            return t
    return None


def both_rows(avail):
    """avail (rows, cols, m) booleans or None -> a function (ui, uj, vi, vj) -> the list of epochs available at both."""
    if avail is None:
        return lambda ui, uj, vi, vj: None
    av = np.asarray(avail, bool)
    return lambda ui, uj, vi, vj: (av[ui, uj] & av[vi, vj]).tolist()


def reduce_sources(src_ij, src_tick=None):
    best = {}
    for n, (i, j) in enumerate(np.asarray(src_ij).reshape(-1, 2)):
        c = 0 if src_tick is None else int(src_tick[n])
        key = (int(i), int(j))
        best[key] = min(best.get(key, NEVER), c)
    return best


def arrive(rows_of, ql, tpe, k, vi, vj, ui, uj, a):
    """g_uv(a) for v = (vi, vj) and u = v + step k, or None."""
    q = ql[k][vi][vj]
    if q is None:
        return None
    t = start(rows_of(ui, uj, vi, vj), a, q, tpe)
    return None if t is None else t + q


def dijkstra(ql, sources, wrap, avail, tpe):
    """Arrival ticks as nested lists of Python ints (NEVER: unreachable)."""
    rows, cols = len(ql[0]), len(ql[0][0])
    rows_of = both_rows(avail)
    A = [[NEVER] * cols for _ in range(rows)]
    heap = []
    for (i, j), c in sources.items():
        if c < A[i][j]:
            A[i][j] = c
            heapq.heappush(heap, (c, i, j))
    done = [[False] * cols for _ in range(rows)]
    while heap:
        au, ui, uj = heapq.heappop(heap)
        if done[ui][uj] or au > A[ui][uj]:
            continue
        done[ui][uj] = True
        for k in range(8):
            vi, vj = ui - DI[k], uj - DJ[k]
            if wrap:
                vj %= cols
            if not (0 <= vi < rows and 0 <= vj < cols):
                continue
            q = ql[k][vi][vj]
            if q is None or au + q >= A[vi][vj]:
                continue
            g = arrive(rows_of, ql, tpe, k, vi, vj, ui, uj, au)
            if g is not None and g < A[vi][vj]:
                A[vi][vj] = g
                heapq.heappush(heap, (g, vi, vj))
    return A


def label_correcting(ql, sources, wrap, avail, tpe, rng):
    """The same fixed point by relaxing the edges in a random order until a pass lowers nothing."""
    rows, cols = len(ql[0]), len(ql[0][0])
    rows_of = both_rows(avail)
    A = [[NEVER] * cols for _ in range(rows)]
    for (i, j), c in sources.items():
        A[i][j] = min(A[i][j], c)
    edges = [(k, i, j) for k in range(8) for i in range(rows) for j in range(cols) if ql[k][i][j] is not None]
    changed = True
    while changed:
        changed = False
        for e in rng.permutation(len(edges)):
            k, vi, vj = edges[e]
            ui, uj = vi + DI[k], vj + DJ[k]
            if wrap:
                uj %= cols
            if A[ui][uj] == NEVER:
                continue
            g = arrive(rows_of, ql, tpe, k, vi, vj, ui, uj, A[ui][uj])
            if g is not None and g < A[vi][vj]:
                A[vi][vj] = g
                changed = True
    return A


def predecessors(A, ql, sources, wrap, avail, tpe):
    rows, cols = len(A), len(A[0])
    rows_of = both_rows(avail)
    pred = np.full((rows, cols), 255, np.uint8)
    for vi in range(rows):
        for vj in range(cols):
            av = A[vi][vj]
            if av == NEVER:
                continue
            code = 254
            for k in range(8):
                ui, uj = vi + DI[k], vj + DJ[k]
                if wrap:
                    uj %= cols
                if not (0 <= ui < rows and 0 <= uj < cols) or not A[ui][uj] < av:
                    continue
                if arrive(rows_of, ql, tpe, k, vi, vj, ui, uj, A[ui][uj]) == av:
                    code = k
                    break
            pred[vi, vj] = code
    for (i, j), c in sources.items():
        if A[i][j] == c:
            pred[i, j] = 8
    return pred


def field(dem, t, src_ij, src_tick=None, penalty=None, avail=None, ticks_per_cost=5.0, tpe=3600):
    """(arrival uint64, pred uint8) of the model: avail = (rows, cols, n_epochs) booleans or None."""
    L = tm.lengths(t, dem.shape)
    D = tm.window_D(dem, t)
    P = None if penalty is None else np.asarray(penalty, np.float32)
    ql = durations(tm.weights(D, P, L, t), ticks_per_cost)
    src = reduce_sources(src_ij, src_tick)
    A = dijkstra(ql, src, t.wrap, avail, tpe)
    return np.array(A, np.uint64), predecessors(A, ql, src, t.wrap, avail, tpe)


def waits_on_routes(arrival, pred, ql, wrap):
    """Per node: True if the route the predecessors give it holds a wait (some step's A[v] - q - A[u] > 0)."""
    rows, cols = arrival.shape
    order = np.argsort(arrival, axis=None, kind="stable")
    waited = np.zeros((rows, cols), bool)
    for n in order:
        vi, vj = divmod(int(n), cols)
        k = int(pred[vi, vj])
        if k > 7:
            continue
        ui, uj = vi + DI[k], vj + DJ[k]
        if wrap:
            uj %= cols
        own = int(arrival[vi, vj]) - ql[k][vi][vj] - int(arrival[ui, uj]) > 0
        waited[vi, vj] = own or waited[ui, uj]
    return waited


# ---- synthetic masks: (rows, cols, n_epochs) booleans
def mask_random(rows, cols, n_epochs, p=0.7, seed=1):
    return np.random.default_rng(seed).random((rows, cols, n_epochs)) < p


def mask_moving_night(rows, cols, n_epochs, width, speed=1.0, j_start=0):
    """A dark band j0(e) <= j < j0(e) + width, j0(e) = j_start + floor(speed e) modulo cols + width, moving across the columns."""
    e = np.arange(n_epochs)
    j0 = (j_start + np.floor(speed * e).astype(np.int64)) % (cols + width) - width
    j = np.arange(cols)
    dark = (j[None, :] >= j0[:, None]) & (j[None, :] < j0[:, None] + width)       # (n_epochs, cols)
    return np.broadcast_to(~dark.T[None, :, :], (rows, cols, n_epochs)).copy()
