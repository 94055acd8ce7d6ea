"""Built cases for the traverse stage's edge rules and tile hand-offs, TEST INFRASTRUCTURE, numpy only:

  pair lattices   period-3 cells of a 48 x 96 window, each a 2 x 2 block with two passable nodes, a source u and its neighbour v,
                  every other node walled by a +inf penalty: a two-node island whose A[v] (d[v]) is exactly g_uv(start_u).  Each
                  pair has its own direction, start, penalties, heights and availability rows, so one call runs some 500
                  independent instances of the edge rule at every phase of the 8, 16 and 32 tile grids.
  corridors       64 x 64 windows with a one-node-wide diagonal of penalty 1 in a sea of +inf: the value can only travel from
                  tile to tile through tile corners.
  thin windows    33 x 65 (a last tile one node high and one node wide at every tile edge), the same wrapped, 1 x 40, 40 x 1
                  and 1 x 1, on relief.

Everything here is input.  The expected results come from traverse_model / timed_traverse_model alone."""
import copy
import math

import numpy as np

import synth_np
import timed_traverse_model as ttm
import traverse_model as tm
from moonrtx_amd import traverse as tv
from traverse_model import DI, DJ

INF = float("inf")
RM = np.float32(1737400.0)
DEM_SHAPE = (180, 360)
ROW0, COL0 = 60, 100                    # the lattice window's first texel
ROWS, COLS = 48, 96
DI_arr, DJ_arr = np.array(DI), np.array(DJ)
TPC = 1.0 / 30000.0                     # ticks per cost of the timed lattices: an edge of penalty m lasts about m ticks


# ---- pair lattices -----------------------------------------------------------------------------------------------------------
def pair_sites(rows=ROWS, cols=COLS, origin=(0, 0), shift=0, force=None):
    """The pairs of a window: arrays k (the step from v to u), ui, uj, vi, vj.  Cell (ci, cj) holds the block whose first node is
    (origin + 3 ci, origin + 3 cj).  Among the 8 cells that share (ci mod 8, cj mod 8) in a 16 x 32 grid of cells every direction
    occurs once, so each direction meets each phase of the tile grids.  force(ci, cj) may give a cell's direction (or None);
    such a pair lies in the block's first row (E, W) or column (N, S), so the forced pairs of a cell row share an edge length."""
    oi, oj = origin
    out = []
    for ci in range((rows - 2 - oi) // 3 + 1):
        for cj in range((cols - 2 - oj) // 3 + 1):
            k = (ci + cj + 4 * (ci // 8) + cj // 8 + shift) % 8
            forced = force is not None and force(ci, cj) is not None
            if forced:
                k = force(ci, cj)
            a = 1 if DI[k] < 0 else 0 if DI[k] > 0 else 0 if forced else (ci + cj // 2) & 1
            b = 1 if DJ[k] < 0 else 0 if DJ[k] > 0 else 0 if forced else (cj + ci // 2) & 1
            vi, vj = oi + 3 * ci + a, oj + 3 * cj + b
            out.append((k, vi + DI[k], vj + DJ[k], vi, vj, ci, cj))
    s = np.array(out, np.int64)
    sites = dict(k=s[:, 0], ui=s[:, 1], uj=s[:, 2], vi=s[:, 3], vj=s[:, 4], ci=s[:, 5], cj=s[:, 6], rows=rows, cols=cols)
    assert (np.bincount(sites["k"], minlength=8) * 16 >= len(s)).all()      # every direction on at least 1/16 of the pairs
    return sites


class Lattice:
    """A pair lattice: dem, window t, penalty P, the sites, src (n, 2) and per-pair start values `start`; for a timed one also
    tpe, tpc, n_epochs, avail (rows, cols, n_epochs booleans) and per pair ok_u, ok_v (lists of booleans) and q."""

    def __init__(self, sites, Pu, Pv, Du=None, Dv=None, start=None, max_grade=INF):
        n = len(sites["k"])
        self.sites = sites
        self.n = n
        rows, cols = sites["rows"], sites["cols"]
        self.dem = np.ones(DEM_SHAPE, np.float32)
        self.P = np.full((rows, cols), np.inf, np.float32)
        self.P[sites["ui"], sites["uj"]] = np.asarray(Pu, np.float32)
        self.P[sites["vi"], sites["vj"]] = np.asarray(Pv, np.float32)
        if Du is not None:
            self.dem[ROW0 + sites["ui"], COL0 + sites["uj"]] = np.asarray(Du, np.float32)
            self.dem[ROW0 + sites["vi"], COL0 + sites["vj"]] = np.asarray(Dv, np.float32)
        self.max_grade = max_grade
        self.src = np.stack([sites["ui"], sites["uj"]], axis=1).astype(np.int32)
        self.start = start
        self.avail = None

    @property
    def t(self):
        return tm.make_window(ROW0, COL0, self.sites["rows"], self.sites["cols"], max_grade=self.max_grade)

    def pair_weights(self):
        """float32 w(u -> v) of every pair, from the model's weights."""
        t = self.t
        wt = tm.weights(tm.window_D(self.dem, t), self.P, tm.lengths(t, self.dem.shape), t)
        return wt[self.sites["k"], self.sites["vi"], self.sites["vj"]]

    def without(self, p):
        """The same lattice with pair p walled in."""
        o = copy.copy(self)
        o.P = self.P.copy()
        o.P[self.sites["ui"][p], self.sites["uj"][p]] = np.inf
        o.P[self.sites["vi"][p], self.sites["vj"][p]] = np.inf
        keep = np.arange(self.n) != p
        o.src = self.src[keep]
        o.start = None if self.start is None else np.asarray(self.start)[keep]
        return o

    def walled(self):
        return np.isinf(self.P)


def edge_lengths(sites):
    """L of every pair's edge, from the library's lengths of the lattice window."""
    t = tm.make_window(ROW0, COL0, sites["rows"], sites["cols"])
    L = tm.lengths(t, DEM_SHAPE)
    k, vi, ui = sites["k"], sites["vi"], sites["ui"]
    col = np.where(DI_arr[k] == 0, 0, np.where(DJ_arr[k] == 0, 1, 2))
    row = np.where(DI_arr[k] == 0, vi, np.minimum(vi, ui))
    return L[row, col]


# The classes of a timed lattice, dealt to the pairs in turn (pair p gets CLASSES[p % len(CLASSES)])
CLASSES = ("same_word", "next_word", "skip_word", "fit_last_tick", "one_tick_more", "cross_one", "block63", "block0", "span2",
           "span2_block3", "last_epoch", "past_table", "never_joint", "src_closed", "q1", "random", "random_short", "random", "random_long")


def _target_q(cls, tpe, rng):
    if cls in ("same_word", "next_word", "skip_word", "src_closed", "never_joint", "random_short"):
        return int(rng.integers(1, 3 * tpe + 1))
    if cls == "fit_last_tick":
        return int(rng.integers(1, tpe + 1))
    if cls == "one_tick_more":
        return int(rng.integers(2, tpe + 2))
    if cls in ("cross_one", "block63", "block0"):
        return int(rng.integers(5 * tpe, 40 * tpe + 1))
    if cls in ("span2", "span2_block3"):
        return int(rng.integers(140 * tpe, 190 * tpe + 1))
    if cls == "last_epoch":
        return int(rng.integers(1, 20 * tpe + 1))
    if cls == "past_table":
        return int(rng.integers(2, 20 * tpe + 1))
    if cls == "q1":
        return 1
    if cls == "random_long":
        return int(rng.integers(60 * tpe, 200 * tpe + 1))
    return int(math.exp(rng.uniform(0.0, math.log(200 * tpe))))


def _runs(n, rng, on=60.0, off=5.0):
    """Alternating runs of available and unavailable epochs with geometric lengths."""
    out, v = [], bool(rng.random() < 0.8)
    while len(out) < n:
        out += [v] * int(rng.geometric(1.0 / (on if v else off)))
        v = not v
    return out[:n]


def _split(both, rng):
    """Rows for u and v whose AND is `both`: where it is False, one of (1, 0), (0, 1), (0, 0)."""
    c = rng.integers(0, 3, len(both))
    b = np.asarray(both, bool)
    return (b | (c == 0)).tolist(), (b | (c == 1)).tolist()


def _design(cls, q, n, tpe, rng):
    """(start tick, both) of a pair of class cls whose edge lasts q ticks, in a table of n >= 300 epochs."""
    span = (q - 1) // tpe + 2                       # epochs that hold a drive of q ticks from any tick of the first
    off = int(rng.integers(0, tpe))
    both = [False] * n
    if cls in ("same_word", "src_closed"):
        wk = int(rng.integers(0, 4))
        ea = 64 * wk + int(rng.integers(0, 40))
        e1 = ea + int(rng.integers(1, 21))
        both[e1:e1 + span] = [True] * span
        return ea * tpe + off, both
    if cls == "next_word":
        wk = int(rng.integers(0, 3))
        ea = 64 * wk + int(rng.integers(30, 64))
        e1 = 64 * (wk + 1) + int(rng.integers(0, 30))
        both[e1:e1 + span] = [True] * span
        return ea * tpe + off, both
    if cls == "skip_word":
        ea = int(rng.integers(0, 64))
        e1 = 64 * int(rng.integers(2, 4)) + int(rng.integers(0, 50))
        both[e1:e1 + span] = [True] * span
        return ea * tpe + off, both
    if cls == "never_joint":
        return int(rng.integers(0, n * tpe)), both
    if cls == "fit_last_tick":                      # q <= tpe: the drive ends on epoch e's last tick, epoch e + 1 is closed
        e = int(rng.integers(1, n - 3))
        both = (rng.random(n) < 0.5).tolist()
        both[e], both[e + 1] = True, False
        return (e + 1) * tpe - q, both
    if cls == "one_tick_more":                      # q <= tpe + 1: the last tick is epoch e + 1's first, and that epoch is closed
        e = int(rng.integers(1, n - 8))
        both = (rng.random(n) < 0.5).tolist()
        both[e], both[e + 1] = True, False
        both[e + 2:e + 2 + span] = [True] * span
        return (e + 1) * tpe - q + 1, both
    if cls in ("cross_one", "block63", "block0"):   # q >= 5 tpe: from 2 to 4 epochs before a word boundary B across it
        B = 64 * int(rng.integers(1, 4))
        e0 = B - int(rng.integers(2, 5))
        both = (rng.random(n) < 0.5).tolist()
        both[e0 - 1] = False
        both[e0:B + span + 2] = [True] * (B + span + 2 - e0)
        if cls == "block63":
            both[B - 1] = False
        if cls == "block0":
            both[B] = False
        return e0 * tpe + off, both
    if cls in ("span2", "span2_block3"):            # q >= 140 tpe: from word 0 into word 3
        ne = (q - 1) // tpe
        e0 = int(rng.integers(max(0, 192 - ne), 64))
        both = [True] * n
        if e0 > 0:
            both[e0 - 1] = False
        if cls == "span2_block3":
            both[int(rng.integers(128, 192))] = False
        return e0 * tpe + off, both
    if cls in ("last_epoch", "past_table"):
        o = off if cls == "last_epoch" else int(rng.integers(0, min(tpe, q - 1)))
        T = (n - 1 if cls == "last_epoch" else n) * tpe + o      # the drive's last tick
        a = T - q + 1
        both = (rng.random(n) < 0.5).tolist()
        both[a // tpe:] = [True] * (n - a // tpe)
        return a, both
    if cls == "q1":
        return int(rng.integers(0, n * tpe)), (rng.random(n) < 0.6).tolist()
    a = int(rng.integers(0, (n // 2 if cls == "random_long" else n) * tpe))
    return a, _runs(n, rng, on=200.0 if cls == "random_long" else 60.0)


def _penalties_for(q_target, L, tpc, rng):
    """Pu, Pv (float32) with 0.5 (Pu + Pv) L tpc about q_target - 0.5, so that the edge lasts q_target ticks."""
    m = (np.asarray(q_target, np.float64) - 0.5) / (L.astype(np.float64) * tpc)
    r = rng.uniform(-0.5, 0.5, len(m))
    return (m * (1 + r)).astype(np.float32), (m * (1 - r)).astype(np.float32)


def _finish_timed(lat, ok_u, ok_v, n_epochs, tpe, tpc, rng):
    rows, cols = lat.sites["rows"], lat.sites["cols"]
    av = rng.random((rows, cols, n_epochs)) < 0.5          # the walled nodes' rows are never read by a correct field
    s = lat.sites
    av[s["ui"], s["uj"]] = np.array(ok_u, bool)
    av[s["vi"], s["vj"]] = np.array(ok_v, bool)
    lat.avail, lat.ok_u, lat.ok_v = av, ok_u, ok_v
    lat.n_epochs, lat.tpe, lat.tpc = n_epochs, tpe, tpc
    return lat


def timed_lattice(n_epochs, tpe, origin=(0, 0), shift=0, seed=1):
    """A pair lattice for the arrival field under a table of n_epochs >= 300 epochs of tpe <= 7 ticks: the pairs are dealt the
    CLASSES in turn, each edge's penalties chosen for a duration that suits its class, its start tick and rows then designed
    around the duration the model gives the edge."""
    rng = np.random.default_rng(seed)
    sites = pair_sites(origin=origin, shift=shift)
    n = len(sites["k"])
    cls = [CLASSES[p % len(CLASSES)] for p in range(n)]
    L = edge_lengths(sites)
    Pu, Pv = _penalties_for([_target_q(c, tpe, rng) for c in cls], L, TPC, rng)
    lat = Lattice(sites, Pu, Pv)
    q = [tv.edge_ticks(w, TPC) for w in lat.pair_weights()]
    assert None not in q
    start, ok_u, ok_v = [], [], []
    for p in range(n):
        a, both = _design(cls[p], q[p], n_epochs, tpe, rng)
        u, v = _split(both, rng)
        if cls[p] == "src_closed":
            u[a // tpe], v[a // tpe] = False, True
        if cls[p] == "never_joint":
            i, j = rng.choice(n_epochs, 2, replace=False)
            u[i], v[i], u[j], v[j] = True, False, False, True
        start.append(a)
        ok_u.append(u)
        ok_v.append(v)
    lat.start, lat.q, lat.cls = np.array(start, np.uint64), q, cls
    return _finish_timed(lat, ok_u, ok_v, n_epochs, tpe, TPC, rng)


BIG_TPE = (1 << 31) - 1
BIG_CLASSES = ("cross32", "above32", "big_q", "too_long", "random")


def big_tick_lattice(n_epochs=130, seed=9):
    """A pair lattice with ticks_per_epoch = 2^31 - 1 and ticks_per_cost = 1: ticks on both sides of 2^32 (tick 2^32 lies in
    epoch 2), durations up to 2^31 and edges too long to be driven."""
    rng = np.random.default_rng(seed)
    sites = pair_sites(origin=(1, 2), shift=3)
    n = len(sites["k"])
    cls = [BIG_CLASSES[p % len(BIG_CLASSES)] for p in range(n)]
    L = edge_lengths(sites)
    target = []
    for c in cls:
        if c == "big_q":
            target.append(rng.uniform(2.0 ** 30 * 1.001, 2.0 ** 31 * 0.999))
        elif c == "too_long":
            target.append(rng.uniform(2.0 ** 31 * 1.001, 2.0 ** 33))
        else:
            target.append(math.exp(rng.uniform(math.log(1e3), math.log(2.0 ** 31 * 0.999))))
    Pu, Pv = _penalties_for(target, L, 1.0, rng)
    lat = Lattice(sites, Pu, Pv)
    q = [tv.edge_ticks(w, 1.0) for w in lat.pair_weights()]
    start, ok_u, ok_v = [], [], []
    for p in range(n):
        if cls[p] == "cross32":                     # a < 2^32 <= a + q - 1, epochs 1 to 3 open
            a = (1 << 32) - 1 - int(rng.integers(0, q[p] - 1))
            both = _runs(n_epochs, rng)
            both[1:4] = [True] * 3
        elif cls[p] == "above32":
            a = int(rng.integers(1 << 32, (n_epochs - 2) * BIG_TPE))
            both = _runs(n_epochs, rng, on=8.0, off=2.0)
        else:
            a = int(rng.integers(0, (n_epochs - 2) * BIG_TPE))
            both = _runs(n_epochs, rng, on=8.0, off=2.0)
        u, v = _split(both, rng)
        start.append(a)
        ok_u.append(u)
        ok_v.append(v)
    lat.start, lat.q, lat.cls = np.array(start, np.uint64), q, cls
    return _finish_timed(lat, ok_u, ok_v, n_epochs, BIG_TPE, 1.0, rng)


def packed(avail, seed=None):
    """pack_mask's words; with a seed, random garbage in the bits past the last epoch of every row's last word."""
    words = tv.pack_mask(avail).copy()
    n = avail.shape[-1]
    if seed is not None and n & 63:
        g = np.random.default_rng(seed).integers(0, 1 << 63, words.shape[:-1], dtype=np.uint64) * np.uint64(2) + \
            np.random.default_rng(seed + 1).integers(0, 2, words.shape[:-1], dtype=np.uint64)
        words[..., -1] |= g & ~np.uint64((1 << (n & 63)) - 1)
    return words


def unpacked_all(words):
    """Every bit of the words, the garbage past the table included: (..., 64 W64) booleans."""
    w = np.ascontiguousarray(words, "<u8")
    return np.unpackbits(w.view(np.uint8), axis=-1, bitorder="little").astype(bool)


def cost_lattice(seed=4):
    """A pair lattice for the cost field on the flat DEM: penalties at 1e-3, at 1e6 and mixed, start costs 0, 2^52 (where
    xu + (double)w rounds) and others."""
    rng = np.random.default_rng(seed)
    sites = pair_sites(origin=(2, 1), shift=5)
    n = len(sites["k"])
    kind = np.arange(n) % 3
    mixed = np.where(rng.random((2, n)) < 0.5, np.float32(1e-3), np.float32(1e6))
    mixed = np.where(rng.random((2, n)) < 0.3, np.exp(rng.uniform(math.log(1e-3), math.log(1e6), (2, n))), mixed).astype(np.float32)
    Pu = np.where(kind == 0, np.float32(1e-3), np.where(kind == 1, np.float32(1e6), mixed[0])).astype(np.float32)
    Pv = np.where(kind == 0, np.float32(1e-3), np.where(kind == 1, np.float32(1e6), mixed[1])).astype(np.float32)
    c0 = np.where(np.arange(n) // 3 % 3 == 0, 0.0, np.where(np.arange(n) // 3 % 3 == 1, 2.0 ** 52, rng.uniform(0.0, 1e9, n)))
    return Lattice(sites, Pu, Pv, start=c0)


# ---- grade cases ---------------------------------------------------------------------------------------------------------------
GRADE_KREF = 7243                       # the reference rise in float32 steps of 2^-23 above 1: about 1500 m, a grade near 0.05
GRADE_REF_ROW = 5                       # the cell row of the reference pairs
GRADE_KINDS = {"ew": (2, 6), "ns": (0, 4), "dg": (1, 5)}       # the two directions of the reference pairs: one edge length
GRADE_VARIANTS = ("climb", "descend", "climb_above", "descend_above", "climb_below", "descend_below")


def _f32_step(x, n):
    """The float32 n steps above (n < 0: below) x, for x = 1 or a float32 in (1, 2): steps of 2^-23, below 1 of 2^-24."""
    x = np.float32(x)
    if n < 0 and x == np.float32(1.0):
        return np.float32(1.0 + n * 2.0 ** -24)
    return np.float32(float(x) + n * 2.0 ** -23)


def grade32(Du, Dv, L):
    """The grade of the edge u -> v in float32, in the spec's order."""
    dh = np.float32(np.float32(np.float32(Dv) - np.float32(Du)) * RM)
    return np.float32(dh / np.float32(L))


def grade_lattice(kind, tight=False, seed=6):
    """A pair lattice with raised nodes.  The pairs of cell row GRADE_REF_ROW share one edge length (directions
    GRADE_KINDS[kind]) and take the GRADE_VARIANTS in turn: u -> v climbs (or descends) by exactly the reference rise, or v is
    one float32 above or below that.  max_grade is the reference pair's float32 grade g32, or with tight the next float32
    towards 0.  The other pairs rise and fall at random around the limit.  Returns the lattice with g32 and per pair `variant`
    (None off the reference row)."""
    rng = np.random.default_rng(seed)
    ka, kb = GRADE_KINDS[kind]
    sites = pair_sites(origin=(0, 1), shift=2, force=lambda ci, cj: (ka if cj % 2 == 0 else kb) if ci == GRADE_REF_ROW else None)
    n = len(sites["k"])
    one, top = np.float32(1.0), _f32_step(1.0, GRADE_KREF)
    Du, Dv, variant = [], [], []
    for p in range(n):
        if sites["ci"][p] != GRADE_REF_ROW:
            d = _f32_step(1.0, int(rng.integers(0, 2 * GRADE_KREF)))
            Du.append(one if rng.random() < 0.5 else d)
            Dv.append(d if Du[-1] == one else one)
            variant.append(None)
            continue
        var = GRADE_VARIANTS[(sites["cj"][p] // 2) % 6]
        step = 1 if var.endswith("above") else -1 if var.endswith("below") else 0
        if var.startswith("climb"):
            Du.append(one)
            Dv.append(_f32_step(top, step))
        else:
            Du.append(top)
            Dv.append(_f32_step(one, step))
        variant.append(var)
    ref = [p for p in range(n) if variant[p] == "climb"][0]
    lat = Lattice(sites, np.ones(n, np.float32), np.ones(n, np.float32), Du, Dv)
    g32 = grade32(one, top, edge_lengths(sites)[ref])
    lat.g32, lat.variant = g32, variant
    lat.max_grade = float(np.nextafter(g32, np.float32(0))) if tight else float(g32)
    return lat


# ---- corridors -----------------------------------------------------------------------------------------------------------------
def _relief(h, w, seed):
    return synth_np.dem(h, w, seed=seed, craters=20)


_DEMS = {}


def _dem(h, w, seed):
    if (h, w, seed) not in _DEMS:
        _DEMS[h, w, seed] = _relief(h, w, seed)
    return _DEMS[h, w, seed]


# name: (corridor, sources, the predecessor code along the run from each source's side)
#   main: j = i (steps SE / NW); anti: j = 63 - i (steps SW / NE); wrap: j = (i + 32) mod 64 in a wrapped window
CORRIDORS = {
    "main-from-nw": ("main", [(0, 0)]),
    "main-from-se": ("main", [(63, 63)]),
    "anti-from-ne": ("anti", [(0, 63)]),
    "anti-from-sw": ("anti", [(63, 0)]),
    "main-from-31": ("main", [(31, 31)]),         # the last node of a tile at every tile edge: its onward edge leaves by the corner
    "anti-from-31": ("anti", [(31, 32)]),
    "wrap-from-n": ("wrap", [(0, 32)]),           # crosses +-180 between (31, 63) and (32, 0): a tile corner at every size
    "wrap-from-s": ("wrap", [(63, 31)]),
}


def corridor(name):
    """(dem, t, src, P, on) of a corridor case: on = the corridor's nodes as a boolean map."""
    shape, src = CORRIDORS[name]
    i = np.arange(64)
    j = i if shape == "main" else 63 - i if shape == "anti" else (i + 32) % 64
    P = np.full((64, 64), np.inf, np.float32)
    P[i, j] = 1.0
    if shape == "wrap":
        dem = _dem(160, 128, 13)
        t = tm.make_window(10, 6, 64, 64, stride=2, wrap=1, max_grade=INF)
    else:
        dem = _dem(180, 360, 11)
        t = tm.make_window(40, 100, 64, 64, max_grade=INF)
    return dem, t, src, P, np.isfinite(P)


def corridor_codes(name):
    """The predecessor code a corridor node has when it is reached from the node before it (smaller i) and from the node after
    it: (from_before, from_after)."""
    shape = CORRIDORS[name][0]
    return (1, 5) if shape == "anti" else (7, 3)      # anti: the node before is (i - 1, j + 1), NE; else (i - 1, j - 1), NW


# 300 epochs: the longest corridor (the wrapped one, on a coarser lattice) takes 98 epochs without a table
CORRIDOR_TIMED = dict(n_epochs=300, tpe=100, tpc=0.001, p=0.9, ticks=[250])


def corridor_mask(name):
    c = CORRIDOR_TIMED
    return ttm.mask_random(64, 64, c["n_epochs"], c["p"], seed=len(name) + sum(map(ord, name)) % 50)


# ---- thin windows --------------------------------------------------------------------------------------------------------------
THIN = {
    # name: (dem shape, dem seed, window, sources, start values)
    "33x65": ((180, 360), 7, dict(row0=30, col0=100, rows=33, cols=65), [(2, 3), (32, 64), (16, 64)]),
    "33x65-wrap": ((100, 130), 5, dict(row0=4, col0=7, rows=33, cols=65, stride=2, wrap=1), [(2, 3), (32, 64), (16, 0)]),
    "1x40": ((180, 360), 7, dict(row0=50, col0=120, rows=1, cols=40), [(0, 5), (0, 39)]),
    "40x1": ((180, 360), 7, dict(row0=50, col0=120, rows=40, cols=1), [(7, 0), (39, 0)]),
    "1x1": ((180, 360), 7, dict(row0=50, col0=120, rows=1, cols=1), [(0, 0)]),
}
THIN_TIMED = dict(n_epochs=130, tpe=1500, tpc=0.01, p=0.8)
# from the model alone: at 0.006 the grade limit closes edges in the first three windows and each is still reached to 0.92 or
# more (0.1 to 0.86 of them at 0.002, all of every one from 0.02 on)
THIN_GRADE = 0.006


def thin(name):
    """(dem, t, src, start costs, start ticks, avail) of a thin window on relief."""
    shape, seed, win, src = THIN[name]
    dem = _dem(shape[0], shape[1], seed)
    t = tm.make_window(max_grade=THIN_GRADE, descent_cost=1.0, **win)
    c = THIN_TIMED
    av = ttm.mask_random(t.rows, t.cols, c["n_epochs"], c["p"], seed=len(name))
    n = len(src)
    return dem, t, src, [0.0, 4e4, 1e4][:n], [0, 3000, 700][:n], av
