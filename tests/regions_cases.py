"""Built cases of the regions stage, each small enough for tests/regions_model.py to answer in about a
second.  A case is a dict: name, wrap, and either mask (rows, cols) uint8 or field (rows, cols, n_ch) float32 with ch, lo, hi.
`answer(case, connectivity)` is the model's (labels, n), computed once per process and shared; `table(case, connectivity,
weights)` its catalogue.

TILE is the shape of the label pass's tiles, (rows, cols) = (16, 64): what "inside a tile" and "a tile border" mean below."""
import functools

import numpy as np

import regions_model as model

TILE = (16, 64)
# float32 rounding is part of the predicate: (float)LO < LO and (float)HI > HI, so float32(LO) and float32(HI) are in the set
# although a float64 comparison would put them out
LO, HI = 0.7, 1.1


def _mask(rows, cols):
    return np.zeros((rows, cols), np.uint8)


def spiral(n=96):
    """A one-node-wide spiral from (0, 0) inwards, arms two nodes apart: one region at either connectivity."""
    m = _mask(n, n)
    i, j, di, dj = 0, 0, 0, 1
    m[0, 0] = 1

    def free(a, b):
        return 0 <= a < n and 0 <= b < n and not m[a, b]

    def can(i, j, di, dj):
        a, b = i + di, j + dj
        if not free(a, b):
            return False
        # the new node touches the corridor only where it comes from
        return all((a + ei, b + ej) == (i, j) or not (0 <= a + ei < n and 0 <= b + ej < n and m[a + ei, b + ej])
                   for ei, ej in ((0, 1), (1, 0), (0, -1), (-1, 0)))

    while True:
        if not can(i, j, di, dj):
            di, dj = dj, -di
            if not can(i, j, di, dj):
                break
        i, j = i + di, j + dj
        m[i, j] = 1
    return m


def serpentine(n=96):
    """Every second row full, joined at alternating ends: one corridor from (0, 0) to the last row."""
    m = _mask(n, n)
    m[0::2, :] = 1
    for k, i in enumerate(range(1, n - 1, 2)):
        m[i, n - 1 if k % 2 == 0 else 0] = 1
    return m


def comb(rows=48, cols=140):
    """Teeth down every second column over rows 0 .. 31 (two rows of tiles) and a spine along row 32, the first row of the
    next tile: a tooth meets the spine only across a tile border, so inside every tile the teeth are separate pieces."""
    m = _mask(rows, cols)
    m[0:32, 0::2] = 1
    m[32, :] = 1
    return m


def u_shape(up):
    """Arms in columns 5, 50 (one tile column) and 100 (the next) and a bar that joins them across a tile border: below them
    (up = False; the root is an arm's top) or above them (up = True; the root is in the bar, found late by the arms' tiles)."""
    m = _mask(50, 120)
    for j in (5, 50, 100):
        m[(16 if up else 0):(48 if up else 32), j] = 1
    m[15 if up else 32, 5:101] = 1
    return m


def diagonal(kind, n=64):
    m = _mask(n, n)
    i = np.arange(n)
    m[i, {"main": i, "anti": n - 1 - i, "wrapped": (i + n // 2) % n}[kind]] = 1
    return m


def checkerboard(rows, cols):
    i, j = np.mgrid[0:rows, 0:cols]
    return ((i + j) % 2 == 0).astype(np.uint8)


def random_mask(rows, cols, density, seed):
    return (np.random.default_rng(seed).random((rows, cols)) < density).astype(np.uint8)


def seam_ring():
    """Rows 3 .. 4 all the way round a wrapped 20 x 70 window, root (3, 0): dj runs from -35 = -cols / 2 to 34."""
    m = _mask(20, 70)
    m[3:5, :] = 1
    return m


def seam_root_first():
    """A block across the seam, columns 65 .. 69 and 0 .. 4: the root is (5, 0), the columns west of the seam have dj < 0."""
    m = _mask(20, 70)
    m[5:9, 65:] = 1
    m[5:9, :5] = 1
    return m


def seam_root_last():
    """The root in the last column, (2, 69); the row below reaches both ways: dj > 0 east of the seam, dj < 0 west of it."""
    m = _mask(20, 70)
    m[2, 69] = 1
    m[3, 66:] = 1
    m[3, :6] = 1
    return m


def predicate_field(rows=24, cols=70, n_ch=4, seed=11):
    """Every channel drawn from a palette with NaN, +-inf, float32(LO), float32(HI) and their float32 neighbours outside."""
    lo32, hi32 = np.float32(LO), np.float32(HI)
    palette = np.array([np.nan, np.inf, -np.inf, lo32, np.nextafter(lo32, np.float32(-np.inf)), hi32,
                        np.nextafter(hi32, np.float32(np.inf)), 0.9, 0.0, 2.0, 0.8, 1.0], np.float32)
    return palette[np.random.default_rng(seed).integers(0, palette.size, (rows, cols, n_ch))]


def _build():
    out = []

    def add(name, mask, wrap=False):
        out.append({"name": name, "mask": np.ascontiguousarray(mask, np.uint8), "wrap": bool(wrap)})

    # thin and ragged windows: no side is a multiple of the tile
    add("1x1", np.ones((1, 1)))
    add("1x1_empty", np.zeros((1, 1)))
    add("1x40", random_mask(1, 40, 0.6, 1))
    add("40x1", random_mask(40, 1, 0.6, 2))
    add("33x65", random_mask(33, 65, 0.6, 3))
    add("33x65_wrapped", random_mask(33, 65, 0.6, 3), True)
    add("1x3_wrapped", np.array([[1, 0, 1]]), True)
    # corridors
    add("spiral", spiral())
    add("serpentine", serpentine())
    # locally separate pieces
    add("comb", comb())
    add("u_down", u_shape(False))
    add("u_up", u_shape(True))
    # diagonals
    add("diag_main", diagonal("main"))
    add("diag_anti", diagonal("anti"))
    add("diag_wrapped", diagonal("wrapped"), True)
    # checkerboards
    for rows, cols in ((32, 66), (33, 65)):
        add(f"checker_{rows}x{cols}", checkerboard(rows, cols))
        add(f"checker_{rows}x{cols}_wrapped", checkerboard(rows, cols), True)
    # empty and full
    add("empty", np.zeros((40, 130)))
    add("full", np.ones((256, 256)))
    add("full_wrapped", np.ones((20, 130)), True)
    # wrapped regions
    add("seam_ring", seam_ring(), True)
    add("seam_root_first", seam_root_first(), True)
    add("seam_root_last", seam_root_last(), True)
    # random masks; 0.59 is the 4-connected percolation threshold
    for d in (0.40, 0.59, 0.75):
        m = random_mask(200, 136, d, 20260 + int(d * 100))
        add(f"random_{d:.2f}", m)
        add(f"random_{d:.2f}_wrapped", m, True)
    # the field predicate, each channel
    f = predicate_field()
    for ch in range(f.shape[2]):
        out.append({"name": f"field_ch{ch}", "field": f, "ch": ch, "lo": LO, "hi": HI, "wrap": bool(ch % 2)})
    one = np.ascontiguousarray(f[:, :, 0])
    out.append({"name": "field_open", "field": one[:, :, None], "ch": 0, "lo": -np.inf, "hi": np.inf, "wrap": False})
    return out


CASES = _build()
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def case_mask(case):
    """The set as (rows, cols) uint8, from the mask or through the model's predicate."""
    if "mask" in case:
        return case["mask"]
    return model.predicate(case["field"], case["ch"], case["lo"], case["hi"]).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _answer(name, connectivity):
    case = BY_NAME[name]
    labels, n = model.label(case_mask(case), connectivity, case["wrap"])
    labels.setflags(write=False)
    return labels, n


def answer(case, connectivity):
    return _answer(case["name"], connectivity)


def weights_for(case, heavy=False):
    """(rows,) uint32 row weights of a case: distinct per row; heavy = near 2^32 - 1, so that sums need 64 bits."""
    rows = case_mask(case).shape[0]
    base = 2 ** 32 - 1 - rows if heavy else 1000
    return (base + np.arange(rows)).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def _table(name, connectivity, weighted, heavy):
    case = BY_NAME[name]
    labels, n = _answer(name, connectivity)
    t = model.catalogue(labels, n, case["wrap"], weights_for(case, heavy) if weighted else None)
    t.setflags(write=False)
    return t


def table(case, connectivity, weighted=False, heavy=False):
    return _table(case["name"], connectivity, bool(weighted), bool(heavy))
