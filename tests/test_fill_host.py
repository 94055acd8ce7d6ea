"""The terrain depressions without a GPU: the model against cases worked by hand and against a Jacobi
relaxation, the identities of the fill, the built lattices of the GPU tests, the height quantiser, the record's layout, every
refusal that needs no device, and the tool's CSV."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import fill_cases as fc
import fill_model as fm
import regions_model as rm
from moonrtx_amd import _lib
from moonrtx_amd import basins as bs

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))


def arr(rows):
    return np.array(rows, np.int32)


def jacobi(z, conn, wrap, edge_outlets, table=None):
    """The fill as the fixed point of whole-lattice steps W[v] = min(W[v], max(z[v], min_u W[u])) from W = z at the outlets."""
    z = np.asarray(z, np.int64)
    rows, cols = z.shape
    o = fm.outlets(rows, cols, wrap, edge_outlets, table)
    w = np.where(o, z, fm.NONE)
    while True:
        new = w.copy()
        for i in range(rows):
            for j in range(cols):
                m = min((w[a, b] for a, b in fm.neighbours(i, j, rows, cols, conn, wrap)), default=fm.NONE)
                new[i, j] = min(w[i, j], max(z[i, j], m))
        if (new == w).all():
            return w.astype(np.int32)
        w = new


# ---- the model against cases worked by hand
def test_a_single_pit():
    z = arr([[5, 5, 5, 5, 5], [5, 4, 3, 4, 5], [5, 4, 1, 4, 5], [5, 4, 4, 4, 5], [5, 5, 5, 5, 5]])
    for conn in (4, 8):
        f = fm.fill(z, conn)
        assert f.tolist() == np.full((5, 5), 5).tolist()
        assert np.array(fm.depth(f, z))[1:4, 1:4].tolist() == [[1, 2, 1], [1, 4, 1], [1, 1, 1]]


def test_a_pit_inside_a_pit_fills_to_the_outer_rim():
    z = np.full((9, 9), 20, np.int32)
    z[1:8, 1:8] = 10            # the outer bowl
    z[2:7, 2:7] = 12            # a rim inside it
    z[3:6, 3:6] = 2             # the inner bowl
    f = fm.fill(z, 8)
    assert (f[1:8, 1:8] == 20).all() and (f == 20).all()
    z[8, 4] = 15                # a notch in the outer rim: both bowls now fill to 15, above the inner rim of 12
    f = fm.fill(z, 4)
    assert (f[1:8, 1:8] == 15).all() and f[8, 4] == 15 and f[0, 0] == 20
    z[8, 4] = 11                # below the inner rim: the outer bowl fills to 11, the inner one to its own rim of 12
    f = fm.fill(z, 4)
    assert (f[1, 1:8] == 11).all() and (f[2:7, 2:7] == 12).all() and f[4, 4] == 12


def test_two_pits_sharing_a_saddle():
    #            rim  pit  saddle pit  rim
    z = arr([[9, 9, 9, 9, 9],
             [9, 1, 6, 2, 7],
             [9, 9, 9, 9, 9]])
    f = fm.fill(z, 4)
    assert f[1].tolist() == [9, 7, 7, 7, 7]         # both drain over the east rim of 7; the saddle of 6 is under water
    z[1, 4] = 3
    assert fm.fill(z, 4)[1].tolist() == [9, 6, 6, 3, 3]     # the east pit now drains at 3, the west one over the saddle
    labels, n = rm.label(np.array(fm.depth(fm.fill(z, 4), z)) > 0, 4)
    assert n == 2
    b = fm.basins(labels, n, z, fm.fill(z, 4), 4)
    assert [(int(r["level_min"]), int(r["pour_at"]), int(r["depth_max"]), int(r["deepest_at"])) for r in b] == [(6, 7, 5, 6), (3, 9, 1, 8)]


def test_a_plateau_has_no_depression():
    z = np.full((6, 7), 4, np.int32)
    z[2:4, 2:5] = 9
    for conn in (4, 8):
        assert (fm.fill(z, conn) == z).all()


def test_a_pit_open_to_the_edge_through_a_notch():
    z = np.full((5, 6), 8, np.int32)
    z[1:4, 1:5] = 2
    z[2, 5] = 3
    f = fm.fill(z, 4)
    assert (f[1:4, 1:5] == 3).all() and f[2, 5] == 3 and f[0, 0] == 8
    z[2, 5] = 1                     # a notch below the floor: nothing is closed
    assert (fm.fill(z, 4) == z).all()


def test_a_diagonal_gap_drains_at_eight_and_not_at_four():
    z = arr([[9, 9, 9, 9],
             [9, 1, 9, 9],
             [9, 9, 2, 9],
             [9, 9, 9, 2]])
    assert fm.fill(z, 8)[1, 1] == 2 and fm.fill(z, 8)[2, 2] == 2
    assert fm.fill(z, 4)[1, 1] == 9 and fm.fill(z, 4)[2, 2] == 9


def test_a_pit_astride_the_seam():
    z = np.full((5, 6), 9, np.int32)
    z[2, 5] = z[2, 0] = 1
    z[3, 0] = 4
    z[4, 0] = 4
    f = fm.fill(z, 4, wrap=True)
    assert f[2, 5] == 4 and f[2, 0] == 4 and f[3, 0] == 4       # one pit across the seam, out through the south row
    g = fm.fill(z, 4, wrap=False)
    assert (g == z).all()                                       # without wrap both halves lie on the edge
    labels, n = rm.label(np.array(fm.depth(f, z)) > 0, 4, True)
    assert n == 1 and fm.basins(labels, n, z, f, 4, True)[0]["count"] == 2


def test_an_outlet_table_inside_a_pit():
    z = np.full((5, 5), 9, np.int32)
    z[1:4, 1:4] = 3
    z[2, 2] = 1
    t = np.zeros((5, 5), np.uint8)
    t[2, 2] = 1
    assert (fm.fill(z, 8, table=t) == z).all()                          # the sink drains the whole floor
    t[2, 2], t[1, 1] = 0, 1
    assert fm.fill(z, 8, table=t)[2, 2] == 3                            # only the deepest node stays closed, up to the floor
    f = fm.fill(z, 8, edge_outlets=False, table=np.zeros((5, 5), np.uint8))
    assert (f == fm.NONE).all()                                         # no outlet at all
    assert (np.array(fm.depth(f, z)) == fm.NONE - z).all()


# ---- the identities
def identities(z, conn, wrap, edge, table):
    rows, cols = z.shape
    f = fm.fill(z, conn, wrap, edge, table)
    assert (f == jacobi(z, conn, wrap, edge, table)).all()
    o = fm.outlets(rows, cols, wrap, edge, table)
    if not o.any():
        assert (f == fm.NONE).all()
        return 0
    d = np.array(fm.depth(f, z))
    assert (d >= 0).all() and (f[o] == z[o]).all() and not (d[o] > 0).any()
    for i, j in zip(*np.nonzero(d > 0)):
        nb = list(fm.neighbours(i, j, rows, cols, conn, wrap))
        assert min(f[a, b] for a, b in nb) == f[i, j]
        assert all(f[a, b] == f[i, j] for a, b in nb if d[a, b] > 0)
    labels, n = rm.label(d > 0, conn, wrap)
    b = fm.basins(labels, n, z, f, conn, wrap)
    for r in b:
        assert r["level_min"] == r["level_max"] == r["pour_level"] and r["pour_at"] >= 0 and r["depth_max"] > 0
        assert labels.reshape(-1)[r["pour_at"]] == -1 and f.reshape(-1)[r["pour_at"]] == r["level_min"]
    return int((d > 0).sum())


@pytest.mark.parametrize("seed", range(6))
def test_the_identities_on_random_lattices(seed):
    rng = np.random.default_rng(300 + seed)
    nodes = 0
    for _ in range(10):
        rows, cols = int(rng.integers(1, 9)), int(rng.integers(3, 11))
        wrap, conn, edge = bool(rng.integers(0, 2)), int(rng.choice([4, 8])), bool(rng.integers(0, 4))
        z = rng.integers(-4, 5, (rows, cols)).astype(np.int32)
        table = (rng.random((rows, cols)) < 0.1).astype(np.uint8) if (not edge or rng.integers(0, 2)) else None
        nodes += identities(z, conn, wrap, edge, table)
    assert nodes > 0


def test_the_built_lattices_do_what_their_names_say():
    for transposed in (False, True):
        z, conn, wrap, edge, t = fc.serpentine(64, 8, transposed)
        f = fm.fill(z, conn, wrap, edge, t)
        assert (f[z < fc.WALL] == 5).all() and (f[z == fc.WALL] == fc.WALL).all() and (z < fc.WALL).sum() > 64 * 64 // 2 - 3 * 64
    for kind in ("main", "anti", "wrapped"):
        z, conn, wrap, edge, t = fc.diagonal(64, 8, kind)
        assert (fm.fill(z, 8, wrap, edge, t)[z < fc.WALL] == 5).all()
        f4 = fm.fill(z, 4, wrap, edge, t)
        assert (f4[(z < fc.WALL) & (t == 0)] == fc.WALL).all() and f4[t != 0].tolist() == [5]
    z, conn, wrap, edge, t = fc.flat_basin(64, 4)
    assert (fm.fill(z, 4)[1:-1, 1:-1] == 7).all()
    z = fc.checkerboard(6, 7, 4)[0]
    assert (fm.fill(z, 4)[1:-1, 1:-1] == 10).all() and (fm.fill(z, 8) == z).all()


def test_the_basin_reducer_on_a_callers_labels():
    z = arr([[5, 5, 5, 5], [5, 1, 2, 5], [5, 5, 5, 5]])
    f = fm.fill(z, 4)
    labels = arr([[0, 0, -1, 2], [0, 2, 2, -1], [-1, -1, -1, 0]])
    b = fm.basins(labels, 4, z, f, 4, False, [1, 2 ** 32 - 1, 3])
    assert b[0].tolist() == (1 + 1 + 2 ** 32 - 1 + 3, 0, 4, 5, 5, 0, 0, 2, 5, 0)
    assert b[2].tolist() == (1 + 2 * (2 ** 32 - 1), (2 ** 32 - 1) * 7, 3, 5, 5, 4, 5, 1, 5, 0)
    assert b[1].tolist() == (0, 0, 0, 2 ** 31 - 1, -2 ** 31, 0, -1, -1, 2 ** 31 - 1, 0) and b[3].tolist() == b[1].tolist()
    whole = fm.basins(np.zeros((3, 4), np.int32), 1, z, f, 8)
    assert whole[0]["pour_at"] == -1 and whole[0]["pour_level"] == 2 ** 31 - 1 and whole[0]["count"] == 12
    big = fm.basins(arr([[0, 0, 0]]), 1, arr([[-2 ** 30, 0, 0]]), arr([[fm.NONE] * 3]), 4, False, [2 ** 32 - 1])
    assert big[0]["volume"] == ((2 ** 32 - 1) * (2 ** 31 - 1 + 2 * (2 ** 31 - 1))) % 2 ** 64 and big[0]["depth_max"] == 2 ** 31 - 1


# ---- the Python surface
def test_quantise_heights():
    q = bs.quantise_heights([[0.0, 0.005, 0.015, -0.025], [1.234, -1e7, 2.0 ** 30 * 0.01, 0.0249999]])
    assert q.dtype == np.int32 and q.tolist() == [[0, 0, 2, -2], [123, -10 ** 9, 2 ** 30, 2]]       # half to even
    assert bs.quantise_heights([1000.0, -3.0], 0.5).tolist() == [2000, -6]
    for bad in ([np.nan], [np.inf], [2.0 ** 30 * 0.01 + 0.01], [-1.1e7]):
        with pytest.raises(ValueError):
            bs.quantise_heights(bad)
    with pytest.raises(ValueError):
        bs.quantise_heights([1.0], 0.0)


def test_fillmap_accessors():
    z = arr([[5, 5, 5], [5, 1, 5], [5, 5, 5]])
    m = bs.FillMap(z, fm.fill(z, 8), unit_m=0.5, connectivity=8, wrap=False)
    assert m.depth().dtype == np.int32 and m.depth()[1, 1] == 4 and m.depth().sum() == 4
    assert m.depth_m()[1, 1] == 2.0 and m.mask().tolist() == [[0, 0, 0], [0, 1, 0], [0, 0, 0]] and m.mask().dtype == np.uint8
    assert m.mask(2.0).sum() == 0 and m.mask(1.9).sum() == 1
    none = bs.FillMap(arr([[-2 ** 30]]), arr([[bs.FILL_NONE]]))
    assert none.depth()[0, 0] == 2 ** 31 - 1
    with pytest.raises(ValueError):
        none.depth_m()
    with pytest.raises(ValueError):
        bs.FillMap(z, z[:2])


def test_basin_dtype_mirrors_the_struct():
    assert C.sizeof(_lib.MrtxBasin) == 48 and bs.BASIN_DTYPE.itemsize == 48 and fm.BASIN == bs.BASIN_DTYPE
    for name, ctype in _lib.MrtxBasin._fields_:
        f = getattr(_lib.MrtxBasin, name)
        assert bs.BASIN_DTYPE.fields[name][1] == f.offset and bs.BASIN_DTYPE.fields[name][0].itemsize == f.size, name
        assert (bs.BASIN_DTYPE.fields[name][0].kind == "i") == (ctype is C.c_int32), name
    assert C.sizeof(_lib.MrtxFill) == 24
    assert [n for n, _ in _lib.MrtxFill._fields_] == ["rows", "cols", "wrap", "connectivity", "edge_outlets", "reserved"]
    assert _lib.FILL_NONE == fm.NONE == 2 ** 31 - 1 and _lib.FILL_ZMAX == fm.ZMAX == 2 ** 30


# ---- the refusals come before any device call: on a machine without a GPU each still gives its own text
@pytest.fixture
def ctx(native_lib):
    """A context handle; without a GPU mrtx_create stops at its first HIP call but hands the context out."""
    c = C.c_void_p()
    rc = native_lib.mrtx_create(C.byref(_lib.MrtxConfig(0, 16, 16, 0, 1, 0, 0)), C.byref(c))
    assert rc in (0, -2) and c.value
    yield c
    native_lib.mrtx_destroy(c)


def test_every_refusal_comes_before_any_device_call(native_lib, ctx, monkeypatch):
    monkeypatch.delenv("MOONRT_FILL", raising=False)
    z, outlet, fill, labels, out = fc.refusal_tables()
    base = 1 << 40                      # never dereferenced: a device call with it, or without a device, would not give -1
    assert native_lib.mrtx_fill(None, None, None, None, None, None, None, None, None, None) == -1
    assert native_lib.mrtx_fill_basins(None, 8, 9, 0, 8, None, None, 0, None, None, None, None, None, None, None, None) == -1
    for text, kw in fc.fill_refusals(z, outlet, fill, base):
        fc.assert_refused(native_lib, ctx, fc.fill_call, text, kw, (fill,))
    for text, kw in fc.basins_refusals(labels, z, fill, out, base):
        fc.assert_refused(native_lib, ctx, fc.basins_call, text, kw, (out,))
    # an unknown value of the variant switch, by name; the two known ones are not refused for it
    F = dict(z=z, fill=fill)
    for bad in ("fast", "", "Sweep"):
        monkeypatch.setenv("MOONRT_FILL", bad)
        fc.assert_refused(native_lib, ctx, fc.fill_call, "MOONRT_FILL must be tiles or sweep", dict(F, f=fc.block()), (fill,))
    for good in ("tiles", "sweep"):
        monkeypatch.setenv("MOONRT_FILL", good)
        fc.assert_refused(native_lib, ctx, fc.fill_call, "reserved must be 0", dict(F, f=fc.block(reserved=1)), (fill,))


# ---- the tool's CSV
def test_the_tools_csv_on_a_synthetic_catalogue():
    import csv
    import io
    import depression_catalogue as tool
    z = np.full((6, 8), 50, np.int32)
    z[1:3, 1:3] = 10            # a bowl of four nodes, 40 deep
    z[4, 5] = 20                # a pit of one node
    z[0:4, 5] = 45              # a trench from its north side to the edge: it pours over node (3, 5) at 45, 25 deep
    f = fm.fill(z, 4)
    labels, n = rm.label(np.array(fm.depth(f, z)) > 0, 4)
    weights = [100, 100, 100, 200, 200, 200]
    table = fm.basins(labels, n, z, f, 4, False, weights)
    lat, lon = 10.0 - np.arange(6), 100.0 + np.arange(8)
    rows = list(tool.catalogue_rows(table, 8, lat, lon, 0.5, 2.0))
    assert rows == [[0, repr(4 * 100 * 2.0 / 1e6), 4, repr(25.0), repr(20.0), repr(9.0), repr(101.0), repr(10.0), repr(101.0),
                     repr(400 * 40 * 2.0 * 0.5)],
                    [1, repr(200 * 2.0 / 1e6), 1, repr(22.5), repr(12.5), repr(6.0), repr(105.0), repr(7.0), repr(105.0),
                     repr(200 * 25 * 2.0 * 0.5)]]
    buf = io.StringIO()
    out = csv.writer(buf)
    out.writerow(tool.HEADER)
    out.writerows(rows)
    back = list(csv.reader(io.StringIO(buf.getvalue())))
    assert back[0] == tool.HEADER and len(back) == 3 and float(back[1][9]) > float(back[2][9]) and back[2][0] == "1"
    # a basin that covers the whole lattice has no pour point: empty columns
    whole = fm.basins(np.zeros((6, 8), np.int32), 1, z, f, 4)
    assert list(tool.catalogue_rows(whole, 8, lat, lon, 1.0, 1.0))[0][7:9] == ["", ""]
