"""The depression hierarchy without a GPU: the sweep of tests/bowls_model.py against cases worked by
hand, the three identities on random lattices against tests/fill_model.py, the record's layout, BowlTree's selections and label
tables, every refusal that needs no device, and the tool's CSV."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import bowls_cases as bc
import bowls_model as bm
import fill_model as fm
from moonrtx_amd import _lib
from moonrtx_amd import basins as bs

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

NONE = 2 ** 31 - 1


def arr(rows):
    return np.array(rows, np.int32)


def rec(t, b, *names):
    return tuple(int(t[b][n]) for n in names)


# ---- the model against cases worked by hand
def test_a_single_pit():
    z = arr([[5, 5, 5, 5, 5], [5, 4, 3, 4, 5], [5, 4, 1, 4, 5], [5, 4, 4, 4, 5], [5, 5, 5, 5, 5]])
    for conn in (4, 8):
        t, lab = bm.bowls(z, conn)
        assert len(t) == 1
        # born at the centre, spills at the first edge node in index order that touches the inner ring: node 1 at 8, node 5 at 4
        spill = 0 if conn == 8 else 1
        assert rec(t, 0, "born_at", "born_level", "floor_at", "floor_level", "spill_at", "spill_level", "parent") == (12, 1, 12, 1, spill, 5, -1)
        assert rec(t, 0, "count", "own_count", "weight", "volume", "n_children", "n_leaves") == (9, 9, 9, 4 + 2 + 7, 0, 1)
        assert (lab[1:4, 1:4] == 0).all() and (lab == -1).sum() == 16


def test_a_pit_inside_a_pit():
    z = np.full((9, 9), 20, np.int32)
    z[1:8, 1:8] = 10            # the outer bowl's floor
    z[2:7, 2:7] = 12            # a rim inside it
    z[3:6, 3:6] = 2             # the inner bowl
    z[1, 1] = 9                 # the outer floor's own lowest node
    t, lab = bm.bowls(z, 8)
    # leaves: the inner bowl (born at 2) and the outer ring's floor (born at 9); they meet on the rim at 12; the meta spills at 20
    assert len(t) == 3
    assert rec(t, 0, "born_at", "born_level", "spill_level", "parent", "count") == (3 * 9 + 3, 2, 12, 2, 9)
    assert rec(t, 1, "born_at", "born_level", "spill_level", "parent", "count") == (1 * 9 + 1, 9, 12, 2, 24)
    assert rec(t, 2, "born_at", "born_level", "floor_at", "floor_level", "spill_level", "parent", "n_children", "n_leaves") == (
        2 * 9 + 2, 12, 3 * 9 + 3, 2, 20, -1, 2, 2)
    assert rec(t, 2, "count", "own_count") == (49, 16) and int(t[2]["volume"]) == 9 * 18 + 16 * 8 + 23 * 10 + 11
    assert (lab[3:6, 3:6] == 0).all() and lab[1, 1] == 1 and lab[2, 2] == 2 and lab[0, 0] == -1


def test_twins_sharing_a_saddle_inside_a_closed_basin():
    z = arr([[9, 9, 9, 9, 9, 9, 9],
             [9, 1, 6, 4, 6, 2, 9],
             [9, 9, 9, 9, 9, 9, 9]])
    t, lab = bm.bowls(z, 4)
    # the pits at 1 and 2 rise to 6 on their own; the saddle node (4) is a third minimum at connectivity 4: it joins the first twin at
    # node 9 (height 6), then the second at node 11
    assert len(t) == 5 and [int(v) for v in t["born_level"]] == [1, 2, 4, 6, 6]
    z[1, 3] = 7                 # now a saddle proper: three records
    t, lab = bm.bowls(z, 4)
    assert len(t) == 3
    assert rec(t, 0, "born_at", "spill_at", "spill_level", "parent", "count", "volume") == (8, 10, 7, 2, 2, 6 + 1)
    assert rec(t, 1, "born_at", "spill_at", "spill_level", "parent", "count", "volume") == (12, 10, 7, 2, 2, 5 + 1)
    assert rec(t, 2, "born_at", "floor_at", "spill_level", "parent", "count", "own_count", "n_children", "volume") == (10, 8, 9, -1, 5, 1, 2,
                                                                                                            8 + 3 + 2 + 3 + 7)
    assert lab[1].tolist() == [-1, 0, 0, 2, 1, 1, -1]


def test_a_four_way_saddle():
    plus = arr([[9, 9, 9, 9, 9],
                [9, 9, 1, 9, 9],
                [9, 2, 5, 3, 9],
                [9, 9, 4, 9, 9],
                [9, 9, 9, 9, 9]])
    t, lab = bm.bowls(plus, 4)
    assert len(t) == 5 and rec(t, 4, "born_at", "n_children", "n_leaves", "floor_at", "count", "own_count") == (12, 4, 4, 7, 5, 1)
    assert (t["parent"][:4] == 4).all() and (t["spill_at"][:4] == 12).all() and t["parent"][4] == -1
    diag = arr([[9, 9, 9, 9, 9],
                [9, 1, 9, 2, 9],
                [9, 9, 5, 9, 9],
                [9, 3, 9, 4, 9],
                [9, 9, 9, 9, 9]])
    t, lab = bm.bowls(diag, 8)
    assert len(t) == 5 and rec(t, 4, "born_at", "n_children", "n_leaves", "floor_at") == (12, 4, 4, 6)
    t4, _ = bm.bowls(diag, 4)
    assert len(t4) == 5 and (t4["parent"] == -1).all()           # at connectivity 4 they are five separate pits


def test_a_diagonal_gap_drains_at_eight_and_not_at_four():
    z = arr([[9, 9, 9, 9, 0],
             [9, 1, 9, 0, 9],
             [9, 9, 2, 9, 9],
             [9, 9, 9, 9, 9]])
    # (1, 1) - (2, 2) - (1, 3) - (0, 4): a diagonal chain to the edge outlet (0, 4)
    t8, lab8 = bm.bowls(z, 8)
    t4, lab4 = bm.bowls(z, 4)
    assert rec(t8, 0, "born_at", "spill_at", "spill_level", "count") == (6, 12, 2, 1) and lab8[2, 2] == -1
    assert len(t4) == 3 and (t4["spill_level"] == 9).all() and lab4[2, 2] == 2


def test_a_u_shaped_flat():
    z = arr([[9, 9, 9, 9, 9],
             [9, 3, 9, 3, 9],
             [9, 3, 3, 3, 9],
             [9, 9, 9, 9, 9]])
    t, lab = bm.bowls(z, 4)
    # nodes 6 and 8 have a lower index than all their equal neighbours: two zero-depth leaves; 11 and 12 join the first, and the
    # two meet at node 13
    assert len(t) == 3
    assert rec(t, 0, "born_at", "spill_at", "spill_level", "volume", "count") == (6, 13, 3, 0, 3)
    assert rec(t, 1, "born_at", "spill_at", "spill_level", "volume", "count") == (8, 13, 3, 0, 1)
    assert rec(t, 2, "born_at", "born_level", "floor_at", "n_children", "count", "spill_level", "volume") == (13, 3, 6, 2, 5, 9, 30)
    tree = bs.BowlTree(t, lab, z, 1.0, 4)
    assert tree.depth().tolist() == [0, 0, 6] and tree.select(min_depth_m=0.5).tolist() == [False, False, True]


def test_a_pit_astride_the_seam():
    z = np.full((5, 6), 9, np.int32)
    z[2, 0], z[2, 5] = 1, 2
    t, lab = bm.bowls(z, 4, wrap=True)
    assert len(t) == 1 and rec(t, 0, "born_at", "count", "volume", "spill_level") == (12, 2, 8 + 7, 9)
    t, lab = bm.bowls(z, 4, wrap=False)
    assert len(t) == 0 and (lab == -1).all()                    # without wrap both lie on the edge


def test_an_outlet_inside_a_pit_and_a_minimum_that_is_an_outlet():
    z = np.full((7, 7), 9, np.int32)
    z[2:5, 2:5] = 3
    z[3, 3] = 1
    t, _ = bm.bowls(z, 8)
    assert len(t) == 1 and t[0]["count"] == 9
    # an outlet on the pit's floor: the minimum rises to it and spills there, one node, volume 2
    t, lab = bm.bowls(z, 8, table=bc.one_outlet(z.shape, (2, 2)))
    assert len(t) == 1 and rec(t, 0, "born_at", "spill_at", "spill_level", "count", "volume") == (24, 16, 3, 1, 2)
    assert (lab >= 0).sum() == 1
    # the minimum itself an outlet: no bowl at all
    t, lab = bm.bowls(z, 8, table=bc.one_outlet(z.shape, (3, 3)))
    assert len(t) == 0 and (lab == -1).all()


def test_no_outlet_at_all_and_outlets_only():
    z = arr([[5, 5, 5], [5, 1, 5], [5, 5, 2]])
    t, lab = bm.bowls(z, 4, edge_outlets=False, table=np.zeros((3, 3), np.uint8))
    # the pits at 1 and 2, and node 0 of the flat at 5, which has a lower index than its equal neighbours: three leaves; node 1
    # joins the flat to the first pit, node 5 the second pit to both; the last meta never spills
    assert len(t) == 5 and [int(v) for v in t["born_at"]] == [4, 8, 0, 1, 5] and t["parent"].tolist() == [3, 4, 3, 4, -1]
    assert rec(t, 4, "spill_at", "spill_level", "volume", "count", "parent", "n_leaves") == (-1, NONE, 0, 9, -1, 3)
    assert (lab >= 0).all()
    t, lab = bm.bowls(z, 4, edge_outlets=False, table=np.zeros((3, 3), np.uint8), invert=True)
    assert t[-1]["spill_level"] == -NONE and t[-1]["spill_at"] == -1
    t, lab = bm.bowls(z, 8, table=np.ones((3, 3), np.uint8))
    assert len(t) == 0 and (lab == -1).all()


def test_invert_gives_peaks_and_prominence():
    z = np.zeros((5, 9), np.int32)
    z[2, 2] = 7
    t, lab = bm.bowls(z, 8, invert=True)
    # the flat around it is an earlier "pit" of -z only where a node has no lower-index equal neighbour: none off the edge
    peak = [b for b in range(len(t)) if t[b]["floor_level"] == 7]
    assert len(peak) == 1 and rec(t, peak[0], "floor_at", "floor_level", "spill_level", "count", "volume") == (20, 7, 0, 1, 7)
    z[2, 6], z[2, 3:6] = 9, 4                                   # twin peaks joined by a ridge at 4
    t, lab = bm.bowls(z, 8, invert=True)
    by_summit = {int(t[b]["floor_level"]): b for b in range(len(t)) if t[b]["n_children"] == 0}
    lo, hi = by_summit[7], by_summit[9]
    assert rec(t, lo, "spill_level", "spill_at") == (4, 2 * 9 + 5) and t[lo]["parent"] == t[hi]["parent"] >= 0
    top = int(t[lo]["parent"])
    assert rec(t, top, "floor_at", "floor_level", "spill_level", "n_children", "parent") == (2 * 9 + 6, 9, 0, 2, -1)
    tree = bs.BowlTree(t, lab, z, 1.0, 8, False, True)
    assert tree.depth()[lo] == 3 and tree.depth()[top] == 9     # prominences


# ---- the identities
def identities(z, conn, wrap, edge, table, weights):
    t, lab = bm.bowls(z, conn, wrap, edge, table, False, weights)
    tree = bs.BowlTree(t, lab, z, None, conn, wrap)
    f = fm.fill(z, conn, wrap, edge, table)
    rows, cols = z.shape
    # 1: the tie to the fill
    assert (tree.fill() == f).all()
    assert (f[lab == -1] == z[lab == -1]).all()
    w = np.ones(rows, np.int64) if weights is None else np.asarray(weights, np.int64)
    if not (f == fm.NONE).any():
        total = sum(int(w[i]) * int((f[i].astype(np.int64) - z[i]).sum()) for i in range(rows))
        assert sum(int(v) for v in t["volume"][tree.roots()]) == total
    # 2: the catchment rule
    out = fm.outlets(rows, cols, wrap, edge, table).reshape(-1)
    zz = z.reshape(-1).tolist()
    key = lambda v: (zz[v], v)
    leaf_at = {int(t[b]["born_at"]): b for b in range(len(t)) if t[b]["n_children"] == 0}
    for v in range(rows * cols):
        m = v
        while True:
            if out[m]:
                m = -1
                break
            nxt = min([m] + [a * cols + b for a, b in fm.neighbours(m // cols, m % cols, rows, cols, conn, wrap)], key=key)
            if nxt == m:
                break
            m = nxt
        want = -1
        if m >= 0:
            b = leaf_at[m]
            while b >= 0:
                s = int(t[b]["spill_at"])
                if key(int(t[b]["born_at"])) <= key(v) and (s < 0 or key(v) < key(s)):
                    want = b
                    break
                b = int(t[b]["parent"])
        assert lab.reshape(-1)[v] == want, v
    # 3: parents, and the sums of the children
    for name, own in (("count", t["own_count"].astype(object)), ("weight", None), ("n_leaves", None)):
        kids = [0] * len(t)
        for b in range(len(t)):
            p = int(t[b]["parent"])
            if p >= 0:
                assert p > b
                kids[p] += int(t[b][name])
        for b in range(len(t)):
            if name == "count":
                assert int(t[b]["count"]) == int(t[b]["own_count"]) + kids[b]
            elif name == "weight":
                mine = sum(int(w[i]) * int((lab[i] == b).sum()) for i in range(rows))
                assert int(t[b]["weight"]) == mine + kids[b]
            else:
                assert int(t[b]["n_leaves"]) == (1 if t[b]["n_children"] == 0 else kids[b])


@pytest.mark.parametrize("seed", range(8))
def test_the_identities_on_random_lattices(seed):
    rng = np.random.default_rng(100 + seed)
    for _ in range(6):
        rows, cols = int(rng.integers(1, 14)), int(rng.integers(3, 14))
        conn, wrap, edge = int(rng.choice([4, 8])), bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
        z = rng.integers(0, int(rng.choice([1, 2, 5, 50])) + 1, (rows, cols)).astype(np.int32)
        table = (rng.random((rows, cols)) < 0.06).astype(np.uint8) if (not edge or rng.integers(0, 2)) else None
        weights = rng.integers(1, 100, rows) if rng.integers(0, 2) else None
        identities(z, conn, wrap, edge, table, weights)


def test_invert_is_the_sweep_of_the_negated_heights():
    rng = np.random.default_rng(7)
    z = rng.integers(-9, 10, (12, 15)).astype(np.int32)
    a, la = bm.bowls(z, 8, True, True, None, True)
    b, lb = bm.bowls(-z, 8, True, True, None, False)
    assert (la == lb).all()
    for name in bm.BOWL.names:
        flip = name in ("floor_level", "born_level", "spill_level")
        assert (a[name] == (-b[name] if flip else b[name])).all(), name


def test_the_built_lattices_do_what_their_names_say():
    t, lab = bm.bowls(*bc.staircase(5, 4))
    # five pits, four metas, and last the zero-depth leaf of the flat of walls, born at node 0
    assert len(t) == 10 and t["n_leaves"][8] == 5 and (t["n_children"][5:9] == 2).all() and t["born_at"][9] == 0
    assert t["parent"].tolist() == [8, 7, 6, 5, 5, 6, 7, 8, -1, -1]
    z, conn, wrap, edge, table = bc.serpentine(16, 4)
    assert (z < bc.WALL).sum() > 16 * 5 and table.sum() == 1
    t, lab = bm.bowls(z, conn, wrap, edge, table)
    assert len(t) >= 2
    t, lab = bm.bowls(*bc.pit_grid(16, 5))
    assert (t["n_children"] == 0).sum() >= 49


# ---- the record and the tree
def test_bowl_dtype_mirrors_the_struct():
    assert C.sizeof(_lib.MrtxBowl) == 64 and bs.BOWL_DTYPE.itemsize == 64 and bm.BOWL == bs.BOWL_DTYPE
    for name, ctype in _lib.MrtxBowl._fields_:
        f = getattr(_lib.MrtxBowl, name)
        assert bs.BOWL_DTYPE.fields[name][1] == f.offset and bs.BOWL_DTYPE.fields[name][0].itemsize == f.size, name
        assert (bs.BOWL_DTYPE.fields[name][0].kind == "i") == (ctype is C.c_int32), name
    assert [n for n, _ in _lib.MrtxBowl._fields_] == list(bs.BOWL_DTYPE.names)
    assert C.sizeof(_lib.MrtxBowls) == 32
    assert [n for n, _ in _lib.MrtxBowls._fields_] == ["rows", "cols", "wrap", "connectivity", "edge_outlets", "invert", "reserved"]


def test_bowltree_select_relabel_and_fill():
    rng = np.random.default_rng(9)
    z = rng.integers(0, 30, (24, 31)).astype(np.int32)
    w = rng.integers(1, 9, 24)
    t, lab = bm.bowls(z, 8, False, True, None, False, w)
    tree = bs.BowlTree(t, lab, z, 0.5, 8)
    assert tree.n == len(t) > 10 and (tree.fill() == fm.fill(z, 8)).all()
    root = tree.root_of()
    level = tree.level()
    for b in range(tree.n):
        chain = [b]
        while t[chain[-1]]["parent"] >= 0:
            chain.append(int(t[chain[-1]]["parent"]))
        assert root[b] == chain[-1] and level[b] == len(chain) - 1
        assert tree.children(b).tolist() == [k for k in range(tree.n) if t[k]["parent"] == b]
    assert tree.roots().tolist() == [b for b in range(tree.n) if t[b]["parent"] < 0]
    assert (tree.depth() == np.abs(t["spill_level"].astype(np.int64) - t["floor_level"])).all()
    keep = tree.select(min_depth_m=2.0, min_area=6, min_count=2)
    assert keep.tolist() == [bool(abs(int(r["spill_level"]) - int(r["floor_level"])) * 0.5 >= 2.0 and r["weight"] >= 6 and r["count"] >= 2)
                             for r in t]
    assert 0 < keep.sum() < tree.n and tree.select().all()
    with pytest.raises(ValueError):
        bs.BowlTree(t, lab, z).select(min_depth_m=1.0)
    for innermost in (True, False):
        table, bowl_of = tree.relabel(keep, innermost)
        assert table.dtype == np.int32 and table.shape == z.shape
        for v in range(z.size):
            b, found = int(lab.reshape(-1)[v]), -1
            while b >= 0:
                if keep[b] and (found < 0 or not innermost):
                    found = b
                b = int(t[b]["parent"])
            got = int(table.reshape(-1)[v])
            assert (bowl_of[got] if got >= 0 else -1) == found, (v, innermost)
        assert (np.diff(bowl_of) > 0).all() and keep[bowl_of].all()
    none, bowl_of = tree.relabel(np.zeros(tree.n, bool))
    assert (none == -1).all() and len(bowl_of) == 0
    with pytest.raises(ValueError):
        tree.relabel(np.zeros(3, bool))
    with pytest.raises(ValueError):
        bs.BowlTree(t, None, z).relabel(keep)
    empty = bs.BowlTree(np.zeros(0, bs.BOWL_DTYPE), np.full((3, 4), -1, np.int32), np.zeros((3, 4), np.int32))
    assert (empty.fill() == 0).all() and (empty.relabel(np.zeros(0, bool))[0] == -1).all() and len(empty.roots()) == 0


# ---- the refusals come before any device call: on a machine without a GPU each still gives its own text
@pytest.fixture
def ctx(native_lib):
    """A context handle; without a GPU mrtx_create stops at its first HIP call but hands the context out."""
    c = C.c_void_p()
    rc = native_lib.mrtx_create(C.byref(_lib.MrtxConfig(0, 16, 16, 0, 1, 0, 0)), C.byref(c))
    assert rc in (0, -2) and c.value
    yield c
    native_lib.mrtx_destroy(c)


def test_every_refusal_comes_before_any_device_call(native_lib, ctx):
    z, outlet, rec_, lab = bc.refusal_tables()
    base = 1 << 40                      # never dereferenced: a device call with it, or without a device, would not give -1
    assert native_lib.mrtx_bowls(None, None, None, None, None, None, None, None, None, 0, None, None, None, None, None) == -1
    cases = bc.refusals(z, outlet, rec_, lab, base)
    assert len({text for text, _ in cases}) >= 20
    for text, kw in cases:
        bc.assert_refused(native_lib, ctx, text, kw, (rec_, lab))


# ---- the tool's CSV
def test_the_tools_csv_on_a_small_tree():
    import bowl_catalogue as tool
    z = np.full((5, 9), 50, np.int32)
    i, j = np.indices((3, 7))
    z[1:4, 1:8] = 30 + np.minimum(abs(i - 1) + abs(j - 1), abs(i - 1) + abs(j - 5))    # a basin floor that falls towards two craters
    z[2, 2], z[2, 6] = 10, 20   # the craters, each one node; the floors meet at (2, 4), height 32
    w = [100, 100, 200, 200, 200]
    t, lab = bm.bowls(z, 4, False, True, None, False, w)
    assert len(t) == 3
    tree = bs.BowlTree(t, lab, z, 0.5, 4)
    lat, lon = 10.0 - np.arange(5), 100.0 + np.arange(9)
    keep = tree.select(min_depth_m=1.0)
    rows = list(tool.catalogue_rows(tree, keep, lat, lon, 2.0))
    assert rows[0][:10] == [0, 2, 1, repr(8.0), repr(102.0), repr(5.0), repr(8.0), repr(104.0), repr(16.0), repr(11.0)]
    assert rows[1][:10] == [1, 2, 1, repr(8.0), repr(106.0), repr(10.0), repr(8.0), repr(104.0), repr(16.0), repr(6.0)]
    assert rows[2][:10] == [2, -1, 0, repr(8.0), repr(102.0), repr(5.0), repr(10.0), repr(101.0), repr(25.0), repr(20.0)]
    assert rows[2][10:] == [repr(int(t[2]["weight"]) * 2.0 / 1e6), repr(int(t[2]["volume"]) * 2.0 * 0.5), 2]
    assert int(t[2]["weight"]) == 7 * (100 + 200 + 200) and rows[0][12] == 1
    # the deeper crater alone: its kept parent is none, its level 0
    only = list(tool.catalogue_rows(tree, np.array([True, False, False]), lat, lon, 2.0))
    assert len(only) == 1 and only[0][:3] == [0, -1, 0]
    assert len(tool.HEADER) == len(tool.PEAK_HEADER) == len(rows[0]) == 13
