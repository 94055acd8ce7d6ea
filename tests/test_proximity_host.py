"""The host side of the proximity maps, without a GPU: node positions by hand and at the 2^29 bound,
the ProximityMap's distances, allocation and integer buffer rule, the record sizes, and the model (tests/proximity_model.py)
against cases worked by hand."""
import ctypes as C
import math

import numpy as np
import pytest

import proximity_model as pm
from moonrtx_amd import _lib
from moonrtx_amd import regions as rg

NONE = 2 ** 64 - 1


def test_record_sizes():
    assert rg.REACH_DTYPE.itemsize == 32 and C.sizeof(_lib.MrtxRegionReach) == 32 and C.sizeof(_lib.MrtxProximity) == 16
    assert [n for n, _ in _lib.MrtxRegionReach._fields_] == list(rg.REACH_DTYPE.names) == list(pm.REACH.names)
    assert [rg.REACH_DTYPE.fields[n][1] for n in rg.REACH_DTYPE.names] == [0, 8, 16, 20, 24, 28]
    assert (_lib.PROX_TO_SET, _lib.PROX_TO_OUTSIDE) == (0, 1)
    assert rg.COORD_MAX == pm.COORD_MAX == 2 ** 29 and int(rg.NO_FEATURE) == NONE
    assert "mrtx_proximity" in _lib.SIGNATURES and "mrtx_regions_reach" in _lib.SIGNATURES


def test_node_positions_by_hand():
    """A 2 x 4 DEM: latitudes +-45 degrees, longitudes -135, -45, 45, 135; cos 45 cos 45 = 1 / 2 and sin 45 = 0.70710678."""
    p = rg.node_positions((0, 0, 2, 4), (2, 4), radius_m=1000.0, unit_m=1.0)
    assert p.shape == (2, 4, 3) and p.dtype == np.int32
    assert p[0, 0].tolist() == [-500, -500, 707]
    assert p[0, 1].tolist() == [500, -500, 707]
    assert p[1, 2].tolist() == [500, 500, -707]
    assert p[1, 3].tolist() == [-500, 500, -707]
    # a height is added to the radius: 1100 / 2 = 550 and 1100 x 0.70710678 = 777.8
    q = rg.node_positions((0, 0, 2, 4), (2, 4), radius_m=1000.0, unit_m=1.0, heights_m=100.0)
    assert q[1, 2].tolist() == [550, 550, -778]
    h = np.zeros((2, 4))
    h[0, 1] = 100.0
    q = rg.node_positions((0, 0, 2, 4), (2, 4), radius_m=1000.0, unit_m=1.0, heights_m=h)
    assert q[0, 1].tolist() == [550, -550, 778] and q[0, 0].tolist() == [-500, -500, 707]
    # the unit divides: 0.5 m units double every coordinate (707.10678 x 2 = 1414.2)
    assert rg.node_positions((0, 0, 2, 4), (2, 4), 1000.0, 0.5)[0, 0].tolist() == [-1000, -1000, 1414]
    # stride and a column offset that wraps: columns 3, 5 mod 4 = 1
    q = rg.node_positions((1, 3, 1, 2, 2, 1), (2, 4), 1000.0, 1.0)
    assert q[0, 0].tolist() == [-500, 500, -707] and q[0, 1].tolist() == [500, -500, -707]


def test_node_positions_of_a_wrapped_polar_window():
    window = (21515, 0, 40, 3840 // 40, 480, 1)         # 96 columns at stride 480 go once round the 46080 columns
    with pytest.raises(ValueError, match="leave the DEM"):
        rg.node_positions(window, (23040, 46080))
    window = (21515, 0, 40, 96, 12, 1)
    H, W = 23040, 1152                                  # 96 columns at stride 12 go once round
    p = rg.node_positions(window, (H, W)).astype(np.int64)
    assert p.shape == (40, 96, 3) and np.abs(p).max() <= 2 ** 29
    # every node on the sphere to within the rounding, z from the row alone
    r = np.sqrt((p * p).sum(-1).astype(np.float64)) * 0.01
    assert np.abs(r - 1737400.0).max() < 0.02
    lat = 0.5 * math.pi - (21515 + 12 * np.arange(40) + 0.5) * (math.pi / H)
    assert np.array_equal(p[:, :, 2], np.broadcast_to(np.rint(1737400.0 * np.sin(lat) / 0.01).astype(np.int64)[:, None], (40, 96)))
    # column j + 48 lies across the axis: x and y change sign to within the rounding
    assert np.abs(p[:, :48, :2] + p[:, 48:, :2]).max() <= 1
    # the seam is no edge: columns 95 and 0 are as far apart as columns 0 and 1
    d_seam = ((p[:, 95] - p[:, 0]) ** 2).sum(-1)
    d_next = ((p[:, 1] - p[:, 0]) ** 2).sum(-1)
    assert np.abs(np.sqrt(d_seam) - np.sqrt(d_next)).max() <= 2.0


def test_node_positions_refuse_what_leaves_the_bound():
    # 2^29 units of 0.01 m are 5368709.12 m: a radius just inside fits (z = R sin 45 and x, y smaller), one 2 x 4 DEM row up
    ok = rg.node_positions((0, 0, 2, 4), (2, 4), radius_m=2 ** 29 * 0.01 * math.sqrt(2.0) * 0.999)
    assert np.abs(ok.astype(np.int64)).max() <= 2 ** 29
    with pytest.raises(ValueError, match="choose a larger unit"):
        rg.node_positions((0, 0, 2, 4), (2, 4), radius_m=2 ** 29 * 0.01 * math.sqrt(2.0) * 1.001)
    with pytest.raises(ValueError, match="choose a larger unit"):
        rg.node_positions((0, 0, 2, 4), (2, 4), unit_m=0.001)
    # the one node of a 1 x 1 DEM lies at lat = lon = 0, at (R, 0, 0) exactly: 2^29 is inside, 2^29 + 1 is not
    edge = rg.node_positions((0, 0, 1, 1), (1, 1), radius_m=float(2 ** 29), unit_m=1.0)
    assert edge[0, 0].tolist() == [2 ** 29, 0, 0]
    assert rg.node_positions((0, 0, 1, 1), (1, 1), radius_m=float(2 ** 29 - 1), unit_m=1.0, heights_m=1.0)[0, 0, 0] == 2 ** 29
    with pytest.raises(ValueError, match="choose a larger unit"):
        rg.node_positions((0, 0, 1, 1), (1, 1), radius_m=float(2 ** 29 + 1), unit_m=1.0)
    with pytest.raises(ValueError, match="choose a larger unit"):
        rg.node_positions((0, 0, 1, 1), (1, 1), radius_m=float(2 ** 29), unit_m=1.0, heights_m=1.0)
    with pytest.raises(ValueError):
        rg.node_positions((0, 0, 2, 4), (2, 4), heights_m=np.zeros((3, 4)))
    with pytest.raises(ValueError):
        rg.node_positions((0, 0, 3, 4), (2, 4))


def test_proximity_map_distances_and_allocation():
    nearest = np.array([[0, 0, -1], [5, 5, 5]], np.int32)
    dist2 = np.array([[0, 25, NONE], [9, 2, 3 * 2 ** 60]], np.uint64)
    m = rg.ProximityMap(nearest, dist2, 0.5)
    c = m.chord_m()
    assert c.dtype == np.float64
    assert c[0].tolist() == [0.0, 2.5, math.inf] and c[1, 0] == 1.5 and c[1, 1] == math.sqrt(2.0) * 0.5
    assert c[1, 2] == math.sqrt(3.0 * 2.0 ** 60) * 0.5
    a = m.arc_m(10.0)
    assert a[0, 0] == 0.0 and a[0, 2] == math.inf
    assert a[0, 1] == 2.0 * 10.0 * math.asin(2.5 / 20.0) and a[1, 0] == 20.0 * math.asin(1.5 / 20.0)
    assert a[1, 2] == 10.0 * math.pi                        # longer than the diameter: the half circle
    labels = np.array([[7, -1, -1], [-1, -1, 3]], np.int32)
    assert m.nearest_label(labels).tolist() == [[7, 7, -1], [3, 3, 3]]
    with pytest.raises(ValueError):
        m.nearest_label(labels[:1])
    with pytest.raises(ValueError, match="no unit"):
        rg.ProximityMap(nearest, dist2).chord_m()
    with pytest.raises(ValueError):
        rg.ProximityMap(nearest, dist2[:1])


def test_within_is_compared_in_integers():
    d2 = np.array([[0, 24, 25, 26, 2 ** 53 + 1, NONE]], np.uint64)
    m = rg.ProximityMap(np.array([[0, 0, 0, 0, 0, -1]], np.int32), d2, 1.0)
    assert m.within(5.0).tolist() == [[True, True, True, False, False, False]]          # 25 <= floor(5^2): the tie is inside
    assert m.within(4.999).tolist() == [[True, True, False, False, False, False]]
    assert m.within(0.0).tolist() == [[True, False, False, False, False, False]]
    assert m.within(-1.0).tolist() == [[False] * 6] and m.within(math.nan).tolist() == [[False] * 6]
    assert m.within(math.inf).tolist() == [[True] * 5 + [False]]                        # no feature: never within
    assert m.within(1e30).tolist() == [[True] * 5 + [False]]
    # beyond float64's integers the rule is still the integer one: 2^53 + 1 <= floor((2^26.5)^2) or not, by the float square
    t = math.sqrt(2.0 ** 53 + 2.0)
    assert m.within(t)[0, 4] == (2 ** 53 + 1 <= math.floor(t * t))
    # the unit divides the distance first
    half = rg.ProximityMap(np.zeros((1, 6), np.int32), d2, 0.5)
    assert half.within(2.5).tolist() == [[True, True, True, False, False, False]]
    assert np.array_equal(half.within(2.5)[:, :4], (half.chord_m() <= 2.5)[:, :4])


# ---- the model on cases worked by hand: a 3 x 3 lattice, node v = 3 i + j
def planar(a=1, b=1):
    i, j = np.mgrid[0:3, 0:3]
    return np.stack([j * a, i * b, np.zeros_like(i)], -1)


def test_model_tie_goes_to_the_least_index():
    lab = np.full((3, 3), -1, np.int32)
    lab[0, 1] = lab[1, 0] = lab[1, 2] = lab[2, 1] = 0       # features 1, 3, 5, 7: the centre is 1 from all four
    near, d2 = pm.proximity(lab, planar())
    assert near.tolist() == [[1, 1, 1], [3, 1, 5], [3, 7, 5]]
    assert d2.tolist() == [[1, 0, 1], [0, 1, 0], [1, 0, 1]]
    near, d2 = pm.proximity(lab, planar(), outside=True)    # features 0, 2, 4, 6, 8
    assert near.tolist() == [[0, 0, 2], [0, 4, 2], [6, 4, 8]]
    assert d2.tolist() == [[0, 1, 0], [1, 0, 1], [0, 1, 0]]
    # anisotropic spacing breaks the tie the other way: rows 3 apart, columns 1
    near, d2 = pm.proximity(np.array([[-1, -1, 0], [-1, -1, -1], [0, -1, -1]], np.int32), planar(1, 3))
    assert near[1].tolist() == [6, 2, 2] and d2[1].tolist() == [9, 10, 9]


def test_model_duplicate_positions():
    pos = planar()
    pos[2, 2] = pos[0, 1]                                   # node 8 sits on node 1
    lab = np.full((3, 3), -1, np.int32)
    lab[0, 1] = lab[2, 2] = 4                               # both twins are features: the lower index takes both
    near, d2 = pm.proximity(lab, pos)
    assert near.tolist() == [[1, 1, 1], [1, 1, 1], [1, 1, 1]] and d2[2, 2] == 0 and d2[0, 1] == 0
    lab[0, 1] = -1                                          # only the upper twin is: node 1 gets it at distance 0
    near, d2 = pm.proximity(lab, pos)
    assert near[0, 1] == 8 and d2[0, 1] == 0 and near[2, 2] == 8
    assert d2[2, 1] == 4 and d2[2, 0] == 5                  # (1, 2) and (0, 2) to the feature's place (1, 0)


def test_model_without_features_and_at_the_corners():
    lab = np.full((3, 3), -1, np.int32)
    near, d2 = pm.proximity(lab, planar())
    assert (near == -1).all() and (d2 == np.uint64(NONE)).all() and d2.dtype == np.uint64 and near.dtype == np.int32
    near, d2 = pm.proximity(np.zeros((3, 3), np.int32), planar(), outside=True)
    assert (near == -1).all() and (d2 == np.uint64(NONE)).all()
    pos = np.zeros((1, 2, 3), np.int64)
    pos[0, 0] = 2 ** 29
    pos[0, 1] = -2 ** 29
    near, d2 = pm.proximity(np.array([[0, -1]], np.int32), pos)
    assert near.tolist() == [[0, 0]] and d2.tolist() == [[0, 3 * 2 ** 60]]


def test_model_reach_by_hand():
    lab = np.array([[0, 0, -1], [0, 2, 2], [-1, 2, 2]], np.int32)
    d2 = np.array([[4, 9, 0], [9, 1, 1], [0, 7, 7]], np.uint64)
    near = np.arange(10, 19, dtype=np.int32).reshape(3, 3)
    r = pm.reach(lab, 4, d2, near)
    assert r[0].tolist() == (9, 4, 1, 0, 10, 3)             # the first of the two nines, nearest[0]
    assert r[1].tolist() == (0, NONE, -1, -1, -1, 0)        # a number no node carries
    assert r[2].tolist() == (7, 1, 7, 4, 14, 4)
    assert r[3].tolist() == (0, NONE, -1, -1, -1, 0)
    r = pm.reach(lab, 1, np.full((3, 3), NONE, np.uint64), np.full((3, 3), -1, np.int32))
    assert r[0].tolist() == (NONE, NONE, 0, 0, -1, 3)
    assert pm.reach(lab, 0, d2, near).shape == (0,)
