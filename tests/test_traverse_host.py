"""Least-cost traverses without a GPU: argument validation of mrtx_traverse and
mrtx_traverse_lengths, the lengths against a numpy haversine, the float64 model against SciPy's Dijkstra, the lattice's lat/lon
against grid_nodes, and route extraction on hand-made fields."""
import ctypes as C
import math

import numpy as np
import pytest

import synth_np
import traverse_model as tm
from moonrtx_amd import _lib
from moonrtx_amd import traverse as tv
from moonrtx_amd.renderer import MoonRT

E_INVALID, E_STATE = -1, -3
INF = float("inf")
NAN = float("nan")


@pytest.fixture
def ctx(native_lib):
    """A context handle; without a GPU mrtx_create stops at its first HIP call but hands the context out."""
    c = C.c_void_p()
    rc = native_lib.mrtx_create(C.byref(_lib.MrtxConfig(0, 16, 16, 0, 1, 0, 0)), C.byref(c))
    assert rc in (0, -2) and c.value
    yield c
    native_lib.mrtx_destroy(c)


def win(**kw):
    t = dict(row0=10, col0=20, rows=8, cols=16, stride=1, wrap=0, radius_m=1737400.0, max_grade=0.36, climb_cost=8.0,
             descent_cost=1.0, reserved=0)
    t.update(kw)
    return _lib.MrtxTraverse(**t)


def test_traverse_arguments_are_checked_before_any_device_call(native_lib, ctx):
    f = native_lib.mrtx_traverse
    rows, cols = 8, 16
    cost = np.empty((rows, cols), np.float64)
    pred = np.empty((rows, cols), np.uint8)
    src = np.array([[1, 2], [7, 15]], np.int32)
    sc = np.array([0.0, 5.0])
    pen = np.ones((rows, cols), np.float32)

    def call(c=ctx, t=None, s=src, s_cost=sc, n=2, dpen=None, hpen=None, dcost=None, hcost=cost, dpred=None, hpred=pred, **kw):
        t = win(**kw) if t is None else t
        return f(c, C.byref(t), None if s is None else s.ctypes.data, None if s_cost is None else s_cost.ctypes.data, n,
                 dpen, None if hpen is None else hpen.ctypes.data, dcost, None if hcost is None else hcost.ctypes.data, dpred,
                 None if hpred is None else hpred.ctypes.data, None, None)
    assert call(c=None) == E_INVALID
    assert f(ctx, None, src.ctypes.data, None, 2, None, None, None, cost.ctypes.data, None, pred.ctypes.data, None, None) == E_INVALID
    H = cost.ctypes.data
    bad = [dict(rows=0), dict(cols=0), dict(rows=-3), dict(stride=0), dict(stride=-2), dict(row0=-1), dict(col0=-1),
           dict(wrap=2), dict(wrap=-1), dict(wrap=1, cols=2, stride=1), dict(reserved=1),
           dict(rows=1 << 16, cols=(1 << 15) + 1),                                     # more than 2^31 nodes
           dict(radius_m=0.0), dict(radius_m=-1.0), dict(radius_m=NAN), dict(radius_m=INF), dict(radius_m=1e300),
           dict(max_grade=0.0), dict(max_grade=-0.5), dict(max_grade=NAN), dict(max_grade=1e-60),
           dict(climb_cost=-1.0), dict(climb_cost=NAN), dict(climb_cost=INF), dict(climb_cost=1e300),
           dict(descent_cost=-0.1), dict(descent_cost=NAN), dict(descent_cost=INF)]
    for kw in bad:
        assert call(**kw) == E_INVALID, kw
    assert call(hcost=None) == E_INVALID                        # neither cost output
    assert call(dcost=H) == E_INVALID                           # both cost outputs
    assert call(hpred=None) == E_INVALID                        # neither predecessor output
    assert call(dpred=H) == E_INVALID                           # both predecessor outputs
    assert call(dpen=H, hpen=pen) == E_INVALID                  # both penalties
    assert call(n=0) == E_INVALID and call(n=-1) == E_INVALID and call(s=None) == E_INVALID
    for s in ([[-1, 0]], [[0, -1]], [[8, 0]], [[0, 16]], [[3, 3], [3, 99]]):
        a = np.array(s, np.int32)
        assert call(s=a, n=len(a), s_cost=None) == E_INVALID, s
    for c0 in (-1.0, NAN, INF, -INF):
        assert call(s_cost=np.array([0.0, c0])) == E_INVALID, c0
    # every argument good: the missing DEM is next (the penalty table is scanned after that, with the DEM's shape known)
    for kw in (dict(), dict(max_grade=INF), dict(climb_cost=0.0, descent_cost=0.0), dict(rows=1 << 15, cols=1 << 16)):
        assert call(**kw) == E_STATE, kw
    one = np.zeros((1, 2), np.int32)
    for kw in (dict(stride=7, wrap=1, cols=3), dict(rows=1, cols=1)):
        assert call(s=one, n=1, s_cost=None, **kw) == E_STATE, kw
    assert call(s_cost=None) == E_STATE
    assert call(s=np.array([[1, 2], [1, 2]], np.int32), s_cost=np.array([-0.0, 3.0])) == E_STATE      # -0 is >= 0
    assert call(hpen=pen) == E_STATE and call(dpen=H) == E_STATE
    assert b"displacement" in native_lib.mrtx_last_error(ctx)


def test_lengths_refuse_bad_windows(native_lib):
    f = native_lib.mrtx_traverse_lengths
    out = np.empty((64, 3), np.float32)

    def call(h=180, w=360, o=out, **kw):
        return f(C.byref(win(**kw)), h, w, None if o is None else o.ctypes.data)
    assert call() == 0
    assert f(None, 180, 360, out.ctypes.data) == E_INVALID
    assert call(o=None) == E_INVALID
    bad = [dict(h=1), dict(w=1), dict(row0=173), dict(row0=179, rows=2), dict(row0=0, rows=61, stride=3),
           dict(col0=360), dict(col0=400), dict(cols=361), dict(rows=4, cols=13, stride=30),     # repeated columns
           dict(wrap=1, cols=16), dict(wrap=1, cols=36, stride=9), dict(wrap=1, cols=2, stride=180),
           dict(radius_m=1e-300),                                                       # lengths round to 0 in float32
           dict(stride=0), dict(rows=0), dict(max_grade=0.0)]
    for kw in bad:
        assert call(**kw) == E_INVALID, kw
    good = [dict(row0=172), dict(row0=0, rows=60, stride=3), dict(cols=360), dict(col0=359, rows=4, cols=12, stride=30),
            dict(wrap=1, rows=4, cols=36, stride=10, col0=5), dict(wrap=1, cols=360), dict(wrap=1, rows=1, cols=3, stride=120)]
    for kw in good:
        assert call(**kw) == 0, kw


def haversine(la1, lo1, la2, lo2, R):
    p1, p2, dl = np.radians(la1), np.radians(la2), np.radians(lo2 - lo1)
    h = np.sin((p2 - p1) / 2) ** 2 + np.cos(p1) * np.cos(p2) * np.sin(dl / 2) ** 2
    return 2 * R * np.arcsin(np.sqrt(h))


@pytest.mark.parametrize("H,W,row0,rows,stride", [(180, 360, 0, 180, 1), (1024, 2048, 3, 200, 5), (46080, 92160, 100, 64, 1)])
def test_lengths_agree_with_a_numpy_haversine(native_lib, H, W, row0, rows, stride):
    R = 1737400.0 * 1.004
    t = win(row0=row0, rows=rows, stride=stride, cols=4, radius_m=R)
    L = tm.lengths(t, (H, W))
    r = row0 + np.arange(rows) * stride
    lat = 90.0 - (r + 0.5) * 180.0 / H
    dlon = stride * 360.0 / W
    ref = [haversine(lat, 0.0, lat, dlon, R), haversine(lat[:-1], 0.0, lat[1:], 0.0, R),
           haversine(lat[:-1], 0.0, lat[1:], dlon, R)]
    for k in range(3):
        got = L[:, k] if k == 0 else L[:-1, k]
        ulp = np.spacing(got.astype(np.float32)).astype(np.float64)
        assert (np.abs(got - ref[k]) <= ulp).all(), k
    assert (L[-1, 1:] == 0).all()
    # along a row the edge falls as cos(lat): sin(L_ew / 2R) = cos(lat) sin(dlon / 2) on the sphere
    ratio = np.sin(L[:, 0].astype(np.float64) / (2 * R)) / math.sin(math.radians(dlon) / 2)
    assert np.allclose(ratio, np.cos(np.radians(lat)), rtol=1e-6, atol=1e-9)
    north = lat > 0
    assert (np.diff(L[north, 0]) >= 0).all() and (np.diff(L[~north, 0]) <= 0).all()


def scipy_field(wt, sources, wrap):
    sp = pytest.importorskip("scipy.sparse")
    csg = pytest.importorskip("scipy.sparse.csgraph")
    _, rows, cols = wt.shape
    us, vs, ws = [], [], []
    ii, jj = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    for k in range(8):
        ui, uj = ii + tm.DI[k], jj + tm.DJ[k]
        if wrap:
            uj = uj % cols
        ok = (ui >= 0) & (ui < rows) & (uj >= 0) & (uj < cols) & np.isfinite(wt[k])
        us.append((ui * cols + uj)[ok]); vs.append((ii * cols + jj)[ok]); ws.append(wt[k][ok].astype(np.float64))
    g = sp.csr_matrix((np.concatenate(ws), (np.concatenate(us), np.concatenate(vs))), shape=(rows * cols, rows * cols))
    idx = [i * cols + j for (i, j) in sources]
    return csg.dijkstra(g, directed=True, indices=idx, min_only=True).reshape(rows, cols)


@pytest.mark.parametrize("case", ["plain", "steep", "wrap", "penalty"])
def test_model_matches_scipy_dijkstra_bit_for_bit(native_lib, case):
    dem = synth_np.dem(180, 360, seed=7, craters=40)
    rng = np.random.default_rng(3)
    if case == "wrap":
        t = tm.make_window(2, 0, 20, 120, stride=3, wrap=1, max_grade=0.05)
    else:
        t = tm.make_window(40, 100, 48, 64, stride=1, max_grade=0.01 if case == "steep" else 0.36, descent_cost=2.0)
    P = None
    if case == "penalty":
        P = rng.uniform(0.5, 20.0, (t.rows, t.cols)).astype(np.float32)
        P[rng.random((t.rows, t.cols)) < 0.15] = np.inf
    L = tm.lengths(t, dem.shape)
    wt = tm.weights(tm.window_D(dem, t), P, L, t)
    if case == "steep":
        assert 0.05 < np.isinf(wt).mean() < 0.9       # the grade limit bites
    srcs = [(5, 7), (t.rows - 3, t.cols - 10)]
    src = {s: 0.0 for s in srcs}
    d = tm.dijkstra(wt, src, t.wrap)
    ref = scipy_field(wt, srcs, t.wrap)
    assert np.array_equal(d.view(np.uint64), ref.view(np.uint64))
    pred = tm.predecessors(d, wt, src, t.wrap)
    assert not (pred == 254).any()
    assert ((pred == 255) == np.isinf(d)).all()
    assert (pred[5, 7], pred[t.rows - 3, t.cols - 10]) == (8, 8)


def test_model_reduces_duplicate_sources_to_the_cheapest(native_lib):
    dem = synth_np.dem(90, 180, seed=2, craters=10)
    t = tm.make_window(20, 30, 16, 24)
    d1, p1 = tm.field(dem, t, [(3, 3), (3, 3), (10, 20)], [5.0, 2.0, 1e8])
    d2, p2 = tm.field(dem, t, [(3, 3), (10, 20)], [2.0, 1e8])
    assert np.array_equal(d1, d2) and np.array_equal(p1, p2)
    assert d1[3, 3] == 2.0 and p1[3, 3] == 8
    assert p1[10, 20] != 8          # a source reached more cheaply from the other is not marked as one


class FakeRT(MoonRT):
    """Only what traverse_nodes needs: the DEM's shape."""

    def __init__(self, h, w):   # noqa: D401 -- no context
        self._dem_shape = (h, w)
        self._ctx = None

    def close(self):
        pass


@pytest.mark.parametrize("H,W,window", [(180, 360, (10, 20, 30, 40)), (180, 360, (4, 350, 12, 20, 1)),
                                         (1024, 2048, (100, 0, 64, 256, 8, 1)), (720, 1440, (3, 7, 50, 60, 3))])
def test_traverse_nodes_line_up_with_grid_nodes(H, W, window):
    rt = FakeRT(H, W)
    lat, lon, grid = rt.traverse_nodes(window)
    w = tv.window_dict(window)
    assert lat.shape == (w["rows"],) and lon.shape == (w["cols"],)
    assert ((lon >= -180.0) & (lon < 180.0)).all()
    glat, glon = MoonRT.grid_nodes(**grid)
    assert np.allclose(glat, lat, atol=1e-9, rtol=0)
    assert np.allclose(((glon - lon + 180.0) % 360.0) - 180.0, 0.0, atol=1e-9)
    # texel centres of the DEM's own lattice (the bowl DEM's convention)
    r = w["row0"] + np.arange(w["rows"]) * w["stride"]
    assert np.allclose(lat, 90.0 - (r + 0.5) * 180.0 / H, atol=1e-12)
    # snapping a node's own position gives the node back; a point near it too
    ij = rt.snap_to_nodes(window, lat[[0, -1]] + 0.1 * 180.0 / H, lon[[0, -1]] - 0.1 * 360.0 / W)
    assert ij.tolist() == [[0, 0], [w["rows"] - 1, w["cols"] - 1]]
    with pytest.raises(ValueError):
        rt.snap_to_nodes(window, [lat[0] + 2 * w["stride"] * 180.0 / H], [lon[0]])


def hand_field(pred, cost=None, wrap=0, lengths=None):
    rows, cols = pred.shape
    cost = np.arange(rows * cols, dtype=np.float64).reshape(rows, cols) if cost is None else cost
    L = np.tile(np.array([[10.0, 20.0, 30.0]], np.float32), (rows, 1)) if lengths is None else lengths
    return tv.TraverseField(cost, pred, (0, 0, rows, cols, 1, wrap), L, 1000.0, np.arange(rows) * -1.0, np.arange(cols) * 2.0,
                            D=np.full((rows, cols), 1.001))


def test_route_follows_the_predecessors():
    pred = np.full((4, 5), 255, np.uint8)
    pred[0, 0] = 8
    pred[0, 1] = 6         # W -> (0, 0)
    pred[1, 2] = 7         # NW -> (0, 1)
    pred[2, 2] = 0         # N -> (1, 2)
    pred[3, 1] = 1         # NE -> (2, 2)
    f = hand_field(pred)
    r = tv.route(f, (3, 1))
    assert list(zip(r["i"], r["j"])) == [(0, 0), (0, 1), (1, 2), (2, 2), (3, 1)]
    assert r["cost"].tolist() == [0.0, 1.0, 7.0, 12.0, 16.0]
    assert r["length_m"].tolist() == [0.0, 10.0, 40.0, 60.0, 90.0]
    assert np.allclose(r["height_m"], 1.0, rtol=1e-4) and r["lat"].tolist() == [0, 0, -1, -2, -3] and r["lon"][1] == 2.0
    assert tv.route(f, (0, 0))["i"].tolist() == [0]


def test_route_crosses_the_wrap_and_raises_on_bad_codes():
    pred = np.full((2, 4), 255, np.uint8)
    pred[0, 3] = 8
    pred[0, 0] = 6         # W across the wrap -> (0, 3)
    pred[1, 1] = 7         # NW -> (0, 0)
    r = tv.route(hand_field(pred, wrap=1), (1, 1))
    assert list(zip(r["i"], r["j"])) == [(0, 3), (0, 0), (1, 1)]
    with pytest.raises(tv.RouteError, match="outside the window"):
        tv.route(hand_field(pred, wrap=0), (1, 1))
    with pytest.raises(tv.RouteError, match="unreachable"):
        tv.route(hand_field(pred, wrap=1), (1, 3))
    p2 = pred.copy(); p2[1, 3] = 254
    with pytest.raises(tv.RouteError, match="254"):
        tv.route(hand_field(p2, wrap=1), (1, 3))
    p3 = pred.copy(); p3[1, 2] = 200
    with pytest.raises(tv.RouteError, match="unknown"):
        tv.route(hand_field(p3, wrap=1), (1, 2))
    p4 = np.full((2, 2), 255, np.uint8); p4[0, 0] = 2; p4[0, 1] = 6      # a cycle with no source
    with pytest.raises(tv.RouteError, match="does not end"):
        tv.route(hand_field(p4), (0, 0))
    with pytest.raises(tv.RouteError, match="outside"):
        tv.route(hand_field(p4), (5, 0))


def test_penalty_builders_stay_in_the_accepted_range():
    view = np.array([[0.0, 3.5], [np.inf, 0.0]], np.float32)
    p = tv.penalty_from_viewshed(view)
    assert p.dtype == np.float32 and p.tolist() == [[1.0, INF], [INF, 1.0]]
    s = tv.penalty_from_sunlit(np.array([0.0, 0.5, 1.0, 0.05]), weight=4.0, min_share=0.1)
    assert s.tolist() == [INF, 3.0, 1.0, INF]
    t = tv.penalty_from_temperature(np.array([200.0, 350.0, 380.0, 400.1]), limit_k=400.0, soft_k=300.0)
    assert np.allclose(t[:3], [1.0, 5.5, 8.2]) and t[3] == INF
    for a in (p, s, t):
        ok = np.isinf(a) | ((a >= np.float32(1e-3)) & (a <= np.float32(1e6)))
        assert ok.all()
    assert tv.max_slope_grade(45.0) == pytest.approx(1.0) and tv.max_slope_grade(90.0) == INF
    with pytest.raises(ValueError):
        tv.max_slope_grade(0.0)


def test_device_tables_must_be_aligned_and_apart(native_lib, ctx):
    f = native_lib.mrtx_traverse
    src = np.array([[1, 2]], np.int32)
    base = 1 << 40                      # never dereferenced: every one of these calls is refused before any device call
    N = 8 * 16

    def call(dpen=None, dcost=None, dpred=None):
        cost = np.empty(N) if dcost is None else None
        pred = np.empty(N, np.uint8) if dpred is None else None
        return f(ctx, C.byref(win()), src.ctypes.data, None, 1, dpen, None, dcost,
                 None if cost is None else cost.ctypes.data, dpred, None if pred is None else pred.ctypes.data, None, None)
    for kw in (dict(dcost=base + 4), dict(dcost=base + 1), dict(dpen=base + 2),
               dict(dcost=base, dpred=base + 8 * N - 1), dict(dcost=base + 64, dpred=base),           # cost and codes overlap
               dict(dpen=base, dcost=base + 4 * N - 8), dict(dpen=base + 8 * N - 4, dcost=base),
               dict(dpen=base, dpred=base + 4 * N - 1)):
        assert call(**kw) == E_INVALID, kw
        assert b"align" in native_lib.mrtx_last_error(ctx) or b"overlap" in native_lib.mrtx_last_error(ctx), kw
    for kw in (dict(dcost=base), dict(dcost=base, dpred=base + 8 * N), dict(dpen=base + 8 * N + N, dcost=base, dpred=base + 8 * N),
               dict(dpen=base + 4)):
        assert call(**kw) == E_STATE, kw


def test_traverse_heights_arguments(native_lib, ctx):
    f = native_lib.mrtx_traverse_heights
    out = np.empty((8, 16), np.float32)
    O = out.ctypes.data
    assert f(None, C.byref(win()), None, O, None) == E_INVALID
    assert f(ctx, None, None, O, None) == E_INVALID
    assert f(ctx, C.byref(win()), None, None, None) == E_INVALID      # neither output
    assert f(ctx, C.byref(win()), O, O, None) == E_INVALID            # both
    assert f(ctx, C.byref(win()), (1 << 40) + 2, None, None) == E_INVALID
    for kw in (dict(rows=0), dict(stride=0), dict(wrap=3), dict(reserved=2)):
        assert f(ctx, C.byref(win(**kw)), None, O, None) == E_INVALID, kw
    assert f(ctx, C.byref(win()), None, O, None) == E_STATE


class FakeLib:
    """What MoonRT.traverse calls, answered on the host from the model (the real library for the lengths); once the
    context is closed every call fails loudly, so that a field that still reached into it would be caught."""

    def __init__(self, dem, lib):
        self.dem, self.lib, self.closed = dem, lib, False

    def _t(self, byref):
        if self.closed:
            raise AssertionError("the context was used after close")
        return byref._obj

    def mrtx_traverse_lengths(self, t, h, w, out):
        return self.lib.mrtx_traverse_lengths(t, h, w, out)

    def mrtx_traverse(self, ctx, t, ij, cost0, n, dpen, hpen, dcost, hcost, dpred, hpred, visits, st):
        t = self._t(t)
        src = np.ctypeslib.as_array(C.cast(ij, C.POINTER(C.c_int32)), (n, 2)).copy()
        d, p = tm.field(self.dem, t, src)
        C.memmove(hcost, d.ctypes.data, d.nbytes)
        C.memmove(hpred, p.ctypes.data, p.nbytes)
        return 0

    def mrtx_traverse_heights(self, ctx, t, dev, host, st):
        D = tm.window_D(self.dem, self._t(t))
        C.memmove(host, D.ctypes.data, D.nbytes)
        return 0

    def mrtx_last_error(self, ctx):
        return b"fake"


def test_route_after_the_context_is_closed(native_lib):
    dem = synth_np.dem(90, 180, seed=4, craters=8)
    rt = FakeRT(*dem.shape)
    rt._lib = FakeLib(dem, native_lib)
    window = (20, 30, 16, 24)
    with pytest.raises(ValueError):
        rt.traverse(window)                                             # neither sources nor nodes
    with pytest.raises(ValueError):
        rt.traverse(window, [(1.0, 2.0)], nodes=[(1, 2)])               # both
    with pytest.raises(ValueError):
        rt.traverse(window, nodes=np.array([[1.0, 2.0]]))               # nodes must be integers
    lat, lon, _ = rt.traverse_nodes(window)
    f = rt.traverse(window, [(lat[3], lon[4])], max_slope_deg=60.0)     # (lat, lon) in whole degrees would snap as well
    g = rt.traverse(window, nodes=[(3, 4)], max_slope_deg=60.0)
    assert np.array_equal(f.cost, g.cost) and f.cost[3, 4] == 0.0
    r = tv.route(f, (15, 20))
    h = rt.traverse(window, nodes=[(3, 4)], heights=False)
    assert np.isnan(tv.route(h, (15, 20))["height_m"]).all()
    rt._lib.closed = True                                               # the context is gone (or holds another DEM)
    r2 = tv.route(f, (15, 20))
    for k in r:
        assert np.array_equal(r[k], r2[k]), k
    D = tm.window_D(dem, tm.make_window(*window))
    assert np.array_equal(r2["height_m"], (D[r2["i"], r2["j"]].astype(np.float64) - 1.0) * 1737400.0)
    assert (r2["i"][0], r2["j"][0], r2["i"][-1], r2["j"][-1]) == (3, 4, 15, 20)
