"""Timed traverses without a GPU: the model's start() against a tick-by-tick search, its Dijkstra against
a randomly ordered label-correcting loop, the argument refusals of mrtx_horizon_mask and mrtx_traverse_timed through a context
without a device, timed_route on hand-made fields and the mask layout helpers."""
import ctypes as C
import math
import re
import os
from datetime import datetime, timedelta, timezone

import numpy as np
import pytest

import synth_np
import timed_traverse_model as ttm
import traverse_model as tm
from moonrtx_amd import _lib
from moonrtx_amd import ephemeris as E
from moonrtx_amd import traverse as tv

E_INVALID, E_STATE = -1, -3
INF, NAN = float("inf"), float("nan")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def ctx(native_lib):
    """A context handle; without a GPU mrtx_create stops at its first HIP call but hands the context out."""
    c = C.c_void_p()
    rc = native_lib.mrtx_create(C.byref(_lib.MrtxConfig(0, 16, 16, 0, 1, 0, 0)), C.byref(c))
    assert rc in (0, -2) and c.value
    yield c
    native_lib.mrtx_destroy(c)


# ---- the model ---------------------------------------------------------------------------------------------------------------
def test_start_agrees_with_a_tick_by_tick_search():
    rng = np.random.default_rng(31)
    seen = dict(short=0, long=0, on=0, off=0, last_epoch=0, none=0)
    for _ in range(3000):
        n = int(rng.integers(1, 20))
        tpe = int(rng.integers(1, 8))
        ok = (rng.random(n) < rng.choice([0.3, 0.6, 0.9])).tolist()
        if rng.random() < 0.3:
            ok[-1] = True                       # a run that ends at the table's last epoch
        q = int(rng.integers(1, 3 * tpe + 2))
        a = int(rng.integers(0, n * tpe + 2))
        want = ttm.start_brute(ok, a, q, tpe)
        got = ttm.start(ok, a, q, tpe)
        assert got == want, (ok, a, q, tpe)
        seen["short" if q < tpe else "long"] += 1
        seen["on" if a % tpe == 0 else "off"] += 1
        seen["none"] += got is None
        if got is not None and (got + q - 1) // tpe == n - 1:
            seen["last_epoch"] += 1
    assert min(seen.values()) >= 50, seen
    assert ttm.start(None, 17, 5, 3) == 17
    # the drive's last tick may be the table's last tick, not one more
    assert ttm.start([True, True], 0, 8, 4) == 0 and ttm.start([True, True], 1, 8, 4) is None
    assert ttm.start([False, True, True, False, True, True, True], 0, 9, 4) == 16


def small_case(rng):
    dem = synth_np.dem(45, 90, seed=int(rng.integers(1 << 30)), craters=6)
    wrap = int(rng.random() < 0.2)
    if wrap:        # a ring of 9 columns, 4 rows, every tenth texel
        t = tm.make_window(int(rng.integers(0, 5)), int(rng.integers(0, 90)), 4, 9, stride=10, wrap=1, max_grade=INF)
    else:
        t = tm.make_window(int(rng.integers(0, 30)), int(rng.integers(0, 80)), 9, 11, max_grade=float(rng.choice([INF, 0.02])))
    P = rng.uniform(0.5, 2.0, (t.rows, t.cols)).astype(np.float32)
    P[rng.random(P.shape) < 0.08] = np.inf
    L = tm.lengths(t, dem.shape)
    wt = tm.weights(tm.window_D(dem, t), P, L, t)
    tpe = int(rng.integers(50, 200))
    finite = wt[np.isfinite(wt)]
    tpc = 2.0 * tpe / float(finite.max()) if finite.size else 1.0       # the longest edge lasts two epochs
    ql = ttm.durations(wt, tpc)
    m = int(rng.integers(20, 80))
    avail = rng.random((t.rows, t.cols, m)) < rng.choice([0.6, 0.85])
    src = ttm.reduce_sources(rng.integers(0, t.rows, (3, 2)), rng.integers(0, 3 * tpe, 3))
    return ql, src, t.wrap, avail, tpe


def test_dijkstra_agrees_with_a_randomly_ordered_label_correcting_loop():
    rng = np.random.default_rng(77)
    reached = 0
    for _ in range(60):
        ql, src, wrap, avail, tpe = small_case(rng)
        A = ttm.dijkstra(ql, src, wrap, avail, tpe)
        B = ttm.label_correcting(ql, src, wrap, avail, tpe, rng)
        assert A == B
        pred = ttm.predecessors(A, ql, src, wrap, avail, tpe)
        assert not (pred == 254).any()
        reached += int((np.array(A, np.uint64) != ttm.NEVER).sum())
    assert reached > 60 * 36 * 0.5


def test_durations_follow_the_rule():
    wt = np.array([[[0.1, 0.2, 0.25, 1.0, 7.3, INF, 4.2e8, 4.4e8]]], np.float32)      # float32(0.2) * 5 is just above 1
    q = ttm.durations(wt, 5.0)[0][0]
    assert q[:5] == [1, 2, 2, 5, 37] and q[5] is None and q[6] == math.ceil(float(np.float32(4.2e8)) * 5.0) and q[7] is None
    edge = np.array([[[2.0 ** 29, np.nextafter(np.float32(2.0 ** 29), np.float32(INF))]]], np.float32)
    assert ttm.durations(edge, 4.0)[0][0] == [1 << 31, None]       # x = 2^31 exactly is driven, the next float32 is not
    for w, tpc in ((0.1, 5.0), (7.3, 5.0), (INF, 1.0), (4.4e8, 5.0), (3.0, 1e-9)):
        assert tv.edge_ticks(np.float32(w), tpc) == ttm.durations(np.array([[[w]]], np.float32), tpc)[0][0][0]


# ---- the ABI -----------------------------------------------------------------------------------------------------------------
def test_the_abi_holds_both_calls(native_lib):
    text = open(os.path.join(ROOT, "include", "moonrt.h")).read()
    for name in ("mrtx_horizon_mask", "mrtx_traverse_timed"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in _lib.SIGNATURES and getattr(native_lib, name) is not None
    assert native_lib.mrtx_abi_version() == 7 == _lib.ABI_VERSION
    assert C.sizeof(_lib.MrtxTraverseTimed) == 24


def test_horizon_mask_arguments_are_checked_before_any_device_call(native_lib, ctx):
    f = native_lib.mrtx_horizon_mask
    pts = np.array([[10.0, 20.0], [-5.0, 190.0]])
    hz = np.zeros((2, 8), np.float32)
    t0 = datetime(2025, 1, 1, tzinfo=timezone.utc)
    times = [t0 + timedelta(hours=24 * k) for k in range(5)]
    obs = E.Observer(52.2, 21.0, 0.0)
    ea, eb = E.sun_epochs(times, obs), E.earth_epochs(times, obs)
    out = np.empty((2, 1), np.uint64)
    O, H = out.ctypes.data, hz.ctypes.data

    def call(p=pts, n=2, n_az=8, dh=None, hh=H, a=ea, b=eb, m=5, ma=0.5, mb=1.0, dev=None, host=O, c=ctx):
        return f(c, None if p is None else p.ctypes.data, n, n_az, dh, hh, None if a is None else a.ctypes.data,
                 None if b is None else b.ctypes.data, m, ma, mb, dev, host, None)
    assert call(c=None) == E_INVALID
    for kw in (dict(p=None), dict(a=None), dict(n=0), dict(m=0), dict(m=(1 << 24) + 1), dict(n_az=6),
               dict(n_az=2), dict(hh=None), dict(dh=H), dict(host=None), dict(dev=O),
               dict(ma=0.0), dict(ma=-0.1), dict(ma=1.0000001), dict(ma=NAN), dict(ma=INF), dict(ma=1e-60),
               dict(mb=0.0), dict(mb=2.0), dict(mb=NAN), dict(mb=-1.0)):
        assert call(**kw) == E_INVALID, kw
    assert native_lib.mrtx_last_error(ctx)
    bad_hz = hz.copy()
    bad_hz[1, 3] = NAN
    assert call(hh=bad_hz.ctypes.data) == E_INVALID
    bad_ep = eb.copy()
    bad_ep[2, 3] = -1.0
    assert call(b=bad_ep) == E_INVALID and call(a=bad_ep) == E_INVALID
    assert call(host=None, dev=4) == E_INVALID                  # a device output that is not 8-byte aligned
    # good arguments: the missing DEM is next; without a second table min_b is not looked at
    for kw in (dict(), dict(ma=1e-6, mb=1e-6), dict(ma=1.0, mb=1.0), dict(m=1), dict(b=None), dict(b=None, mb=NAN),
               dict(b=None, mb=-3.0), dict(host=None, dev=8)):
        assert call(**kw) == E_STATE, kw
    assert b"displacement" in native_lib.mrtx_last_error(ctx)


def win(**kw):
    t = dict(row0=10, col0=20, rows=8, cols=16, stride=1, wrap=0, radius_m=1737400.0, max_grade=0.36, climb_cost=8.0,
             descent_cost=1.0, reserved=0)
    t.update(kw)
    return _lib.MrtxTraverse(**t)


def test_traverse_timed_arguments_are_checked_before_any_device_call(native_lib, ctx):
    f = native_lib.mrtx_traverse_timed
    rows, cols = 8, 16
    arr = np.empty((rows, cols), np.uint64)
    pred = np.empty((rows, cols), np.uint8)
    src = np.array([[1, 2], [7, 15]], np.int32)
    st = np.array([0, 5], np.uint64)
    pen = np.ones((rows, cols), np.float32)
    av = np.full((rows, cols, 2), ~np.uint64(0), np.uint64)
    H = arr.ctypes.data
    NOTT = object()

    def call(c=ctx, t=None, tt=None, s=src, s_tick=st, n=2, dpen=None, hpen=None, dav=None, hav=None, darr=None, harr=arr,
             dpred=None, hpred=pred, tpc=5.0, tpe=3600, ne=100, res=0, **kw):
        t = win(**kw) if t is None else t
        tt = _lib.MrtxTraverseTimed(tpc, tpe, ne, res) if tt is None else tt
        return f(c, C.byref(t), None if tt is NOTT else C.byref(tt), None if s is None else s.ctypes.data,
                 None if s_tick is None else s_tick.ctypes.data, n, dpen, None if hpen is None else hpen.ctypes.data, dav,
                 None if hav is None else hav.ctypes.data, darr, None if harr is None else harr.ctypes.data, dpred,
                 None if hpred is None else hpred.ctypes.data, None, None)
    assert call(c=None) == E_INVALID
    tt0 = _lib.MrtxTraverseTimed(5.0, 3600, 100, 0)
    assert f(ctx, None, C.byref(tt0), src.ctypes.data, None, 2, None, None, None, None, None, arr.ctypes.data, None,
             pred.ctypes.data, None, None) == E_INVALID
    assert call(tt=NOTT) == E_INVALID                           # a null tt
    # everything mrtx_traverse refuses about the window and the effort model
    bad = [dict(rows=0), dict(cols=0), dict(rows=-3), dict(stride=0), dict(stride=-2), dict(row0=-1), dict(col0=-1),
           dict(wrap=2), dict(wrap=-1), dict(wrap=1, cols=2, stride=1), dict(reserved=1),
           dict(rows=1 << 16, cols=(1 << 15) + 1),
           dict(radius_m=0.0), dict(radius_m=-1.0), dict(radius_m=NAN), dict(radius_m=INF), dict(radius_m=1e300),
           dict(max_grade=0.0), dict(max_grade=-0.5), dict(max_grade=NAN), dict(max_grade=1e-60),
           dict(climb_cost=-1.0), dict(climb_cost=NAN), dict(climb_cost=INF), dict(climb_cost=1e300),
           dict(descent_cost=-0.1), dict(descent_cost=NAN), dict(descent_cost=INF)]
    for kw in bad:
        assert call(**kw) == E_INVALID, kw
    # the tick scales
    for kw in (dict(res=1), dict(tpc=0.0), dict(tpc=-1.0), dict(tpc=NAN), dict(tpc=INF), dict(tpe=0), dict(tpe=-5)):
        assert call(**kw) == E_INVALID, kw
    for ne in (0, -1, (1 << 24) + 1):
        assert call(ne=ne, hav=av) == E_INVALID, ne               # out of range while a table is given
        assert call(ne=ne, dav=H + 4096) == E_INVALID, ne
        assert call(ne=ne) == E_STATE, ne                         # ignored without a table
    assert call(harr=None) == E_INVALID                         # neither arrival output
    assert call(darr=H) == E_INVALID                            # both arrival outputs
    assert call(hpred=None) == E_INVALID and call(dpred=H) == E_INVALID
    assert call(dpen=H, hpen=pen) == E_INVALID                  # both penalties
    assert call(dav=H, hav=av) == E_INVALID                     # both availability tables
    assert call(dav=H + 4, harr=None, darr=H + (1 << 20)) == E_INVALID      # dev_avail not 8-byte aligned
    assert call(harr=None, darr=H + 4) == E_INVALID             # dev_arrival not 8-byte aligned
    N = rows * cols
    big = 1 << 24
    # overlapping device tables: the availability table (N x 2 words) against each of the others, and mrtx_traverse's pairs
    assert call(dav=big, harr=None, darr=big + 8 * N * 2 - 8) == E_INVALID
    assert call(dav=big, hpred=None, dpred=big + 5) == E_INVALID
    assert call(dav=big, dpen=big + 8 * N) == E_INVALID
    assert call(harr=None, darr=big, hpred=None, dpred=big + 8 * N - 1) == E_INVALID
    assert call(harr=None, darr=big, dpen=big + 8) == E_INVALID
    assert call(n=0) == E_INVALID and call(n=-1) == E_INVALID and call(s=None) == E_INVALID
    for s in ([[-1, 0]], [[0, -1]], [[8, 0]], [[0, 16]], [[3, 3], [3, 99]]):
        a = np.array(s, np.int32)
        assert call(s=a, n=len(a), s_tick=None) == E_INVALID, s
    # with a table a start tick lies inside it
    assert call(hav=av, ne=100, tpe=10, s_tick=np.array([0, 1000], np.uint64)) == E_INVALID
    assert call(hav=av, ne=100, tpe=10, s_tick=np.array([0, 999], np.uint64)) == E_STATE
    assert call(tpe=10, s_tick=np.array([0, 1000], np.uint64)) == E_STATE
    assert call(s_tick=np.array([0, 1 << 62], np.uint64)) == E_INVALID
    # every argument good: the missing DEM is next, before the window is checked against the DEM's shape
    for kw in (dict(), dict(max_grade=INF), dict(hav=av), dict(dav=big, harr=None, darr=big + 8 * N * 2, hpred=None,
                                                               dpred=big + 8 * N * 3, dpen=big + 8 * N * 4),
               dict(s_tick=None), dict(ne=1 << 24, dav=big), dict(tpc=1e-300), dict(tpe=(1 << 31) - 1),
               dict(row0=100000), dict(col0=1 << 30), dict(hpen=pen)):
        assert call(**kw) == E_STATE, kw
    assert b"displacement" in native_lib.mrtx_last_error(ctx)


# ---- routes ------------------------------------------------------------------------------------------------------------------
def flat_field(arrival, pred, tpc=0.01, tpe=100, penalty=None, wrap=0, n_epochs=None):
    arrival = np.asarray(arrival, np.uint64)
    rows, cols = arrival.shape
    L = np.tile(np.array([[1000.0, 1000.0, 1414.0]], np.float32), (rows, 1))
    return tv.TimedField(arrival, pred, (0, 0, rows, cols, 1, wrap), L, D=np.ones((rows, cols), np.float32), ticks_per_cost=tpc,
                         ticks_per_epoch=tpe, n_epochs=n_epochs, penalty=penalty)


def test_timed_route_waits_add_up():
    # q = 10 ticks E-W and N-S, 15 (ceil(14.14)) diagonally; source (0, 0) starts at tick 7
    N_ = int(tv.NEVER)
    A = np.array([[7, 17, 40], [N_, 32, 55], [N_, N_, 90]], np.uint64)
    P = np.array([[8, 6, 6], [255, 7, 7], [255, 255, 7]], np.uint8)          # W, W / NW, NW / NW
    f = flat_field(A, P)
    assert f.edge_ticks_at(0, 1, 6) == 10 and f.edge_ticks_at(1, 1, 7) == 15
    r = tv.timed_route(f, (2, 2))
    assert r["i"].tolist() == [0, 1, 2] and r["j"].tolist() == [0, 1, 2]
    assert r["arrive_tick"].tolist() == [7, 32, 90]
    assert r["wait_ticks"].tolist() == [10, 43, 0] and r["depart_tick"].tolist() == [17, 75, 90]
    assert r["longest_wait_ticks"] == 43 and r["total_wait_ticks"] == 53 and r["drive_ticks"] == 30
    assert int(A[2, 2]) - 7 == r["drive_ticks"] + r["total_wait_ticks"]
    assert r["wait_ticks"].dtype == np.uint64 and r["cost"].tolist() == [7.0, 32.0, 90.0]
    r = tv.timed_route(f, (0, 2))
    assert r["wait_ticks"].tolist() == [0, 13, 0] and int(A[0, 2]) - 7 == r["drive_ticks"] + r["total_wait_ticks"] == 33
    r = tv.timed_route(f, (0, 0))                               # the source itself
    assert r["arrive_tick"].tolist() == [7] and r["longest_wait_ticks"] == 0 and r["drive_ticks"] == 0
    # a penalty map enters q: the mean of the two ends' penalties
    f2 = flat_field(A, P, penalty=np.array([[1, 3, 1], [1, 1, 1], [1, 1, 1]], np.float32))
    assert f2.edge_ticks_at(0, 1, 6) == 20 and f2.edge_ticks_at(0, 2, 6) == 20
    with pytest.raises(tv.RouteError):                          # 17 - 20 < 7: the step does not fit
        tv.timed_route(f2, (0, 1))
    # across the seam of a wrapped window
    fw = flat_field(np.array([[12, N_, 2]], np.uint64), np.array([[2 + 4, 255, 8]], np.uint8), wrap=1)     # W of column 0 is 2
    r = tv.timed_route(fw, (0, 0))
    assert r["j"].tolist() == [2, 0] and r["wait_ticks"].tolist() == [0, 0]
    tv.timed_route_csv(r, os.devnull)


def test_timed_route_errors():
    N_ = int(tv.NEVER)
    A = np.array([[7, 17, N_]], np.uint64)
    f = flat_field(A, np.array([[8, 6, 255]], np.uint8))
    with pytest.raises(tv.RouteError, match="unreachable"):
        tv.timed_route(f, (0, 2))
    with pytest.raises(tv.RouteError, match="outside"):
        tv.timed_route(f, (0, 3))
    with pytest.raises(tv.RouteError, match="254"):
        tv.timed_route(flat_field(A, np.array([[8, 254, 255]], np.uint8)), (0, 1))
    with pytest.raises(tv.RouteError, match="unknown"):
        tv.timed_route(flat_field(A, np.array([[8, 9, 255]], np.uint8)), (0, 1))
    with pytest.raises(tv.RouteError, match="outside the window"):
        tv.timed_route(flat_field(A, np.array([[6, 6, 255]], np.uint8)), (0, 1))
    with pytest.raises(tv.RouteError, match="source"):         # a cycle never ends at a source
        tv.timed_route(flat_field(A, np.array([[2, 6, 255]], np.uint8)), (0, 1))
    with pytest.raises(ValueError):
        tv.TimedField(A, np.zeros((2, 2), np.uint8), (0, 0, 1, 3), np.ones((1, 3), np.float32))
    assert np.isinf(f.cost[0, 2]) and f.cost[0, 1] == 17.0


# ---- mask layout ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 63, 64, 65, 130, 200])
def test_pack_and_unpack_against_packbits(m):
    rng = np.random.default_rng(m)
    bits = rng.random((3, 5, m)) < 0.5
    words = tv.pack_mask(bits)
    W64 = tv.mask_words(m)
    assert words.shape == (3, 5, W64) and words.dtype == np.uint64 and W64 == (m + 63) // 64
    pad = np.zeros((3, 5, W64 * 64), np.uint8)
    pad[..., :m] = bits
    want = np.packbits(pad, axis=-1, bitorder="little").reshape(3, 5, W64, 8)
    assert np.array_equal(words.view(np.uint8).reshape(3, 5, W64, 8), want)
    for k in (0, m // 2, m - 1):
        assert np.array_equal((words[..., k >> 6] >> np.uint64(k & 63)) & np.uint64(1), bits[..., k].astype(np.uint64))
    if m % 64:
        assert not (words[..., -1] >> np.uint64(m % 64)).any()     # the tail bits are 0
    assert np.array_equal(tv.unpack_mask(words, m), bits)
    with pytest.raises(ValueError):
        tv.unpack_mask(words, m + 64)


def test_moving_night_mask_moves():
    av = ttm.mask_moving_night(2, 10, 30, width=3, speed=0.5, j_start=3)
    assert av.shape == (2, 10, 30) and np.array_equal(av[0], av[1])
    dark = ~av[0]                               # (cols, epochs)
    assert dark[:, 0].nonzero()[0].tolist() == [0, 1, 2] and dark[:, 2].nonzero()[0].tolist() == [1, 2, 3]
    assert dark[:, 20].nonzero()[0].tolist() == [] and dark[:, 22].nonzero()[0].tolist() == [0]      # the band comes round
    assert dark.sum(0).max() == 3
