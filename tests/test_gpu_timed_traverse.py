"""Timed traverses on the MI355X (DESIGN.md sections 3.19 and 4.22): arrival fields and predecessor codes bit-equal to the integer
model (tests/timed_traverse_model.py) on relief with partial tiles, a strided window with several sources and start ticks, a
wrapped polar window and a spiral maze, under random, moving-night, closed-node, all-ones and short availability tables of odd
lengths, with slow edges and a start on an epoch boundary; tile sizes, host and device tables and repeats; wrapped windows one and two tiles wide; and one end-to-end
run from drive_mask to timed_route."""
import ctypes as C
import math
from datetime import datetime, timedelta, timezone

import numpy as np
import pytest

import model_cases as mc
import synth_np
import timed_traverse_model as ttm
import traverse_model as tm
from moonrtx_amd import _lib
from moonrtx_amd import traverse as tv
from moonrtx_amd.renderer import DeviceBuffer, MoonRT
from test_gpu_horizon import OBS, scene
from test_gpu_illumination import make
from test_gpu_traverse import SEAM_CASES, seam_case, spiral_maze

pytestmark = pytest.mark.gpu

INF = float("inf")
NEVER = np.uint64(ttm.NEVER)


def relief():
    return synth_np.dem(180, 360, seed=7, craters=40)


def polar():
    return synth_np.dem(180, 360, seed=3, craters=60)


def maze_dem():
    return synth_np.dem(180, 360, seed=11, craters=20)


# The windows (name: DEM, window, sources, start ticks, penalty)
WINDOWS = {
    "relief": (relief, lambda: tm.make_window(30, 100, 70, 90, max_grade=0.02), [(35, 45)], None, None),     # partial tiles
    "strided": (mc.crater_dem, lambda: tm.make_window(10, 300, 50, 60, stride=3, max_grade=0.03, descent_cost=2.0),
                [(5, 5), (45, 50), (25, 30), (5, 5)], [0, 40000, 9000, 700], None),
    "polar-wrap": (polar, lambda: tm.make_window(0, 0, 30, 180, stride=2, wrap=1, max_grade=0.03), [(3, 10), (20, 170)],
                   [0, 2500], None),
    "maze": (maze_dem, lambda: tm.make_window(30, 100, 48, 48, max_grade=INF), [(24, 24)], None, "maze"),
}
# The cases (name: window, mask flavour, n_epochs, ticks_per_epoch, ticks_per_cost, what the flavour needs).  The relief
# window's edges weigh 15 390 to 49 596 (metres of effort on a 1 degree lattice), so ticks_per_cost = 0.01 makes them 154 to
# 496 ticks long: several to an epoch of 2000 ticks, two and more epochs each at 200 ticks (relief-slow).
#   random        bits set with probability p
#   night         a dark band of `width` columns that moves `speed` columns per epoch (timed_traverse_model.mask_moving_night)
#   closed        night, and one node with an all-zero row
#   ones          every bit set
CASES = {
    "relief-random": ("relief", "random", 130, 2000, 0.01, dict(p=0.7)),
    "relief-night": ("relief", "night", 130, 2000, 0.01, dict(width=12, speed=0.7, j_start=30)),
    "relief-closed": ("relief", "closed", 130, 2000, 0.01, dict(width=12, speed=0.7, j_start=30, node=(38, 50))),
    "relief-short": ("relief", "random", 7, 2000, 0.01, dict(p=0.7)),
    "relief-slow": ("relief", "random", 300, 200, 0.01, dict(p=0.85)),
    "relief-boundary": ("relief", "night", 130, 2000, 0.01, dict(width=12, speed=0.7, j_start=30, start=[6000])),
    "strided-night": ("strided", "night", 65, 3000, 0.005, dict(width=8, speed=0.5, j_start=12)),
    "polar-random": ("polar-wrap", "random", 63, 1500, 0.01, dict(p=0.7)),
    "polar-night": ("polar-wrap", "night", 130, 1500, 0.01, dict(width=25, speed=1.5, j_start=20)),
    "maze-night": ("maze", "night", 130, 3000, 0.01, dict(width=8, speed=0.4, j_start=20)),
    "odd-1": ("strided", "random", 1, 400000, 0.005, dict(p=0.8)),
    "odd-63": ("strided", "random", 63, 3000, 0.005, dict(p=0.7)),
    "odd-65": ("strided", "random", 65, 3000, 0.005, dict(p=0.7)),
    "odd-130": ("strided", "random", 130, 1500, 0.005, dict(p=0.7)),
}
# Measured on the CPU from the model alone: (share of the window's nodes reached, share of the reached nodes whose route holds a
# wait).  Every masked case must reach half the window and make a tenth of the reached nodes wait, except where that cannot be:
# a table of one epoch (odd-1) has no later epoch to wait for, so its waits are 0 by construction and only its reach is held.
MEASURED = {
    "relief-random": (0.995, 0.752), "relief-night": (0.995, 0.355), "relief-closed": (0.995, 0.355),
    "relief-short": (0.745, 0.603), "relief-slow": (0.995, 0.926), "relief-boundary": (0.995, 0.375),
    "strided-night": (0.994, 0.228), "polar-random": (1.000, 0.910), "polar-night": (1.000, 0.269),
    "maze-night": (0.672, 0.421), "odd-1": (0.798, 0.000), "odd-63": (0.994, 0.999), "odd-65": (0.994, 0.445),
    "odd-130": (0.994, 0.437),
}


def build(name):
    """(dem, t, sources, start ticks, penalty, avail booleans, n_epochs, tpe, tpc) of a case."""
    wname, flavour, n_ep, tpe, tpc, kw = CASES[name]
    mk, mkwin, src, ticks, pk = WINDOWS[wname]
    dem, t = mk(), mkwin()
    P = spiral_maze(t.rows, t.cols, gap=3) if pk == "maze" else None
    kw = dict(kw)
    node = kw.pop("node", None)
    ticks = kw.pop("start", ticks)
    if flavour == "random":
        av = ttm.mask_random(t.rows, t.cols, n_ep, kw["p"], seed=len(name))
    elif flavour in ("night", "closed"):
        av = ttm.mask_moving_night(t.rows, t.cols, n_ep, **kw)
    else:
        av = np.ones((t.rows, t.cols, n_ep), bool)
    if node is not None:
        av[node[0], node[1], :] = False
    return dem, t, src, ticks, P, av, n_ep, tpe, tpc


def ctx(dem):
    rt = MoonRT(16, 16)
    rt.upload_dem(dem)
    return rt


def gpu_field(rt, t, src, ticks=None, penalty=None, avail=None, n_epochs=0, tpe=3600, tpc=5.0, stats=None, dev_avail=None):
    """mrtx_traverse_timed straight through the ABI (the grade exactly as given), host pointers; avail = packed words."""
    ij = np.ascontiguousarray(np.asarray(src, np.int32).reshape(-1, 2))
    t0 = None if ticks is None else np.ascontiguousarray(ticks, np.uint64)
    pen = None if penalty is None else np.ascontiguousarray(penalty, np.float32)
    av = None if avail is None else np.ascontiguousarray(avail, np.uint64)
    A = np.empty((t.rows, t.cols), np.uint64)
    p = np.empty((t.rows, t.cols), np.uint8)
    tt = _lib.MrtxTraverseTimed(float(tpc), int(tpe), int(n_epochs), 0)
    visits = C.c_uint64()
    st = _lib.MrtxStats()
    rt._check(rt._lib.mrtx_traverse_timed(rt._ctx, C.byref(t), C.byref(tt), ij.ctypes.data, None if t0 is None else t0.ctypes.data,
                                          ij.shape[0], None, None if pen is None else pen.ctypes.data, dev_avail,
                                          None if av is None else av.ctypes.data, None, A.ctypes.data, None, p.ctypes.data,
                                          C.byref(visits), C.byref(st)), "mrtx_traverse_timed")
    if stats is not None:
        stats.update(launches=st.launches, kernel_ms=st.kernel_ms, tile_visits=visits.value)
    return A, p


def assert_field_equal(got, want, what):
    (A, p), (Am, pm) = got, want
    assert np.array_equal(A, Am), f"{what}: {int((A != Am).sum())} arrivals differ, first at {np.argwhere(A != Am)[:3].tolist()}"
    assert np.array_equal(p, pm), f"{what}: {int((p != pm).sum())} predecessor codes differ"
    assert not (p == 254).any(), what


def shares(name, want, dem, t, P, tpc):
    """(reached, waited) of a model field."""
    A, pred = want
    ql = ttm.durations(tm.weights(tm.window_D(dem, t), P, tm.lengths(t, dem.shape), t), tpc)
    reach = A != NEVER
    waited = ttm.waits_on_routes(A, pred, ql, t.wrap)
    return float(reach.mean()), float(waited[reach].mean()) if reach.any() else 0.0


@pytest.mark.parametrize("name", list(CASES))
def test_field_matches_the_model(native_lib, name):
    dem, t, src, ticks, P, av, n_ep, tpe, tpc = build(name)
    want = ttm.field(dem, t, src, ticks, P, av, tpc, tpe)
    reached, waited = shares(name, want, dem, t, P, tpc)
    print(f"{name}: {t.rows} x {t.cols}, reached {reached:.3f}, waiting routes {waited:.3f} (measured {MEASURED[name]})")
    assert reached >= 0.5, reached
    assert waited >= 0.1 or n_ep == 1, waited
    assert abs(reached - MEASURED[name][0]) < 1e-3 and abs(waited - MEASURED[name][1]) < 1e-3      # the model alone: it is pinned
    if name == "relief-short":              # the table ends before the far nodes are reached
        assert reached < 0.9 and (want[1][want[0] == NEVER] == 255).all()
    if name == "relief-closed":
        node = CASES[name][5]["node"]
        assert want[0][node] == NEVER and all(want[0][node[0] + a, node[1] + b] != NEVER for a in (-1, 1) for b in (-1, 1))
    if name == "relief-slow":               # the longest driven edges span two or more epochs
        ql = ttm.durations(tm.weights(tm.window_D(dem, t), P, tm.lengths(t, dem.shape), t), tpc)
        assert max(q for k in ql for row in k for q in row if q is not None) >= 2 * tpe
    if name == "relief-boundary":
        assert ticks[0] % tpe == 0 and ticks[0] > 0
    rt = ctx(dem)
    st = {}
    got = gpu_field(rt, t, src, ticks, P, tv.pack_mask(av), n_ep, tpe, tpc, st)
    rt.close()
    print(f"{name}: {st['launches']} launches, {st['tile_visits']} tile visits, {st['kernel_ms']:.3f} ms")
    assert_field_equal(got, want, name)


def test_all_ones_is_the_call_without_a_table_and_the_plain_dijkstra(native_lib):
    for wname in ("relief", "polar-wrap", "maze"):
        mk, mkwin, src, ticks, pk = WINDOWS[wname]
        dem, t = mk(), mkwin()
        P = spiral_maze(t.rows, t.cols, gap=3) if pk == "maze" else None
        tpe, tpc, n_ep = 2000, 0.01, 200
        plain = ttm.field(dem, t, src, ticks, P, None, tpc, tpe)            # the integer Dijkstra, no table
        assert (plain[0] != NEVER).mean() >= 0.45 and int(plain[0][plain[0] != NEVER].max()) < n_ep * tpe
        rt = ctx(dem)
        none = gpu_field(rt, t, src, ticks, P, None, 0, tpe, tpc)
        ones = gpu_field(rt, t, src, ticks, P, tv.pack_mask(np.ones((t.rows, t.cols, n_ep), bool)), n_ep, tpe, tpc)
        # words of all ones with garbage past the last epoch: the table still ends at n_epochs
        full = np.full((t.rows, t.cols, tv.mask_words(n_ep)), ~np.uint64(0), np.uint64)
        garbage = gpu_field(rt, t, src, ticks, P, full, n_ep, tpe, tpc)
        rt.close()
        assert_field_equal(none, plain, f"{wname}: no table")
        assert_field_equal(ones, plain, f"{wname}: all ones")
        assert_field_equal(garbage, plain, f"{wname}: all ones, tail bits set")
        if pk == "maze":
            assert (none[1][np.isinf(P)] == 255).all()


def test_tile_sizes_tables_and_repeats_agree(native_lib, monkeypatch):
    for name in ("relief-night", "polar-random"):
        dem, t, src, ticks, P, av, n_ep, tpe, tpc = build(name)
        words = tv.pack_mask(av)
        rt = ctx(dem)
        ref = gpu_field(rt, t, src, ticks, P, words, n_ep, tpe, tpc)
        buf = DeviceBuffer(words.nbytes)
        buf.upload(words)
        for ts in ("8", "16", "32"):
            monkeypatch.setenv("MOONRT_TRAVERSE_TILE", ts)
            for _ in range(2):
                assert_field_equal(gpu_field(rt, t, src, ticks, P, words, n_ep, tpe, tpc), ref, f"{name}: tile {ts}")
            assert_field_equal(gpu_field(rt, t, src, ticks, P, None, n_ep, tpe, tpc, dev_avail=buf.ptr), ref,
                               f"{name}: device table, tile {ts}")
        monkeypatch.delenv("MOONRT_TRAVERSE_TILE")
        # device arrival and predecessor buffers
        n = t.rows * t.cols
        ab, qb = DeviceBuffer(8 * n), DeviceBuffer(n)
        ij = np.ascontiguousarray(np.asarray(src, np.int32))
        tk = None if ticks is None else np.ascontiguousarray(ticks, np.uint64)
        tt = _lib.MrtxTraverseTimed(tpc, tpe, n_ep, 0)
        rc = rt._lib.mrtx_traverse_timed(rt._ctx, C.byref(t), C.byref(tt), ij.ctypes.data, None if tk is None else tk.ctypes.data,
                                         len(ij), None, None, buf.ptr, None, ab.ptr, None, qb.ptr, None, None, None)
        assert rc == 0, rt._lib.mrtx_last_error(rt._ctx)
        assert_field_equal((ab.download(np.uint64, (t.rows, t.cols)), qb.download(np.uint8, (t.rows, t.cols))), ref,
                           f"{name}: device outputs")
        for b in (buf, ab, qb):
            b.free()
        rt.close()


_SEAM_WANT = {}


@pytest.mark.parametrize("ts,wname,across", SEAM_CASES)
def test_narrow_wrapped_windows_match_the_model(native_lib, monkeypatch, ts, wname, across):
    """test_gpu_traverse's seam windows, one and two tiles wide at every tile edge, under a random table and without one.  The
    edges last 22 to 1916 ticks of epochs of 1500; the model alone reaches 0.875 to 0.9 of each window either way."""
    dem, t, src, P = seam_case(wname)
    assert (t.cols + int(ts) - 1) // int(ts) == across
    ticks, n_ep, tpe, tpc = [0, 700], 130, 1500, 0.001
    av = ttm.mask_random(t.rows, t.cols, n_ep, 0.8, seed=len(wname))
    if wname not in _SEAM_WANT:
        _SEAM_WANT[wname] = (ttm.field(dem, t, src, ticks, P, av, tpc, tpe), ttm.field(dem, t, src, ticks, P, None, tpc, tpe))
    masked, plain = _SEAM_WANT[wname]
    for want in (masked, plain):
        assert (want[0] != NEVER).mean() > 0.3
        assert np.isin(want[1][:, -1], (1, 2, 3)).any()     # predecessors east of the last column: across the seam
    assert not np.array_equal(masked[0], plain[0])          # the table makes routes wait
    monkeypatch.setenv("MOONRT_TRAVERSE_TILE", ts)
    rt = ctx(dem)
    got_masked = gpu_field(rt, t, src, ticks, P, tv.pack_mask(av), n_ep, tpe, tpc)
    got_plain = gpu_field(rt, t, src, ticks, P, None, 0, tpe, tpc)
    rt.close()
    assert_field_equal(got_masked, masked, f"{wname}, tile {ts}: random table")
    assert_field_equal(got_plain, plain, f"{wname}, tile {ts}: no table")


def test_drive_mask_to_route(native_lib):
    """traverse.drive_mask over a 24 x 24 strided window of the crater DEM for 300 hourly epochs, traverse_timed on it and a
    timed route: the mask is horizon_mask called per node, every step is driven only in epochs set at both of its ends, and
    the arrival is the model's on that mask."""
    s, dem = scene(), mc.crater_dem()
    rt = make(s, dem, 0)
    window = (40, 100, 24, 24, 4)
    t0 = datetime(2025, 3, 12, tzinfo=timezone.utc)         # sunrise crosses the window from east to west in epochs 49 to 140
    times = [t0 + timedelta(hours=k) for k in range(300)]
    buf = tv.drive_mask(rt, window, times, min_sun=0.5, n_az=64, n_bis=10, observer=OBS, chunk=200)
    W64 = tv.mask_words(300)
    words = buf.download(np.uint64, (24, 24, W64))
    lat, lon, _ = rt.traverse_nodes(window)
    la, lo = (a.ravel() for a in np.meshgrid(lat, lon, indexing="ij"))
    from moonrtx_amd import ephemeris as E
    ea = E.sun_epochs(times, OBS)
    hz = rt.horizon(la, lo, n_az=64, n_bis=10)
    assert np.array_equal(words.reshape(-1, W64), rt.horizon_mask(la, lo, hz, ea, min_a=0.5))
    bits = tv.unpack_mask(words, 300)
    assert 0.05 < bits.mean() < 0.95
    # 1 s ticks, hourly epochs; a speed that makes an edge last about half an hour
    Lmax = 2 * math.pi * 1737400.0 / 720 * 4 * 1.5
    tpc = 1800.0 / Lmax
    src = np.array([[12, 12]])
    start = int(np.flatnonzero(bits[12, 12])[0]) * 3600 if bits[12, 12].any() else 0
    kw = dict(nodes=src, start_tick=[start], n_epochs=300, ticks_per_epoch=3600, ticks_per_cost=tpc, max_slope_deg=25.0)
    f = rt.traverse_timed(window, avail=buf, **kw)
    f2 = rt.traverse_timed(window, avail=words, **kw)
    assert np.array_equal(f.arrival, f2.arrival) and np.array_equal(f.pred, f2.pred) and f.avail is None and f2.avail is not None
    t = tm.make_window(40, 100, 24, 24, stride=4, max_grade=tv.max_slope_grade(25.0))
    want = ttm.field(dem, t, src, [start], None, bits, tpc, 3600)
    assert_field_equal((f.arrival, f.pred), want, "drive mask")
    reach = f.arrival != NEVER
    assert reach.mean() > 0.5
    far = np.unravel_index(np.argmax(np.where(reach, f.arrival, 0)), reach.shape)
    r = tv.timed_route(f2, far)
    assert int(r["arrive_tick"][-1]) - start == r["drive_ticks"] + r["total_wait_ticks"] and r["total_wait_ticks"] > 0
    for k in range(len(r["i"]) - 1):
        i0, j0, i1, j1 = r["i"][k], r["j"][k], r["i"][k + 1], r["j"][k + 1]
        e0, e1 = int(r["depart_tick"][k]) // 3600, (int(r["arrive_tick"][k + 1]) - 1) // 3600
        assert bits[i0, j0, e0:e1 + 1].all() and bits[i1, j1, e0:e1 + 1].all(), k
    print(f"route of {len(r['i'])} nodes: {r['drive_ticks']} s driving, {r['total_wait_ticks']} s waiting, longest wait "
          f"{r['longest_wait_ticks']} s; reached {reach.mean():.3f}")
    buf.free()
    rt.close()
