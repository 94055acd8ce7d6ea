"""Least-cost traverses on the MI355X (DESIGN.md sections 3.13 and 4.14): cost and predecessor fields bit-equal to the float64
model (tests/traverse_model.py) on relief, the bowl, strided and wrapped polar windows, several sources and a spiral maze of
impassable walls; the minimum over sources; tile sizes, repeats, device pointers and a device penalty check; wrapped windows one and two tiles wide; routes that keep
the slope limit and a line of sight; the smooth sphere's symmetry; the render state left alone; the full-size DEM."""
import ctypes as C
import math
import time

import numpy as np
import pytest

import model_cases as mc
import synth_np
import traverse_model as tm
from bowl_dem import bowl_dem
from common import assert_bit_equal
from moonrtx_amd import _lib
from moonrtx_amd import traverse as tv
from moonrtx_amd.renderer import DeviceBuffer, MoonRT, MoonRTError, synth_ldem, dem_from_ldem
from moonrtx_amd.scene import named_scene
from test_gpu_illumination import make

pytestmark = pytest.mark.gpu

RM = 1737400.0
INF = float("inf")


def ctx(dem):
    rt = MoonRT(16, 16)
    rt.upload_dem(dem)
    return rt


def spiral_maze(rows, cols, gap=3):
    """+inf walls of a square spiral with one gap per turn: routes from the centre wind outwards."""
    P = np.ones((rows, cols), np.float32)
    r0, c0, r1, c1 = 0, 0, rows - 1, cols - 1
    turn = 0
    while r1 - r0 > 2 * gap and c1 - c0 > 2 * gap:
        if turn % 4 == 0:
            P[r0, c0:c1 - gap + 1] = np.inf
        elif turn % 4 == 1:
            P[r0:r1 - gap + 1, c1] = np.inf
        elif turn % 4 == 2:
            P[r1, c0 + gap:c1 + 1] = np.inf
        else:
            P[r0 + gap:r1 + 1, c0] = np.inf
            r0, c0, r1, c1 = r0 + gap, c0 + gap, r1 - gap, c1 - gap
        turn += 1
    return P


def gpu_field(rt, t, src, cost0=None, penalty=None, stats=None):
    """mrtx_traverse straight through the ABI (the grade exactly as given), host pointers."""
    rows, cols = t.rows, t.cols
    ij = np.ascontiguousarray(np.asarray(src, np.int32).reshape(-1, 2))
    c0 = None if cost0 is None else np.ascontiguousarray(cost0, np.float64)
    pen = None if penalty is None else np.ascontiguousarray(penalty, np.float32)
    d = np.empty((rows, cols), np.float64)
    p = np.empty((rows, cols), np.uint8)
    visits = C.c_uint64()
    st = _lib.MrtxStats()
    rt._check(rt._lib.mrtx_traverse(rt._ctx, C.byref(t), ij.ctypes.data, None if c0 is None else c0.ctypes.data, ij.shape[0],
                                    None, None if pen is None else pen.ctypes.data, None, d.ctypes.data, None, p.ctypes.data,
                                    C.byref(visits), C.byref(st)), "mrtx_traverse")
    if stats is not None:
        stats.update(launches=st.launches, kernel_ms=st.kernel_ms, tile_visits=visits.value)
    return d, p


def assert_field_equal(got, want, what):
    (d, p), (dm, pm) = got, want
    assert np.array_equal(d.view(np.uint64), dm.view(np.uint64)), (
        f"{what}: {int((d.view(np.uint64) != dm.view(np.uint64)).sum())} costs differ; max |diff| "
        f"{np.nanmax(np.abs(np.where(np.isfinite(d) & np.isfinite(dm), d - dm, 0.0)))}")
    assert np.array_equal(p, pm), f"{what}: {int((p != pm).sum())} predecessor codes differ"
    assert not (p == 254).any(), what


def bowl():
    return bowl_dem(360, 720, lat0_deg=-30.0, lon0_deg=40.0, theta_c_deg=6.0, d_over_D=0.2)


CASES = {
    # name: (dem, window, sources, start costs, penalty)
    "synth": (lambda: synth_np.dem(180, 360, seed=7, craters=40), tm.make_window(30, 100, 70, 90, max_grade=0.005),
              [(35, 45)], None, None),
    "craters-stride3": (mc.crater_dem, tm.make_window(10, 300, 100, 120, stride=3, max_grade=0.01, descent_cost=2.0),
                        [(5, 5), (90, 100), (50, 60)], [0.0, 1e5, 3e4], None),
    "bowl": (bowl, tm.make_window(200, 400, 80, 80, max_grade=math.tan(math.radians(25.0)), climb_cost=20.0),
             [(2, 3), (79, 79)], None, None),
    "polar-cap-wrap": (lambda: synth_np.dem(180, 360, seed=3, craters=60), tm.make_window(0, 0, 30, 180, stride=2, wrap=1, max_grade=0.01),
                       [(3, 10), (20, 170)], None, None),
    "penalty": (lambda: synth_np.dem(180, 360, seed=7, craters=40), tm.make_window(40, 20, 64, 100, max_grade=0.02, descent_cost=1.0),
                [(10, 10), (60, 90), (10, 10)], [7.0, 0.0, 3.0], "random"),
}


def case_penalty(kind, t):
    if kind == "random":
        rng = np.random.default_rng(5)
        P = rng.uniform(1e-3, 50.0, (t.rows, t.cols)).astype(np.float32)
        P[rng.random(P.shape) < 0.1] = np.inf
        return P
    return None


@pytest.mark.parametrize("name", list(CASES))
def test_field_matches_the_model(native_lib, name):
    mk, t, src, c0, pk = CASES[name]
    dem = mk()
    P = case_penalty(pk, t)
    want = tm.field(dem, t, src, c0, P)
    assert np.isfinite(want[0]).mean() > 0.3
    rt = ctx(dem)
    st = {}
    got = gpu_field(rt, t, src, c0, P, st)
    rt.close()
    print(f"{name}: {t.rows} x {t.cols}, {st['launches']} launches, {st['tile_visits']} tile visits, {st['kernel_ms']:.3f} ms")
    assert_field_equal(got, want, name)
    assert st["launches"] >= 1 and st["tile_visits"] >= 1


def test_spiral_maze_forces_many_launches(native_lib, monkeypatch):
    dem = synth_np.dem(180, 360, seed=11, craters=20)
    t = tm.make_window(30, 100, 128, 128, max_grade=INF)
    P = spiral_maze(128, 128, gap=2)
    src = [(64, 64)]
    want = tm.field(dem, t, src, None, P)
    monkeypatch.setenv("MOONRT_TRAVERSE_TILE", "8")        # 16 x 16 tiles: the corridors cross tiles again and again
    rt = ctx(dem)
    st = {}
    got = gpu_field(rt, t, src, None, P, st)
    rt.close()
    print(f"maze: {st['launches']} launches, {st['tile_visits']} tile visits, {st['kernel_ms']:.3f} ms")
    assert_field_equal(got, want, "maze")
    assert np.isfinite(want[0]).mean() > 0.45 and (got[1][np.isinf(P)] == 255).all()
    assert st["launches"] >= 16 and st["tile_visits"] > 4 * 16 * 16     # 24 launches and 1350 visits when measured


def test_multi_source_is_the_minimum_of_single_sources(native_lib):
    dem = mc.crater_dem()
    t = tm.make_window(100, 200, 90, 110, max_grade=0.06)
    src = [(5, 5), (80, 100), (40, 20)]
    cost0 = [0.0, 2e4, 5e3]
    rt = ctx(dem)
    d, p = gpu_field(rt, t, src, cost0)
    singles = [gpu_field(rt, t, [s], [c])[0] for s, c in zip(src, cost0)]
    rt.close()
    assert np.array_equal(d, np.minimum.reduce(singles))
    for (i, j), c in zip(src, cost0):
        assert (p[i, j] == 8) == (d[i, j] == c)


def test_tile_sizes_repeats_and_device_pointers_agree(native_lib, monkeypatch):
    dem = synth_np.dem(180, 360, seed=7, craters=40)
    t = tm.make_window(20, 40, 77, 133, max_grade=0.04, descent_cost=0.5)      # partial tiles at every size
    rng = np.random.default_rng(9)
    P = rng.uniform(0.5, 3.0, (t.rows, t.cols)).astype(np.float32)
    P[30:33, 10:120] = np.inf
    src = [(3, 4), (70, 130)]
    # a wrapped polar cap whose last tile is partial at every size (90 columns): joined to tile 0 across +-180
    tw = tm.make_window(1, 0, 37, 90, stride=4, wrap=1, max_grade=0.02)
    Pw = rng.uniform(0.5, 3.0, (tw.rows, tw.cols)).astype(np.float32)
    Pw[10:30, 45] = np.inf
    srcw = [(5, 88), (30, 2)]
    rt = ctx(dem)
    ref = gpu_field(rt, t, src, None, P)
    refw = gpu_field(rt, tw, srcw, None, Pw)
    assert_field_equal(ref, tm.field(dem, t, src, None, P), "tile 32")
    assert_field_equal(refw, tm.field(dem, tw, srcw, None, Pw), "wrapped, tile 32")
    for ts in ("8", "16", "32"):
        monkeypatch.setenv("MOONRT_TRAVERSE_TILE", ts)
        for _ in range(2):
            assert_field_equal(gpu_field(rt, t, src, None, P), ref, f"tile {ts}")
            assert_field_equal(gpu_field(rt, tw, srcw, None, Pw), refw, f"wrapped, tile {ts}")
    monkeypatch.setenv("MOONRT_TRAVERSE_TILE", "12")
    with pytest.raises(MoonRTError):
        gpu_field(rt, t, src, None, P)
    monkeypatch.delenv("MOONRT_TRAVERSE_TILE")
    # device penalty, cost and predecessor buffers
    n = t.rows * t.cols
    pb, cb, qb = DeviceBuffer(4 * n), DeviceBuffer(8 * n), DeviceBuffer(n)
    pb.upload(P)
    ij = np.ascontiguousarray(np.array(src, np.int32))
    rc = rt._lib.mrtx_traverse(rt._ctx, C.byref(t), ij.ctypes.data, None, 2, pb.ptr, None, cb.ptr, None, qb.ptr, None, None, None)
    assert rc == 0, rt._lib.mrtx_last_error(rt._ctx)
    assert_field_equal((cb.download(np.float64, (t.rows, t.cols)), qb.download(np.uint8, (t.rows, t.cols))), ref, "device")
    # a bad entry of a device penalty table is caught in the kernel
    for bad in (np.nan, -1.0, 0.0, 5e-4, 2e6, -np.inf):
        Q = P.copy()
        Q[40, 50] = bad
        pb.upload(Q)
        rc = rt._lib.mrtx_traverse(rt._ctx, C.byref(t), ij.ctypes.data, None, 2, pb.ptr, None, cb.ptr, None, qb.ptr, None, None,
                                   None)
        assert rc == -1 and b"penalty" in rt._lib.mrtx_last_error(rt._ctx), bad
        d = np.empty((t.rows, t.cols)); p = np.empty((t.rows, t.cols), np.uint8)
        rc = rt._lib.mrtx_traverse(rt._ctx, C.byref(t), ij.ctypes.data, None, 2, None, Q.ctypes.data, None, d.ctypes.data, None,
                                   p.ctypes.data, None, None)
        assert rc == -1, bad
    for buf in (pb, cb, qb):
        buf.free()
    # and the context still works after the refusals
    assert_field_equal(gpu_field(rt, t, src, None, P), ref, "after refusals")
    # the window's DEM-dependent checks
    for kw in (dict(row0=175), dict(col0=360), dict(cols=361), dict(wrap=1)):
        bad_t = tm.make_window(**{**dict(row0=20, col0=40, rows=10, cols=10), **kw})
        with pytest.raises(MoonRTError):
            gpu_field(rt, bad_t, [(0, 0)])
    rt.close()


# Wrapped windows of a 180 x 360 DEM (cols x stride = 360) so narrow that the tile grid is one tile wide -- a tile's east and
# west neighbour is the tile itself -- or two tiles wide -- both are the same other tile -- at every tile edge.
# name: (row0, rows, cols, stride); case: (tile edge, window, tiles across)
SEAM_WINDOWS = {"w8": (10, 4, 8, 45), "w15": (5, 8, 15, 24), "w24": (3, 12, 24, 15), "w40": (4, 19, 40, 9)}
SEAM_CASES = [("8", "w8", 1), ("8", "w15", 2), ("16", "w15", 1), ("16", "w24", 2), ("32", "w24", 1), ("32", "w40", 2)]
_SEAM_DEM = []


def seam_case(wname):
    """(dem, t, sources, penalty) of a seam window: a wall of +inf penalties down the middle column and both sources just east
    of the seam, so that the nodes between the wall and the seam are reached across the seam only.  max_grade = 0.004 from the
    model alone: it reaches 0.875 to 0.9 of the four windows (0.53 to 0.81 at 0.002, under 0.1 of three of them at 0.001)."""
    if not _SEAM_DEM:
        _SEAM_DEM.append(synth_np.dem(180, 360, seed=3, craters=60))
    row0, rows, cols, stride = SEAM_WINDOWS[wname]
    t = tm.make_window(row0, 6, rows, cols, stride=stride, wrap=1, max_grade=0.004, descent_cost=1.0)
    P = np.ones((rows, cols), np.float32)
    P[:, cols // 2] = np.inf
    return _SEAM_DEM[0], t, [(rows // 2, 1), (1, 2)], P


_SEAM_WANT = {}


@pytest.mark.parametrize("ts,wname,across", SEAM_CASES)
def test_narrow_wrapped_windows_match_the_model(native_lib, monkeypatch, ts, wname, across):
    dem, t, src, P = seam_case(wname)
    assert (t.cols + int(ts) - 1) // int(ts) == across
    if wname not in _SEAM_WANT:
        _SEAM_WANT[wname] = tm.field(dem, t, src, [0.0, 5e5], P)
    want = _SEAM_WANT[wname]
    assert np.isfinite(want[0]).mean() > 0.3
    assert np.isin(want[1][:, -1], (1, 2, 3)).any()         # predecessors east of the last column: across the seam
    monkeypatch.setenv("MOONRT_TRAVERSE_TILE", ts)
    rt = ctx(dem)
    st = {}
    got = gpu_field(rt, t, src, [0.0, 5e5], P, st)
    rt.close()
    print(f"{wname}, tile {ts}: {st['launches']} launches, {st['tile_visits']} tile visits, {st['kernel_ms']:.3f} ms")
    assert_field_equal(got, want, f"{wname}, tile {ts}")


def test_routes_keep_the_slope_limit_and_a_line_of_sight(native_lib):
    dem = mc.crater_dem()
    s = named_scene("S1", 16, 16)
    rt = make(s, dem, 0)
    window = (120, 200, 64, 96)
    lat, lon, grid = rt.traverse_nodes(window)
    start = (lat[4], lon[6])
    plain = rt.traverse(window, [start], max_slope_deg=2.0, climb_cost=10.0, descent_cost=1.0)
    reach = np.isfinite(plain.cost)
    assert 0.3 < reach.mean() and not (plain.pred == 254).any()
    goal = np.unravel_index(np.argmax(np.where(reach, plain.cost, -1.0)), reach.shape)
    r = tv.route(plain, goal)
    D = tm.window_D(dem, tm.make_window(*window))
    for a, b in zip(range(len(r["i"]) - 1), range(1, len(r["i"]))):
        i0, j0, i1, j1 = r["i"][a], r["j"][a], r["i"][b], r["j"][b]
        k = [kk for kk in range(8) if (i1 + tm.DI[kk], j1 + tm.DJ[kk]) == (i0, j0)][0]
        L = plain.step_length(i1, k)
        dh = (np.float32(D[i1, j1]) - np.float32(D[i0, j0])) * np.float32(RM)
        assert abs(dh / np.float32(L)) <= np.float32(math.tan(math.radians(2.0)))
    assert np.allclose(r["height_m"], (D[r["i"], r["j"]].astype(np.float64) - 1.0) * RM)
    assert r["i"][0] == 4 and r["j"][0] == 6 and r["cost"][0] == 0.0 and (np.diff(r["cost"]) > 0).all()
    assert (np.diff(r["length_m"]) > 0).all()
    # keep sight of a relay 40 km above the start (a 15 km texel: a lander's own horizon lies inside its node): impassable
    # where the viewshed says the node cannot see it
    view = rt.viewshed((lat[4], lon[6], 40000.0), target_height_m=2.0, radius_m=RM, **grid)
    P = tv.penalty_from_viewshed(view)
    assert 0.02 < np.isinf(P).mean() < 0.98
    f2 = rt.traverse(window, [start], penalty=P, max_slope_deg=2.0, climb_cost=10.0, descent_cost=1.0)
    reach = np.isfinite(f2.cost)
    ti, tj = np.argwhere(reach)[np.argmax(np.where(reach, f2.cost, -1.0)[reach])]
    r2 = tv.route(f2, (ti, tj))
    assert len(r2["i"]) > 5 and (view[r2["i"], r2["j"]] == 0).all() and np.isfinite(P[r2["i"], r2["j"]]).all()
    assert (f2.cost[reach] >= plain.cost[reach]).all()
    # the sources snap to their nearest node; explicit (i, j) gives the same field
    f3 = rt.traverse(window, nodes=np.array([[4, 6]]), max_slope_deg=2.0, climb_cost=10.0, descent_cost=1.0)
    assert np.array_equal(f3.cost, plain.cost) and np.array_equal(f3.pred, plain.pred)
    # the field holds its own copy of the window's heights: routes do not reach into the context's DEM, which may hold
    # another DEM or be gone by then
    assert np.array_equal(plain.D, D) and np.array_equal(rt.traverse_heights(window), D)
    rt.upload_dem(synth_np.dem(360, 720, seed=99, craters=5))
    assert_routes_equal(tv.route(plain, goal), r)
    rt.close()
    del rt
    assert_routes_equal(tv.route(plain, goal), r)
    assert_routes_equal(tv.route(f2, (ti, tj)), r2)


def assert_routes_equal(a, b):
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_smooth_sphere_is_symmetric(native_lib):
    dem = np.ones((181, 360), np.float32)       # row 90's centre is the equator
    rt = ctx(dem)
    t = tm.make_window(70, 160, 41, 41)
    d, p = gpu_field(rt, t, [(20, 20)])
    rt.close()
    assert_field_equal((d, p), tm.field(dem, t, [(20, 20)]), "sphere")
    assert np.array_equal(d, d[:, ::-1])                         # about the source column: bit for bit
    assert np.allclose(d, d[::-1, :], rtol=1e-12, atol=0.0)     # about the source row (the equator)
    assert np.isfinite(d).all() and d[20, 20] == 0.0 and p[20, 20] == 8


def test_leaves_the_render_state_alone(native_lib):
    s = named_scene("S1", 16, 16).with_size(48, 32, spp_per_launch=16)
    dem = mc.crater_dem()

    def run(with_traverse):
        rt = make(s, dem, _lib.F_COUNT_STATS)
        st1 = rt.render(1)
        if with_traverse:
            rt.traverse((100, 100, 40, 50), nodes=np.array([[3, 4]]), penalty=np.full((40, 50), 2.0, np.float32), radius_m=RM)
        st2 = rt.render(1)
        out = rt.read_linear(), rt.read_hits(), rt.samples_done(), st1, st2
        rt.close()
        return out
    a, b = run(False), run(True)
    assert_bit_equal(b[0], a[0], "linear radiance")
    assert_bit_equal(b[1], a[1], "hit buffer")
    assert b[2] == a[2] == 32
    for k in ("primary_hits", "shadow_rays", "height_samples", "bounce_rays"):
        assert b[4][k] == a[4][k], k


def test_full_size(native_lib):
    """The headline DEM (23040 x 46080, more than 4 GiB: 64-bit texel offsets): a 1024 x 1024 mid-latitude window."""
    DEM_H, DEM_W = 23040, 46080
    src = synth_ldem(DEM_H, DEM_W)
    dem, scale = dem_from_ldem(src, DEM_H, DEM_W, 1)
    src.free()
    rt = MoonRT(16, 16)
    rt.bind_dem(dem, DEM_H, DEM_W)
    window = (17000, 30000, 1024, 1024)
    t0 = time.time()
    st = {}
    f = rt.traverse(window, nodes=np.array([[512, 512]]), max_slope_deg=15.0, radius_m=RM * scale, stats=st)
    wall = time.time() - t0
    rt.close()
    dem.free()
    r = tv.route(f, (1000, 30))          # after the context and its DEM are gone: the heights travel with the field
    print(f"full size 1024^2: {st['kernel_ms']:.2f} ms, {st['launches']} launches, {st['tile_visits']} tile visits, "
          f"reachable {float(np.isfinite(f.cost).mean()):.3f}, wall {wall:.2f} s, route {len(r['i'])} nodes")
    assert wall < 60.0
    assert np.isfinite(f.cost).mean() > 0.5 and not (f.pred == 254).any()
    assert len(r["i"]) > 500 and np.isfinite(r["height_m"]).all()
