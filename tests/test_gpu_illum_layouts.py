"""The wave layouts of the march-based terrain queries on the MI355X (DESIGN.md sections 4.8, 4.9, 4.12 and 4.13), on the built
cases of tests/illum_layout_cases.py: every n_sun's PW x PH block on grids ragged against it, held to the float64 model; a
node's bits whatever its place in a wave (map, point list, single points, bands from every row residue); every branch of the
series' narrowing against the per-epoch loop; view_hits at partial last waves; viewsheds whose rows straddle a 64-column
wave; and guard bands behind the output of every march-based call."""
import ctypes as C
import math
import time

import numpy as np
import pytest

import illum_layout_cases as lc
import illum_model as im
import sight_model as sm
from common import assert_bit_equal
from moonrtx_amd import _lib
from moonrtx_amd._lib import MrtxStats
from moonrtx_amd.renderer import DeviceBuffer, MoonRT
from test_gpu_illum_series import COUNTERS, loop
from test_gpu_illumination import make, mu_tol

pytestmark = pytest.mark.gpu

FILL = 0x7FC12345               # the guard band's word: a quiet NaN of known payload
TAIL = 256
RM = 1737400.0
NARROW, WIDE, COUNT = 0, _lib.F_FORCE_WIDE, _lib.F_COUNT_STATS
WIDE_SHAPE = (9, 21)            # the shape both addressing builds run


@pytest.fixture(scope="module")
def ctxs(native_lib):
    """One context per build: production and counting, narrow and WIDE addressing.  No test changes their light or frame."""
    rts = {flags: make(lc.scene(), lc.dem(), flags) for flags in (NARROW, COUNT, WIDE, WIDE | COUNT)}
    yield rts
    for rt in rts.values():
        rt.close()


def builds(shape):
    return (NARROW, COUNT, WIDE, WIDE | COUNT) if shape == WIDE_SHAPE else (NARROW, COUNT)


def full_sun(e):
    """The irradiance of the whole disc at normal incidence, 2 L (1 - cos th_max) (tests/test_gpu_illum_series.py's)."""
    Lb, _ = im.sun_dir_moon_frame(e)
    sin2 = (e.light_radius / np.linalg.norm(Lb)) ** 2
    return 2 * e.light_radiance * sin2 / (1 + math.sqrt(1 - sin2))


def against_the_model(got, m, lat, full, what):
    """tests/test_gpu_illumination.py's bounds: lit exactly on the nodes without a flagged sample, irr within full Sun x
    mu_tol there (full: one value, or one per node), mu within mu_tol and D within 1e-6 everywhere."""
    ok = ~m["flagged"].any(-1)
    tol = mu_tol(lc.dem().shape, lat)
    assert np.array_equal(got[ok, 0], m["lit"][ok].astype(np.float32)), \
        (what, np.c_[got[ok, 0], m["lit"][ok]][got[ok, 0] != m["lit"][ok].astype(np.float32)][:6])
    assert (np.abs(got[:, 1] - m["irr"]) < tol * full)[ok].all(), what
    assert (np.abs(got[:, 2] - m["mu"]) < tol).all(), what
    assert np.abs(got[:, 3] - m["D"]).max() < 1e-6, what


def test_the_cases_sample_table_is_the_librarys(native_lib):
    """What the cases restate so that the CPU suite needs no library: the Sun tables and the node centres."""
    for n in lc.N_SUN:
        assert_bit_equal(MoonRT.sun_samples(n), lc.sun_table(n), f"n_sun {n}")
    lat, lon = lc.window()
    for shape in lc.SHAPES + ((3, 129),):
        la, lo = MoonRT.grid_nodes(lat, lon, shape)
        LA, LO = np.meshgrid(la, lo, indexing="ij")
        assert np.array_equal(np.stack([LA.ravel(), LO.ravel()]), np.stack(lc.grid_nodes(lat, lon, shape))), shape


@pytest.mark.parametrize("n_sun", lc.N_SUN)
def test_every_layout_matches_the_model(ctxs, n_sun):
    """Per grid shape: lit is the model's on every node without a flagged sample, irr, mu and D within the illumination
    stage's bounds, the counting build's shadow_rays is the model's count (a lane past the edge that marched would add to
    it), and the production, counting and WIDE builds agree bit for bit."""
    t0 = time.perf_counter()
    lat, lon = lc.window()
    full = full_sun(lc.scene())
    for shape in lc.SHAPES:
        m = lc.grid_model(shape)[n_sun]
        la, _ = lc.grid_nodes(lat, lon, shape)
        ref = None
        for flags in builds(shape):
            st = {}
            got = ctxs[flags].illumination_map(lat, lon, shape, n_sun=n_sun, stats=st).reshape(-1, 4)
            if ref is None:
                ref = got
                against_the_model(got, m, la, full, f"{shape}, n_sun {n_sun}")
            assert_bit_equal(got, ref, f"{shape}, n_sun {n_sun}: flags {flags} against production")
            if flags & COUNT:
                assert st["shadow_rays"] == m["shadow_rays"], (shape, n_sun, flags, st["shadow_rays"], m["shadow_rays"])
                assert st["launches"] == 1
    print(f"n_sun {n_sun}: {time.perf_counter() - t0:.2f} s")


def chosen(shape, n_sun):
    """The nodes asked for one at a time: all of the two smallest shapes, else 16 with the corners, the last row's and the
    last column's among them."""
    h, w = shape
    if h * w <= 16:
        return np.arange(h * w)
    rng = np.random.default_rng([h, w, n_sun])
    fixed = [0, w - 1, (h - 1) * w, h * w - 1, (h - 1) * w + w // 2, (h // 2) * w + w - 1]
    rest = rng.choice(np.setdiff1d(np.arange(h * w), fixed), 16 - len(fixed), replace=False)
    return np.concatenate([fixed, rest])


@pytest.mark.parametrize("n_sun", lc.N_SUN)
def test_a_nodes_bits_do_not_depend_on_its_place_in_a_wave(ctxs, n_sun):
    """Per grid shape, bit for bit: the map; the point list at its nodes (PW = 64 / n_sun side by side); single points (a
    wave of one node); the map put together from one-row bands, and from two bands split at every row residue modulo PH."""
    t0 = time.perf_counter()
    lat, lon = lc.window()
    for shape in lc.SHAPES:
        la, lo = lc.grid_nodes(lat, lon, shape)
        PH = lc.GRID_BLOCK[n_sun][1]
        for flags in (NARROW, WIDE) if shape == WIDE_SHAPE else (NARROW,):
            rt = ctxs[flags]
            what = f"{shape}, n_sun {n_sun}, flags {flags}"
            base = rt.illumination_map(lat, lon, shape, n_sun=n_sun)
            flat = base.reshape(-1, 4)
            assert_bit_equal(rt.illumination_at(la, lo, n_sun=n_sun), flat, f"{what}: points at the nodes")
            for i in chosen(shape, n_sun):
                assert_bit_equal(rt.illumination_at(la[i:i + 1], lo[i:i + 1], n_sun=n_sun), flat[i:i + 1], f"{what}: node {i} alone")
            rows = [rt.illumination_map(lat, lon, shape, n_sun=n_sun, rows=(r, r + 1)) for r in range(shape[0])]
            assert_bit_equal(np.concatenate(rows), base, f"{what}: one-row bands")
            for r in range(1, min(PH, shape[0] - 1) + 1):
                two = [rt.illumination_map(lat, lon, shape, n_sun=n_sun, rows=b) for b in ((0, r), (r, shape[0]))]
                assert_bit_equal(np.concatenate(two), base, f"{what}: bands split at row {r}")
    print(f"n_sun {n_sun}: {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("n_sun", lc.N_SUN)
def test_series_windows_equal_the_per_epoch_loop(native_lib, n_sun):
    """Every window length of the cases, at 1, 3 or 7 points with per-point starts: the series is the per-epoch
    illumination_at loop bit for bit in the production and the counting build, whose counters are the loop's sums; at
    n_sun 2, 8 and 32 the 33-epoch case is also held to the float64 model."""
    t0 = time.perf_counter()
    s, ep = lc.scene(), lc.epochs()
    lat, lon = lc.series_points()
    for flags in (NARROW, COUNT):
        rt = make(s, lc.dem(), flags)
        rays = 0
        for name, n, k, first, count in lc.series_cases():
            if n != n_sun:
                continue
            st_s, st_l = {}, {}
            got = rt.illumination_series(lat[:k], lon[:k], ep, n_sun=n, first=first, count=count, stats=st_s)
            want = loop(rt, s.radius, lat[:k], lon[:k], ep, first, count, n, st_l)
            assert_bit_equal(got, want, f"series vs loop: {name}, flags {flags}")
            for key in COUNTERS:
                assert st_s[key] == st_l[key], (name, key, st_s, st_l)
            rays += st_s["shadow_rays"]
            if flags == NARROW and count == 33 and n in (2, 8, 32):
                # every (point, j) of the window as one list of nodes, each under its own epoch's Sun
                table = lc.series_model()[n]
                m = {key: lc.series_window(table[key], k, first, count).reshape((k * count,) + table[key].shape[2:])
                     for key in ("flagged", "lit", "irr", "mu")}
                m["D"] = np.repeat(table["D"][:k], count)
                suns = np.array([full_sun(lc.Epoch(row, s)) for row in ep])
                against_the_model(got.reshape(-1, 4), m, np.repeat(lat[:k], count), lc.series_window(np.tile(suns, (k, 1)), k, first, count).ravel(), name)
        rt.close()
        assert (rays > 0) == bool(flags & COUNT)
    print(f"n_sun {n_sun}: {time.perf_counter() - t0:.2f} s")


VIEW_PICK = (3, 5, 10, 15, 20)


def view_points():
    """Five of tests/test_gpu_scatter.py's points(11, 24) on the egg-crate relief whose terrain share, from the float64 model
    alone, is 1/16 to 1/8 at K = 16 (at K = 32 one of them sees only sky)."""
    rng = np.random.default_rng(11)
    lat, lon = np.degrees(np.arcsin(rng.uniform(-0.95, 0.95, 24))), rng.uniform(-180.0, 180.0, 24)
    return lat[list(VIEW_PICK)], lon[list(VIEW_PICK)]


@pytest.mark.parametrize("k", [16, 32])
def test_view_hits_at_partial_waves(ctxs, k):
    """1, 3 and 5 points at K < 64: n K is no multiple of 64 (a partial last wave, several points in a wave) and the share
    kernel's one wave is short.  Hits and shares equal the per-point calls bit for bit, the shares are hits / K of the hits
    returned, and the counting build marches n K view rays."""
    lat, lon = view_points()
    for n in (1, 3, 5):
        assert (n * k) % 64
        for flags in (NARROW, COUNT):
            st = {}
            hits, share = ctxs[flags].view_hits(lat[:n], lon[:n], k=k, stats=st)
            assert hits.shape == (n, k, 2) and share.shape == (n,)
            for p in range(n):
                h1, s1 = ctxs[flags].view_hits(lat[p:p + 1], lon[p:p + 1], k=k)
                assert_bit_equal(hits[p:p + 1], h1, f"K {k}, {n} points, flags {flags}: hits of point {p}")
                assert_bit_equal(share[p:p + 1], s1, f"K {k}, {n} points, flags {flags}: share of point {p}")
            assert np.array_equal(np.isnan(hits[..., 0]), np.isnan(hits[..., 1]))
            want = ((~np.isnan(hits[..., 0])).sum(1) / float(k)).astype(np.float32)
            assert_bit_equal(share, want, f"K {k}, {n} points, flags {flags}: shares against the hits")
            assert share[0] > 0 and (share < 1).all()
            if flags & COUNT:
                assert st["bounce_rays"] == n * k, st


@pytest.mark.parametrize("w", [63, 64, 65, 129])
def test_viewshed_rows_across_a_wave_edge(ctxs, w):
    """3 x w targets about test_gpu_sight's corrugated observer (in view, from the model alone: 9 %; within the mast: 67 %):
    the map equals line_of_sight at its nodes and its one-row bands bit for bit, and the float64 model on every unflagged
    target, as a plain viewshed and with a 9-probe mast search."""
    s, dem = lc.scene(), lc.dem()
    obs = (-10.0, 60.0, 1000.0)
    g = dict(lat=(-7.0, -13.0), lon=(57.0, 63.0), shape=(3, w))
    la, lo = lc.grid_nodes(g["lat"], g["lon"], g["shape"])
    rt = ctxs[NARROW]
    for n_bis, mast in ((0, 0.0), (9, 4000.0)):
        args = dict(target_height_m=1.5, mast_max_m=mast, n_bis=n_bis, radius_m=RM)
        a = rt.viewshed(obs, **g, **args)
        assert_bit_equal(rt.line_of_sight(la, lo, obs, **args), a.ravel(), f"w {w}, n_bis {n_bis}: points at the nodes")
        bands = np.concatenate([rt.viewshed(obs, rows=(r, r + 1), **g, **args) for r in range(3)])
        assert_bit_equal(bands, a, f"w {w}, n_bis {n_bis}: one-row bands")
        assert_bit_equal(ctxs[WIDE].viewshed(obs, **g, **args), a, f"w {w}, n_bis {n_bis}: WIDE")
        m = sm.sight(s, dem, la, lo, obs, target_h_m=1.5, mast_max_m=mast, n_bis=n_bis, radius_m=RM)
        ok = ~m["flagged"]
        bad = np.flatnonzero(ok & (a.ravel() != m["m"]))
        assert bad.size == 0, (w, n_bis, [(i, a.ravel()[i], m["m"][i]) for i in bad[:6]])
        if n_bis == 0:
            assert ok.mean() > 0.9 and 0.03 < (m["m"][ok] == 0).mean() < 0.5
        else:
            assert ok.mean() > 0.3 and 0.4 < np.isfinite(m["m"]).mean() < 0.9


# ---- writes stay inside the output ---------------------------------------------------------------------------------------------
def guarded(rt, what, host, call):
    """`call(dev_ptr)` through the ABI into a device buffer TAIL words longer than `host` (the host-output call's result),
    filled with FILL: the head is the host output bit for bit, the tail is untouched."""
    words = np.ascontiguousarray(host).view(np.uint32).ravel()
    buf = DeviceBuffer((words.size + TAIL) * 4)
    try:
        buf.upload(np.full(words.size + TAIL, FILL, np.uint32))
        rt._check(call(buf.ptr), what)
        back = buf.download(np.uint32, (words.size + TAIL,))
    finally:
        buf.free()
    assert np.array_equal(back[:words.size], words), f"{what}: device output differs from host output"
    assert np.array_equal(back[words.size:], np.full(TAIL, FILL, np.uint32)), f"{what}: wrote past its {words.size} words"


@pytest.mark.parametrize("flags", [NARROW, WIDE], ids=["narrow", "wide"])
def test_writes_stay_inside_the_output(ctxs, flags):
    """Every march-based call writes its output and nothing behind it: ragged grid bands, a short series, horizons of few
    points and few azimuths, view hits with their shares directly behind, a viewshed row of 65 and 65 sight targets."""
    rt = ctxs[flags]
    lib, ctx = rt._lib, rt._ctx
    st = MrtxStats()
    lat, lon = lc.window()
    shape = WIDE_SHAPE
    for n_sun in (2, 32):
        g = _lib.MrtxIllumGrid(lat[0], lat[1], lon[0], lon[1], shape[0], shape[1], 2, 7, n_sun, 0)
        host = rt.illumination_map(lat, lon, shape, n_sun=n_sun, rows=(2, 7))
        assert host.shape == (5, 21, 4)
        guarded(rt, f"mrtx_illum_grid, n_sun {n_sun}", host, lambda dev: lib.mrtx_illum_grid(ctx, C.byref(g), dev, None, C.byref(st)))
    # 3 points x 5 epochs at n_sun = 8
    pla, plo = lc.series_points()
    pts = np.ascontiguousarray(np.stack([pla[:3], plo[:3]], -1))
    ep = np.ascontiguousarray(lc.epochs())
    first = np.array([0, 41, 75], np.int32)
    host = rt.illumination_series(pla[:3], plo[:3], ep, n_sun=8, first=first, count=5)
    guarded(rt, "mrtx_illum_series", host, lambda dev: lib.mrtx_illum_series(ctx, pts.ctypes.data, 3, ep.ctypes.data, ep.shape[0],
                                                                              first.ctypes.data, 5, 8, dev, None, C.byref(st)))
    # horizons: 3 points at 4 azimuths (16 points' worth of lanes idle), 1 point at 128 (two waves)
    hts = np.array([0.0, 2.0, 150.0])
    for n, n_az in ((3, 4), (1, 128)):
        host = rt.horizon(pla[:n], plo[:n], n_az=n_az, n_bis=8)
        guarded(rt, f"mrtx_horizon_points, {n} x {n_az}", host,
                lambda dev: lib.mrtx_horizon_points(ctx, pts.ctypes.data, n, n_az, 8, dev, None, C.byref(st)))
        host = rt.horizon(pla[:n], plo[:n], n_az=n_az, n_bis=8, height_m=hts[:n], radius_m=RM)
        guarded(rt, f"mrtx_horizon_raised, {n} x {n_az}", host,
                lambda dev: lib.mrtx_horizon_raised(ctx, pts.ctypes.data, hts.ctypes.data, RM, n, n_az, 8, dev, None, C.byref(st)))
    # view hits: 3 x 16 float2 and the 3 shares directly behind them
    vla, vlo = view_points()
    vpts = np.ascontiguousarray(np.stack([vla[:3], vlo[:3]], -1))
    hits, share = rt.view_hits(vla[:3], vlo[:3], k=16)
    host = np.concatenate([hits.ravel(), share])
    assert host.size == 3 * (2 * 16 + 1) and (share > 0).any()
    guarded(rt, "mrtx_view_hits", host, lambda dev: lib.mrtx_view_hits(ctx, vpts.ctypes.data, 3, 16, dev, None, C.byref(st)))
    # sight: a 3 x 65 viewshed and 65 targets
    obs = (-10.0, 60.0, 1000.0)
    g = dict(lat=(-7.0, -13.0), lon=(57.0, 63.0), shape=(3, 65))
    args = dict(target_height_m=1.5, mast_max_m=4000.0, n_bis=9, radius_m=RM)
    host = rt.viewshed(obs, **g, **args)
    sg = _lib.MrtxSightGrid(obs[0], obs[1], obs[2], 1.5, 4000.0, RM, g["lat"][0], g["lat"][1], g["lon"][0], g["lon"][1], 3, 65, 0, 3, 9, 0)
    guarded(rt, "mrtx_sight_grid", host, lambda dev: lib.mrtx_sight_grid(ctx, C.byref(sg), dev, None, C.byref(st)))
    la, lo = lc.grid_nodes(g["lat"], g["lon"], (1, 65))
    tp = np.ascontiguousarray(np.stack([la, lo], -1))
    ob = np.ascontiguousarray(np.asarray(obs, np.float64).reshape(1, 3))
    host = rt.line_of_sight(la, lo, obs, **args)
    assert np.isfinite(host).any() and np.unique(host).size > 8      # mast heights along the row: a head worth comparing
    guarded(rt, "mrtx_sight_points", host, lambda dev: lib.mrtx_sight_points(ctx, tp.ctypes.data, 65, ob.ctypes.data, 1, 1.5, 4000.0, RM,
                                                                              9, dev, None, C.byref(st)))
