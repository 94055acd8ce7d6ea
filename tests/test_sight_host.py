"""Terrain line of sight without a GPU: argument validation of mrtx_sight_grid / mrtx_sight_points,
the float64 model's known answers on a smooth sphere, and how MoonRT.viewshed / line_of_sight split and pass their calls."""
import ctypes as C
import math

import numpy as np
import pytest

import sight_model as sm
from moonrtx_amd import _lib
from moonrtx_amd import renderer as rmod
from moonrtx_amd.renderer import MoonRT
from moonrtx_amd.scene import named_scene

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


def good_grid(**kw):
    g = dict(obs_lat=10.0, obs_lon=20.0, obs_h_m=2.0, target_h_m=0.0, mast_max_m=100.0, radius_m=1737400.0,
             lat_north=20.0, lat_south=0.0, lon_west=10.0, lon_east=30.0, h=8, w=16, row_begin=0, row_end=8, n_bis=6,
             reserved=0)
    g.update(kw)
    return _lib.MrtxSightGrid(**g)


def test_sight_grid_arguments_are_checked_before_any_device_call(native_lib, ctx):
    f = native_lib.mrtx_sight_grid
    out = np.empty((8, 16), np.float32)
    O = out.ctypes.data

    def call(dev=None, host=O, c=ctx, **kw):
        return f(c, C.byref(good_grid(**kw)), dev, host, None)
    assert f(None, C.byref(good_grid()), None, O, None) == E_INVALID
    assert f(ctx, None, None, O, None) == E_INVALID
    assert call(host=None) == E_INVALID                      # neither output
    assert call(dev=O) == E_INVALID                          # both outputs
    assert native_lib.mrtx_last_error(ctx)
    bad = [dict(obs_lat=NAN), dict(obs_lat=90.5), dict(obs_lat=-91.0), dict(obs_lon=INF), dict(obs_lon=2e6),
           dict(obs_h_m=-1.0), dict(obs_h_m=NAN), dict(obs_h_m=INF), dict(obs_h_m=1.1e9),
           dict(target_h_m=-0.5), dict(target_h_m=NAN), dict(target_h_m=2e9),
           dict(mast_max_m=0.0), dict(mast_max_m=-5.0), dict(mast_max_m=NAN), dict(mast_max_m=INF), dict(mast_max_m=1e10),
           dict(radius_m=0.0), dict(radius_m=-1737400.0), dict(radius_m=NAN), dict(radius_m=INF),
           dict(n_bis=-1), dict(n_bis=25), dict(n_bis=100),
           # what mrtx_illum_grid refuses
           dict(lat_north=0.0), dict(lat_north=91.0), dict(lat_south=-90.5), dict(lat_north=NAN), dict(lon_east=10.0),
           dict(lon_west=INF), dict(lon_east=2e6), dict(h=0), dict(w=0), dict(w=-3), dict(row_begin=-1), dict(row_end=9),
           dict(row_begin=4, row_end=4), dict(row_begin=5, row_end=3),
           dict(h=1 << 20, w=1 << 12, row_begin=0, row_end=(1 << 19) + 1)]     # a band of more than 2^31 nodes
    for kw in bad:
        assert call(**kw) == E_INVALID, kw
    # every argument good: the missing DEM is next
    for kw in (dict(), dict(n_bis=0, mast_max_m=0.0), dict(n_bis=24), dict(obs_h_m=1e9, target_h_m=1e9, mast_max_m=1e9),
               dict(row_begin=3, row_end=5), dict(obs_lat=-90.0, lon_west=170.0, lon_east=200.0)):
        assert call(**kw) == E_STATE, kw
    assert b"displacement" in native_lib.mrtx_last_error(ctx)


def test_sight_points_arguments_are_checked_before_any_device_call(native_lib, ctx):
    f = native_lib.mrtx_sight_points
    pts = np.array([[10.0, 20.0], [-5.0, 190.0], [-89.5, 0.0]])
    obs = np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 0.0], [0.0, 0.0, 10.0]])
    out = np.empty(3, np.float32)
    O = out.ctypes.data

    def call(p=pts, n=3, o=obs, no=1, th=0.0, mm=50.0, rm=1737400.0, nb=8, dev=None, host=O, c=ctx):
        return f(c, None if p is None else p.ctypes.data, n, None if o is None else o.ctypes.data, no, th, mm, rm, nb, dev,
                 host, None)
    assert call(c=None) == E_INVALID
    assert call(p=None) == E_INVALID
    assert call(o=None) == E_INVALID
    assert call(host=None) == E_INVALID
    assert call(dev=O) == E_INVALID
    for kw in (dict(n=0), dict(n=-1), dict(no=0), dict(no=2), dict(no=4), dict(no=-1), dict(th=-1.0), dict(th=NAN),
               dict(th=1.5e9), dict(mm=0.0), dict(mm=-1.0), dict(mm=INF), dict(rm=0.0), dict(rm=-1.0), dict(rm=NAN),
               dict(nb=-1), dict(nb=25)):
        assert call(**kw) == E_INVALID, kw
    for bad in ([90.5, 0.0], [-91.0, 0.0], [NAN, 0.0], [0.0, INF], [0.0, 2e6]):
        p = pts.copy()
        p[1] = bad
        assert call(p=p) == E_INVALID, bad
    for bad in ([91.0, 0.0, 0.0], [NAN, 0.0, 0.0], [0.0, INF, 0.0], [0.0, 0.0, -1.0], [0.0, 0.0, NAN], [0.0, 0.0, 2e9]):
        o = obs.copy()
        o[2] = bad
        assert call(o=o, no=3) == E_INVALID, bad
    o = obs.copy()
    o[2] = [0.0, 0.0, -1.0]
    assert call(o=o, no=1) == E_STATE                         # only the first observer is read when it is shared
    # good arguments: the missing DEM
    for kw in (dict(), dict(no=3), dict(nb=0, mm=0.0), dict(nb=24), dict(n=1, no=1)):
        assert call(**kw) == E_STATE, kw


def smooth(D=0.999):
    return np.full((90, 180), D, np.float32)


def along_equator(theta_deg):
    return np.zeros_like(theta_deg), np.asarray(theta_deg, float)


def chord_low(ra, rb, theta):
    """The least radius along the chord between points at radii ra and rb, theta apart at the centre."""
    A = np.stack([np.zeros_like(theta) + ra, np.zeros_like(theta)], -1)
    B = np.stack([rb * np.cos(theta), rb * np.sin(theta)], -1)
    t = B - A
    s = np.clip(-(A * t).sum(-1) / (t * t).sum(-1), 0.0, 1.0)
    return np.sqrt(((A + s[:, None] * t) ** 2).sum(-1))


def test_model_on_a_smooth_sphere():
    """D constant: two raised points see each other iff theta < acos(R'/(R'+a)) + acos(R'/(R'+b)), R' = R D, a and b their
    heights including scene_eps -- away from the band the march step leaves: a chord that dips below the surface by less
    than a step's sag (step^2 / 8 R') can fall between two steps."""
    s = named_scene("S1", 16, 16)
    D = 0.999
    R = s.radius * D
    rm = 1737400.0
    for h_obs, h_t in ((0.0, 0.0), (2000.0, 0.0), (500.0, 3000.0), (1e5, 10.0)):
        a = s.scene_epsilon + sm.scene_height(s, h_obs, rm)
        b = s.scene_epsilon + sm.scene_height(s, h_t, rm)
        lim = math.degrees(math.acos(R / (R + a)) + math.acos(R / (R + b)))
        th = np.concatenate([np.linspace(0.02, 2.0 * lim, 60), [lim * 0.98, lim * 1.02]])
        la, lo = along_equator(th)
        m = sm.sight(s, smooth(D), la, lo, (0.0, 0.0, h_obs), target_h_m=h_t, radius_m=rm)
        want = sm.sphere_visible(R, a, b, np.radians(th))
        sag = s.marching_step ** 2 / (8 * R)
        near = np.abs(chord_low(R + a, R + b, np.radians(th)) - R) < 4 * sag + 2e-5
        vis = m["m"] == 0
        assert np.array_equal(vis[~near], want[~near]), (h_obs, h_t, th[~near][vis[~near] != want[~near]])
        assert (~near).sum() > 40
        assert set(np.unique(m["m"]).tolist()) <= {0.0, INF}


def test_model_mast_height_on_a_smooth_sphere():
    """The least mast over the target is R'/cos(theta - acos(R'/(R'+a))) - R' - b; the bisection lands within one final step
    (mast_max / 2^(n_bis - 1)) of it, plus what a step's sag is worth in height."""
    s = named_scene("S1", 16, 16)
    D = 0.999
    R = s.radius * D
    rm = 1737400.0
    h_obs, mast, n_bis = 50.0, 20000.0, 12
    a = s.scene_epsilon + sm.scene_height(s, h_obs, rm)
    b = s.scene_epsilon
    lim = math.degrees(math.acos(R / (R + a)) + math.acos(R / (R + b)))
    th = np.linspace(lim * 1.2, lim * 3.0, 25)
    la, lo = along_equator(th)
    m = sm.sight(s, smooth(D), la, lo, (0.0, 0.0, h_obs), mast_max_m=mast, n_bis=n_bis, radius_m=rm)
    want_m = sm.sphere_mast(R, a, b, np.radians(th)) * rm / s.radius
    assert np.isfinite(m["m"]).all() and (m["m"] > 0).all()
    sag_m = s.marching_step ** 2 / (8 * R) * rm / s.radius
    tol = mast / 2 ** (n_bis - 1) + 4 * sag_m + 1.0
    assert np.all(m["m"] >= want_m - 4 * sag_m - 1.0), (m["m"] - want_m)
    assert np.all(m["m"] - want_m <= tol), (m["m"] - want_m, tol)
    # beyond the reach of mast_max: +inf
    x2 = 2 * mast / rm * s.radius
    beyond = math.degrees(math.acos(R / (R + a)) + math.acos(R / (R + b + x2)))
    far = sm.sight(s, smooth(D), [0.0], [beyond], (0.0, 0.0, h_obs), mast_max_m=mast, n_bis=n_bis, radius_m=rm)
    assert far["m"][0] == INF
    # the counters: 10 vertex taps per target, probes = 1 (seen at once), 2 (+inf) or 2 + n_bis - 1
    assert set(np.unique(m["probes"]).tolist()) <= {1, 2, n_bis + 1}
    assert m["shadow_rays"] == int(m["probes"].sum())


def test_model_is_symmetric_and_sees_over_nothing_when_the_ends_coincide():
    s = named_scene("S1", 16, 16)
    dem = smooth()
    # the same point: L = 0 (or only the target's mast apart: ends closer than a step have no steps) -> clear
    same = sm.sight(s, dem, [3.0], [4.0], (3.0, 4.0, 0.0))
    assert same["m"][0] == 0.0 and same["height_samples"] == 10
    # swapping the two ends with their heights gives the same answer
    la, lo = np.linspace(-3, 3, 7), np.linspace(0.5, 4.0, 7)
    fw = sm.sight(s, dem, la, lo, np.stack([np.zeros(7), np.zeros(7), np.full(7, 900.0)], -1), target_h_m=0.0)
    bw = np.concatenate([sm.sight(s, dem, [0.0], [0.0], (la[i], lo[i], 0.0), target_h_m=900.0)["m"] for i in range(7)])
    assert np.array_equal(fw["m"], bw)


class FakeBuffer:
    made = []

    def __init__(self, nbytes, device=0):
        self.nbytes, self.ptr, self.data, self.freed = int(nbytes), 0x1000 * (len(FakeBuffer.made) + 1), None, False
        FakeBuffer.made.append(self)

    def download(self, dtype, shape):
        return np.asarray(self.data, dtype).reshape(shape)

    def free(self):
        self.freed = True


class FakeLib:
    """mrtx_sight_grid / mrtx_sight_points on the host: a node's value is 1000 * row + column of the whole map; a point's
    is its index in the call plus 0.25 x (the observer's index, shared = 0)."""

    def __init__(self):
        self.calls = []

    def mrtx_sight_grid(self, ctx, gref, dev, host, st):
        g = gref._obj
        self.calls.append(("grid", g.row_begin, g.row_end, g.w, g.n_bis, g.mast_max_m, g.obs_h_m, dev is not None))
        rows = np.arange(g.row_begin, g.row_end)[:, None] * 1000.0 + np.arange(g.w)[None, :]
        vals = rows.astype(np.float32)
        if host is not None:
            C.memmove(host, vals.ctypes.data, vals.nbytes)
        else:
            next(b for b in FakeBuffer.made if b.ptr == dev).data = vals.copy()
        st._obj.launches = 1
        return 0

    def mrtx_sight_points(self, ctx, pts, n, obs, n_obs, th, mm, rm, nb, dev, host, st):
        o = np.ctypeslib.as_array((C.c_double * (3 * n_obs)).from_address(obs)).reshape(n_obs, 3)
        p = np.ctypeslib.as_array((C.c_double * (2 * n)).from_address(pts)).reshape(n, 2)
        self.calls.append(("points", n, n_obs, float(p[0, 0]), float(o[0, 0]), th, mm, rm, nb))
        vals = (np.arange(n) + (0.25 * np.arange(n) if n_obs > 1 else 0.0)).astype(np.float32)
        C.memmove(host, vals.ctypes.data, vals.nbytes)
        st._obj.launches = 1
        return 0

    def mrtx_get_config(self, ctx, cfg):
        return 0


def fake_rt(monkeypatch):
    FakeBuffer.made.clear()
    monkeypatch.setattr(rmod, "DeviceBuffer", FakeBuffer)
    rt = MoonRT.__new__(MoonRT)
    rt._lib = FakeLib()
    rt._ctx = None
    return rt


def test_viewshed_streams_bands(monkeypatch):
    rt = fake_rt(monkeypatch)
    st = {}
    whole = rt.viewshed((1.0, 2.0, 30.0), lat=(10, -10), lon=(0, 40), shape=(10, 6), mast_max_m=50.0, n_bis=7, stats=st)
    want = (np.arange(10)[:, None] * 1000.0 + np.arange(6)[None, :]).astype(np.float32)
    assert whole.shape == (10, 6) and whole.dtype == np.float32 and np.array_equal(whole, want)
    assert rt._lib.calls == [("grid", 0, 10, 6, 7, 50.0, 30.0, False)] and st["launches"] == 1 and not FakeBuffer.made
    # bands of 4 rows x 6 columns x 4 bytes through one device buffer
    rt._lib.calls.clear()
    st = {}
    band = rt.viewshed((1.0, 2.0, 30.0), lat=(10, -10), lon=(0, 40), shape=(10, 6), rows=(1, 10), band_bytes=4 * 6 * 4,
                       stats=st)
    assert np.array_equal(band, want[1:10])
    assert [c[1:3] for c in rt._lib.calls] == [(1, 5), (5, 9), (9, 10)] and all(c[-1] for c in rt._lib.calls)
    assert len(FakeBuffer.made) == 1 and FakeBuffer.made[0].freed and FakeBuffer.made[0].nbytes == 4 * 6 * 4
    assert st["launches"] == 3
    with pytest.raises(ValueError):
        rt.viewshed((1.0, 2.0))
    with pytest.raises(ValueError):
        rt.viewshed(np.zeros((2, 3)))


def test_line_of_sight_chunks_and_observers(monkeypatch):
    rt = fake_rt(monkeypatch)
    la, lo = np.linspace(-5, 5, 10), np.linspace(0, 9, 10)
    got = rt.line_of_sight(la, lo, (1.0, 2.0, 3.0), target_height_m=2.0, mast_max_m=40.0, n_bis=5, radius_m=1.5e6,
                           chunk_bytes=16)
    # 4 targets per call, one shared observer
    assert np.array_equal(got, np.array([0, 1, 2, 3, 0, 1, 2, 3, 0, 1], np.float32))
    assert [c[1:3] for c in rt._lib.calls] == [(4, 1), (4, 1), (2, 1)]
    assert [c[3] for c in rt._lib.calls] == [la[0], la[4], la[8]]
    assert all(c[4] == 1.0 and c[5:] == (2.0, 40.0, 1.5e6, 5) for c in rt._lib.calls)
    # one observer per target: each call gets its own slice of them
    rt._lib.calls.clear()
    obs = np.stack([np.arange(10.0), np.zeros(10), np.ones(10)], -1)
    got = rt.line_of_sight(la, lo, obs, chunk_bytes=16)
    assert np.array_equal(got, np.array([0, 1.25, 2.5, 3.75, 0, 1.25, 2.5, 3.75, 0, 1.25], np.float32))
    assert [(c[2], c[4]) for c in rt._lib.calls] == [(4, 0.0), (4, 4.0), (2, 8.0)]
    # one call by default
    rt._lib.calls.clear()
    assert rt.line_of_sight(la, lo, (0, 0, 0)).shape == (10,) and len(rt._lib.calls) == 1
    for bad in (np.zeros((9, 3)), np.zeros((10, 2)), (1.0, 2.0)):
        with pytest.raises(ValueError):
            rt.line_of_sight(la, lo, bad)
    with pytest.raises(ValueError):
        rt.line_of_sight(la, lo[:5], (0, 0, 0))
