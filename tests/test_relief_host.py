"""Terrain relief without a GPU: known answers and properties of the float64 model
(tests/relief_model.py), the host scale helper, the argument validation of mrtx_relief and mrtx_relief_share, the wrapper's
split into row bands, the derived slope and aspect, the traverse penalties, and the share model against a brute-force count."""
import ctypes as C
import math

import numpy as np
import pytest

import relief_model as rm
import synth_np
from moonrtx_amd import _lib
from moonrtx_amd import relief as rl
from moonrtx_amd import traverse as tv

E_INVALID, E_STATE = -1, -3
INF = float("inf")
NAN = float("nan")
RM = 1737400.0


@pytest.fixture
def ctx(native_lib):
    """A context handle; without a GPU mrtx_create stops at its first HIP call but hands the context out."""
    c = C.c_void_p()
    rc = native_lib.mrtx_create(C.byref(_lib.MrtxConfig(0, 16, 16, 0, 1, 0, 0)), C.byref(c))
    assert rc in (0, -2) and c.value
    yield c
    native_lib.mrtx_destroy(c)


def win(**kw):
    t = dict(row0=10, col0=20, rows=8, cols=16, stride=1, ri=2, rj=3, reserved=0, radius_m=RM)
    t.update(kw)
    return _lib.MrtxRelief(**t)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- known answers
def test_a_smooth_sphere_is_level_and_smooth(native_lib):
    dem = np.ones((180, 360), np.float32)
    for s, ri, rj in ((1, 1, 1), (2, 3, 5), (1, 32, 32)):
        out = rm.relief(dem, rm.make_window(70, 350, 6, 20, stride=s, ri=ri, rj=rj))
        assert (out == 0.0).all()                         # exactly +-0, all four


@pytest.mark.parametrize("stride", [1, 2])
def test_an_index_space_plane_gives_its_gradient_and_no_residual(native_lib, stride):
    a, b = 2.0 ** -16, -3.0 * 2.0 ** -18
    H, W = 180, 360
    dem = (1.0 + a * np.arange(W)[None, :] + b * np.arange(H)[:, None]).astype(np.float32)
    assert np.array_equal(dem.astype(np.float64), 1.0 + a * np.arange(W)[None, :] + b * np.arange(H)[:, None])     # exact
    t = rm.make_window(40, 30, 50, 60, stride=stride, ri=3, rj=2)
    k = rm.scales(t, dem.shape)
    out = rm.relief(dem, t)
    ge, gn = out[..., 2].astype(np.float64), out[..., 3].astype(np.float64)
    e_ge = np.abs(ge / (a * stride * k[:, 0:1]) - 1.0).max()
    e_gn = np.abs(gn / (-b * stride * k[:, 1:2]) - 1.0).max()
    print(f"stride {stride}: ge off by {e_ge:.3g}, gn off by {e_gn:.3g}")
    assert e_ge <= 2.0 ** -23 and e_gn <= 2.0 ** -23
    assert (out[..., 1] == 0.0).all()                     # the sums are exact: no residual at all
    # the derived angles: the slope is the plane's, the descent points down the gradient
    m = rl.ReliefMap(out, (40, 30, 50, 60, stride), RM, 3, [(0, 50, 2)])
    g = np.hypot(a * stride * k[:, 0], -b * stride * k[:, 1])
    assert np.allclose(m.slope_deg, np.degrees(np.arctan(g))[:, None], rtol=1e-6)
    want = np.degrees(np.arctan2(-(a * stride * k[:, 0]), -(-b * stride * k[:, 1]))) % 360.0
    assert np.allclose(m.aspect_deg, want[:, None], atol=1e-4)
    assert ((m.aspect_deg > 180.0) & (m.aspect_deg < 270.0)).all()        # rises to the east and to the north: descends to the SW


def test_a_parabolic_trough_has_the_analytic_roughness(native_lib):
    g, rj, c0 = 2.0 ** -20, 4, 100
    H, W = 180, 360
    dem = np.broadcast_to((1.0 + g * (np.arange(W) - c0) ** 2.0)[None, :], (H, W)).astype(np.float32)
    t = rm.make_window(90, c0, 1, 1, ri=2, rj=rj)
    out = rm.relief(dem, t)[0, 0]
    d = np.arange(-rj, rj + 1, dtype=np.float64)
    want = math.sqrt((d ** 4).mean() - (d ** 2).mean() ** 2) * g * RM
    print(f"rms_m {out[1]!r} against {want!r}")
    assert out[0] == 0.0 and out[2] == 0.0 and out[3] == 0.0
    assert abs(out[1] / want - 1.0) <= 2.0 ** -21


# ---- other properties of the model
def test_nan_exactly_where_the_footprint_leaves_the_dem(native_lib):
    dem = synth_np.dem(90, 180, seed=3, craters=10)
    for s, ri in ((1, 4), (3, 2)):
        t = rm.make_window(0, 5, (90 - 1) // s + 1, 12, stride=s, ri=ri, rj=2)
        out = rm.relief(dem, t)
        r = t.row0 + np.arange(t.rows) * s
        want = (r - ri * s < 0) | (r + ri * s >= 90)
        assert want.any() and not want.all()
        assert np.array_equal(np.isnan(out).all(-1), np.broadcast_to(want[:, None], out.shape[:2]))
        assert np.array_equal(np.isnan(out).any(-1), np.isnan(out).all(-1))


def test_a_window_over_the_seam_equals_the_rolled_dem(native_lib):
    dem = synth_np.dem(90, 180, seed=4, craters=15)
    k = 37
    t = rm.make_window(20, 170, 30, 25, stride=1, ri=2, rj=5)             # columns 170 .. 194: over +-180
    a = rm.relief(dem, t)
    t2 = rm.make_window(20, (170 + k) % 180, 30, 25, stride=1, ri=2, rj=5)
    b = rm.relief(np.roll(dem, k, axis=1), t2)
    assert np.array_equal(bits(a), bits(b))
    t3 = rm.make_window(20, 2, 30, 10, stride=1, ri=2, rj=5)              # a footprint alone reaches over the seam
    assert np.array_equal(bits(rm.relief(dem, t3)), bits(rm.relief(np.roll(dem, k, axis=1), rm.make_window(20, 2 + k, 30, 10, ri=2, rj=5))))


def test_two_row_bands_equal_the_whole_window(native_lib):
    dem = synth_np.dem(90, 180, seed=5, craters=15)
    whole = rm.relief(dem, rm.make_window(1, 10, 40, 30, stride=2, ri=3, rj=2))
    top = rm.relief(dem, rm.make_window(1, 10, 17, 30, stride=2, ri=3, rj=2))
    bottom = rm.relief(dem, rm.make_window(1 + 17 * 2, 10, 23, 30, stride=2, ri=3, rj=2))
    assert np.array_equal(bits(np.concatenate([top, bottom])), bits(whole))


# ---- the scale helper
@pytest.mark.parametrize("H,W,row0,rows,stride", [(180, 360, 0, 180, 1), (1024, 2048, 3, 200, 5), (23040, 46080, 100, 64, 3)])
def test_scales_are_the_spacings_of_the_lattice(native_lib, H, W, row0, rows, stride):
    R = RM * 1.004
    k = rm.scales(win(row0=row0, rows=rows, stride=stride, cols=4, ri=1, rj=1, radius_m=R), (H, W))
    lat = np.radians(90.0 - (row0 + np.arange(rows) * stride + 0.5) * 180.0 / H)
    L_ew = R * np.cos(lat) * stride * 2.0 * np.pi / W
    L_ns = R * stride * np.pi / H
    assert np.abs(R / k[:, 0] / L_ew - 1.0).max() <= 1e-12
    assert np.abs(R / k[:, 1] / L_ns - 1.0).max() <= 1e-12


def test_scales_refuse_bad_windows(native_lib):
    f = native_lib.mrtx_relief_scales
    out = np.empty((64, 2), np.float64)

    def call(h=180, w=360, o=out, **kw):
        return f(C.byref(win(**kw)), h, w, None if o is None else o.ctypes.data)
    assert call() == 0
    assert f(None, 180, 360, out.ctypes.data) == E_INVALID
    assert call(o=None) == E_INVALID
    bad = [dict(h=1), dict(w=1), dict(row0=173), dict(row0=179, rows=2), dict(row0=0, rows=61, stride=3), dict(col0=360),
           dict(cols=361), dict(rows=4, cols=13, stride=30),                         # repeated columns
           dict(rows=4, cols=4, stride=60, rj=3),                                    # the footprint goes round the circle
           dict(stride=0), dict(rows=0), dict(ri=0), dict(rj=33), dict(reserved=1), dict(radius_m=0.0)]
    for kw in bad:
        assert call(**kw) == E_INVALID, kw
    good = [dict(row0=172), dict(row0=0, rows=60, stride=3), dict(cols=360), dict(col0=359, rows=4, cols=12, stride=30, rj=1),
            dict(rows=4, cols=4, stride=40, rj=4), dict(ri=32, rj=32)]
    for kw in good:
        assert call(**kw) == 0, kw


# ---- refusals before any device call
def test_relief_arguments_are_checked_before_any_device_call(native_lib, ctx):
    f = native_lib.mrtx_relief
    out = np.empty((8, 16, 4), np.float32)
    O = out.ctypes.data

    def call(c=ctx, dev=None, host=O, **kw):
        return f(c, C.byref(win(**kw)), dev, host, None)
    assert call(c=None) == E_INVALID
    assert f(ctx, None, None, O, None) == E_INVALID
    bad = [dict(rows=0), dict(cols=0), dict(rows=-3), dict(stride=0), dict(stride=-2), dict(row0=-1), dict(col0=-1),
           dict(ri=0), dict(rj=0), dict(ri=33), dict(rj=33), dict(ri=-1), dict(reserved=1),
           dict(rows=1 << 16, cols=(1 << 15) + 1),                                     # more than 2^31 nodes
           dict(radius_m=0.0), dict(radius_m=-1.0), dict(radius_m=NAN), dict(radius_m=INF), dict(radius_m=1e300)]
    for kw in bad:
        assert call(**kw) == E_INVALID, kw
    assert call(host=None) == E_INVALID                         # neither output
    assert call(dev=1 << 40) == E_INVALID                       # both outputs
    assert call(dev=(1 << 40) + 4, host=None) == E_INVALID      # a float4 table is 16-byte aligned
    # every argument good: the missing DEM is next (the window meets the DEM's shape after that)
    for kw in (dict(), dict(ri=1, rj=1), dict(ri=32, rj=32), dict(rows=1 << 15, cols=1 << 16), dict(stride=7), dict(row0=10 ** 6)):
        assert call(**kw) == E_STATE, kw
    assert call(dev=1 << 40, host=None) == E_STATE
    assert b"displacement" in native_lib.mrtx_last_error(ctx)


def test_relief_tile_switch_is_checked(native_lib, ctx, monkeypatch):
    out = np.empty((8, 16, 4), np.float32)
    for v, rc in (("16", E_STATE), ("32", E_STATE), ("64", E_STATE), ("0", E_STATE), ("12", E_INVALID), ("x", E_INVALID)):
        monkeypatch.setenv("MOONRT_RELIEF_TILE", v)
        assert native_lib.mrtx_relief(ctx, C.byref(win()), None, out.ctypes.data, None) == rc, v


def test_share_arguments_are_checked_before_any_device_call(native_lib, ctx):
    f = native_lib.mrtx_relief_share
    rows, cols = 8, 16
    N = rows * cols
    table = np.zeros((rows, cols, 4), np.float32)
    out = np.empty((rows, cols), np.float32)
    T, O = table.ctypes.data, out.ctypes.data
    base = 1 << 40                          # never dereferenced: every one of these calls is refused

    def call(c=ctx, dt=None, ht=T, do=None, ho=O, **kw):
        s = dict(rows=rows, cols=cols, Ri=2, Rj=3, wrap=0, reserved=0, grade_max=0.2, rms_max=1.0)
        s.update(kw)
        return f(c, C.byref(_lib.MrtxReliefShare(**s)), dt, ht, do, ho, None)
    assert call(c=None) == E_INVALID
    assert f(ctx, None, None, T, None, O, None) == E_INVALID
    bad = [dict(rows=0), dict(cols=0), dict(cols=-1), dict(rows=1 << 16, cols=(1 << 15) + 1), dict(Ri=-1), dict(Rj=-1),
           dict(Ri=1025), dict(Rj=1025), dict(wrap=2), dict(wrap=-1), dict(wrap=1, cols=2), dict(reserved=1),
           dict(grade_max=NAN), dict(grade_max=-0.1), dict(grade_max=-INF), dict(rms_max=NAN), dict(rms_max=-1.0)]
    for kw in bad:
        assert call(**kw) == E_INVALID, kw
    assert call(ht=None) == E_INVALID                           # neither table
    assert call(dt=base) == E_INVALID                           # both tables
    assert call(ho=None) == E_INVALID                           # neither output
    assert call(do=base) == E_INVALID                           # both outputs
    assert call(dt=base + 8, ht=None) == E_INVALID              # alignment
    assert call(do=base + 2, ho=None) == E_INVALID
    for dt, do in ((base, base), (base, base + 16 * N - 4), (base + 4 * N - 16, base), (base, base + 64)):
        assert call(dt=dt, ht=None, do=do, ho=None) == E_INVALID, (dt - base, do - base)
        assert b"overlap" in native_lib.mrtx_last_error(ctx)


# ---- the wrapper's band split
def test_footprint_in_metres_splits_the_window_into_bands_of_constant_rj(native_lib):
    H, W = 23040, 46080
    window = (200, 1000, 900, 64, 1)                 # 88.4 .. 81.4 N: L_ew from 6.5 m to 35 m at 237 m texels' cos(lat)
    fm = 400.0
    ri, bands = rl.footprint_bands(native_lib, window, fm, RM, (H, W))
    k = rm.scales(rm.make_window(200, 1000, 900, 64), (H, W))
    L_ew, L_ns = RM / k[:, 0], RM / k[:, 1]
    assert ri == max(1, int(math.floor(fm / 2 / L_ns[0] + 0.5)))
    assert bands[0][0] == 0 and sum(n for _, n, _ in bands) == 900 and len(bands) > 3
    for (a, n, rj), nxt in zip(bands, bands[1:] + [(900, 0, -1)]):
        assert a + n == nxt[0] and n >= 1 and 1 <= rj <= 32            # the bands cover the window, in order
        want = np.maximum(1, np.floor(fm / 2 / L_ew[a:a + n] + 0.5))
        assert (want == rj).all()
        assert rj != nxt[2]
    # nearer the pole the rows need more than 32 nodes: refused, naming a stride that fits -- and that stride does
    with pytest.raises(ValueError, match="stride of") as e:
        rl.footprint_bands(native_lib, (20, 1000, 900, 64, 1), fm, RM, (H, W))
    fit = int(str(e.value).split("stride of ")[1].split()[0])
    assert fit > 1
    ri2, bands2 = rl.footprint_bands(native_lib, (20, 1000, 900 // fit, 64, fit), fm, RM, (H, W))
    assert max(rj for _, _, rj in bands2) <= 32 and ri2 <= 32
    if fit > 2:
        with pytest.raises(ValueError):
            rl.footprint_bands(native_lib, (20, 1000, 900 // (fit - 1), 64, fit - 1), fm, RM, (H, W))
    with pytest.raises(ValueError):
        rl.footprint_bands(native_lib, window, 0.0, RM, (H, W))
    # a footprint smaller than a texel is the 3 x 3 neighbourhood
    assert rl.footprint_bands(native_lib, (11000, 0, 50, 50, 1), 10.0, RM, (H, W)) == (1, [(0, 50, 1)])


def test_penalties_from_slope_and_roughness_keep_traverses_range():
    grade = np.array([0.0, 0.1, math.tan(math.radians(15.0)), 0.5, NAN, 1e9], np.float32)
    p = tv.penalty_from_slope(grade, 20.0, weight=4.0)
    assert p.dtype == np.float32 and p[0] == 1.0 and np.isinf(p[3:]).all() and (np.diff(p[:3]) > 0).all() and p[2] < 5.0
    m = rl.ReliefMap(np.stack([grade, 10 * grade, grade, 0 * grade], -1).reshape(2, 3, 4), (0, 0, 2, 3), RM, 1, [(0, 2, 1)])
    assert np.array_equal(tv.penalty_from_slope(m, 20.0).ravel(), p)
    r = tv.penalty_from_roughness(m, 2.0, weight=1e9)
    assert r.ravel().tolist()[:2] == [1.0, 1e6] and np.isinf(r.ravel()[2:]).all()          # clamped into [1e-3, 1e6]
    assert tv.penalty_from_slope(grade[:4], 90.0).tolist() == [1.0, 1.0, 1.0, 1.0]           # no limit
    for a in (p, r):
        assert (np.isinf(a) | ((a >= np.float32(1e-3)) & (a <= np.float32(1e6)))).all() and not np.isnan(a).any()
    with pytest.raises(ValueError):
        tv.penalty_from_roughness(m, 0.0)


# ---- the share model
@pytest.mark.parametrize("Ri,Rj,wrap", [(0, 0, 0), (0, 0, 1), (2, 3, 0), (2, 3, 1), (1, 9, 1), (1, 30, 1), (40, 2, 0), (3, 40, 0)])
def test_share_model_equals_a_brute_force_count(Ri, Rj, wrap):
    rng = np.random.default_rng(11)
    rows, cols = 13, 19
    table = rng.uniform(0.0, 1.0, (rows, cols, 4)).astype(np.float32)
    table[rng.random((rows, cols)) < 0.1] = np.nan                  # NaN nodes
    table[0] = np.nan                                               # a NaN row at the map's edge
    got = rm.share(table, Ri, Rj, wrap, 0.6, 0.7)
    want = rm.share_brute(table, Ri, Rj, wrap, 0.6, 0.7)
    assert np.array_equal(bits(got), bits(want))
    assert got.min() >= 0.0 and got.max() <= 1.0 and 0.1 < got.mean() < 0.6
    if Ri == Rj == 0:
        assert np.array_equal(got, rm.safe_mask(table, 0.6, 0.7).astype(np.float32))
    assert (rm.share(table, Ri, Rj, wrap, INF, INF) == rm.share(np.where(np.isnan(table), 9.0, 0.0), Ri, Rj, wrap, 1.0, 1.0)).all()
    assert (rm.share(table, Ri, Rj, wrap, 0.0, 0.0) == 0.0).all()
