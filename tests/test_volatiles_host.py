"""Subsurface columns and ice-stability depths without a GPU: the water-ice law and its folded form,
the stability depth on profiles with known answers, the new symbol, struct and prototype, and mrtx_thermal_column's
argument checks, which run before any device call."""
import ctypes as C
import math

import numpy as np
import pytest

from moonrtx_amd import _lib, volatiles
from moonrtx_amd.renderer import MoonRT
from test_thermal_host import E_INVALID, E_STATE, ctx, good_epochs      # noqa: F401 -- ctx is a fixture

H2O = volatiles.H2O


def test_h2o_law_reproduces_the_triple_point():
    assert float(volatiles.vapour_pressure(273.16, H2O)) == pytest.approx(611.657, rel=1e-6)


def test_one_mm_per_gyr_is_crossed_between_100_and_101_K():
    r = volatiles.sublimation_rate(np.array([100.0, 101.0]), H2O) / H2O.rho_solid
    assert r[0] < volatiles.RATE_MAX < r[1], r * volatiles.MM_PER_GYR
    assert volatiles.RATE_MAX * volatiles.MM_PER_GYR == pytest.approx(1.0, rel=1e-15)


def test_folded_law_is_the_sublimation_rate():
    """exp(b0 - b1 / T + b2 ln T + b3 T) in float64 against sublimation_rate (whose exponent is formed in long double), to
    1e-14 relative on [200, 450] K.  There every term of the exponent is below 32 in size (b1 / T <= 28.7), so each of its
    four large roundings moves it by at most half an ulp of 32, 1.8e-15, the two small ones (b3 T, the last sum) by 1.2e-15
    together, and exp and the reference's own rounding add 2.3e-16: 8.6e-15 at worst.  Below 200 K the exponent's terms grow
    as 1 / T and float64 itself no longer gives 1e-14."""
    b = list(volatiles.law(H2O).b)
    assert b[1] == H2O.a[1] and b[3] == H2O.a[3] and b[2] == H2O.a[2] - 0.5
    assert b[0] == pytest.approx(H2O.a[0] + 0.5 * math.log(H2O.molar_mass / (2.0 * math.pi * 8.314462618)), rel=1e-15)
    T = np.linspace(200.0, 450.0, 25001)
    got = np.exp(b[0] - b[1] / T + b[2] * np.log(T) + b[3] * T)
    want = volatiles.sublimation_rate(T, H2O)
    err = np.abs(got / want - 1.0).max()
    print(f"folded law against sublimation_rate on [200, 450] K: max relative error {err:.2e}")
    assert err <= 1e-14
    assert list(volatiles.law((1.0, 2.0, 3.0, 4.0)).b) == [1.0, 2.0, 3.0, 4.0]
    with pytest.raises(ValueError):
        volatiles.law((1.0, 2.0))


def test_stability_depth_on_profiles_with_known_answers():
    z = np.array([0.0, 0.01, 0.03, 0.07, 0.15, 0.31])
    rho, rmax = H2O.rho_solid, volatiles.RATE_MAX
    # ln r linear in z: r = rmax exp(a - s z) crosses rmax at exactly z = a / s, between nodes 3 and 4 / nodes 1 and 2
    for a, s in ((2.0, 20.0), (0.4, 20.0), (3.1, 10.0)):
        e = rho * rmax * np.exp(a - s * z)
        assert float(volatiles.stability_depth(e, z, H2O)) == pytest.approx(a / s, rel=1e-12)
    # several points at once, one of each kind: crossing, stable at the surface, stable nowhere, stable exactly from a node on
    e = rho * rmax * np.stack([np.exp(2.0 - 20.0 * z), np.exp(-1.0 - 20.0 * z), np.exp(50.0 - 20.0 * z),
                               np.where(z >= 0.07, 1.0, 7.0)])
    d = volatiles.stability_depth(e, z, H2O)
    assert d.shape == (4,) and d[0] == pytest.approx(0.1, rel=1e-12) and d[1] == 0.0 and d[2] == np.inf
    assert d[3] == pytest.approx(0.07, rel=1e-12)
    # a rate of exactly rmax at the surface is stable there; a rate of exactly 0 at the first stable node gives its depth
    assert float(volatiles.stability_depth(rho * rmax * np.ones(6), z, H2O)) == 0.0
    assert float(volatiles.stability_depth(rho * rmax * np.array([5.0, 5.0, 5.0, 0.0, 0.0, 0.0]), z, H2O)) == 0.07
    # another threshold
    e = rho * rmax * np.exp(2.0 - 20.0 * z)
    assert float(volatiles.stability_depth(e, z, H2O, rate_max=rmax * math.exp(1.0))) == pytest.approx(0.05, rel=1e-12)
    # a dry lag of diffusion length l attenuates node i by l / (l + z_i): a constant rate 3 rmax is never stable when exposed,
    # and with l = 0.05 m stable where 3 l / (l + z) <= 1, z >= 0.1: ln r interpolated between nodes 3 and 4
    e = np.full(6, 3.0 * rho * rmax)
    assert float(volatiles.stability_depth(e, z, H2O)) == np.inf
    r3, r4 = 3.0 * 0.05 / 0.12, 3.0 * 0.05 / 0.20
    want = 0.07 + (0.0 - math.log(r3)) / (math.log(r4) - math.log(r3)) * 0.08
    assert 0.07 < want < 0.15
    assert float(volatiles.stability_depth(e, z, H2O, barrier_m=0.05)) == pytest.approx(want, rel=1e-12)
    with pytest.raises(ValueError):
        volatiles.stability_depth(e[:5], z, H2O)
    with pytest.raises(ValueError):
        volatiles.stability_depth(e, z, H2O, barrier_m=0.0)


def test_thermal_depths_are_the_cumulated_spacings():
    md = MoonRT.thermal_grid()
    z = MoonRT.thermal_depths(md)
    assert z.shape == (22,) and z[0] == 0.0 and np.allclose(np.diff(z), md.dz[:21], rtol=1e-15)
    assert z[-1] == pytest.approx(0.68, abs=0.005)


def test_symbol_struct_and_prototype_exist(native_lib):
    assert C.sizeof(_lib.MrtxVolatile) == 32
    res, args = _lib.SIGNATURES["mrtx_thermal_column"]
    assert res is C.c_int and len(args) == 18 and args[14] is C.POINTER(_lib.MrtxVolatile)
    fn = native_lib.mrtx_thermal_column
    assert fn.argtypes == args and native_lib.mrtx_abi_version() == 7
    assert hasattr(MoonRT, "thermal_column") and hasattr(MoonRT, "thermal_depths")


def column_refusals(native_lib, ctx, ok):
    """Every refusal section 3.16 adds; `ok` is the code a good call reaches (E_STATE without a DEM, 0 with one)."""
    pts = np.array([[10.0, 20.0], [-89.5, 0.0]])
    hz = np.zeros((2, 16), np.float32)
    m = 8
    ep = good_epochs(m)
    fl = np.full(m, 1361.0)
    out = np.empty(2 * 6 * 22 * 2, np.float64)
    md = MoonRT.thermal_grid(3600.0, 1, 1)
    md.n_spin, md.block, md.n_reset = 2, 1, 1
    good = volatiles.law(H2O)

    def call(mode, sp=good, dev=None, host=out.ctypes.data):
        return native_lib.mrtx_thermal_column(ctx, pts.ctypes.data, 2, 16, None, hz.ctypes.data, ep.ctypes.data, fl.ctypes.data,
                                              m, C.byref(md), mode, None, None, 0, None if sp is None else C.byref(sp), dev,
                                              host, None)

    def law(*b):
        return volatiles.law(b)
    for mode in (-1, 6, 9):
        assert call(mode, None) == E_INVALID, mode
    assert call(5, None) == E_INVALID and b"species" in native_lib.mrtx_last_error(ctx)
    for mode in range(5):
        assert call(mode) == E_INVALID and b"species" in native_lib.mrtx_last_error(ctx), mode
    b = list(good.b)
    for i in range(4):
        for bad in (float("nan"), float("inf"), -float("inf")):
            c = list(b)
            c[i] = bad
            assert call(5, law(*c)) == E_INVALID and b"finite" in native_lib.mrtx_last_error(ctx), (i, bad)
    # not strictly increasing on [20, 450] K: a constant, a falling law, one that turns over at 300 K (b1 / T^2 + b3 = 0)
    for c in ((0.0, 0.0, 0.0, 0.0), (0.0, -100.0, 0.0, 0.0), (0.0, 900.0, 0.0, -0.01)):
        assert call(5, law(*c)) == E_INVALID and b"increase" in native_lib.mrtx_last_error(ctx), c
    # x(450 K) = 1.6 x 450 = 720 > 700; 1.5 x 450 = 675 passes
    assert call(5, law(0.0, 0.0, 0.0, 1.6)) == E_INVALID and b"700" in native_lib.mrtx_last_error(ctx)
    assert call(5, law(0.0, 0.0, 0.0, 1.5)) == ok
    # VOLATILE's float64 pairs need an 8-byte aligned device pointer (refused before the pointer is ever used)
    assert call(5, dev=C.c_void_p(0x1004), host=None) == E_INVALID and b"aligned" in native_lib.mrtx_last_error(ctx)
    assert call(5, host=None) == E_INVALID and call(5, dev=C.c_void_p(0x1000)) == E_INVALID     # none, or both outputs
    for mode in range(5):
        assert call(mode, None) == ok, mode
    assert call(5) == ok
    if ok == E_STATE:
        assert b"displacement" in native_lib.mrtx_last_error(ctx)
    # the two older entry points know neither mode
    for mode in (4, 5):
        assert native_lib.mrtx_thermal(ctx, pts.ctypes.data, 2, 16, None, hz.ctypes.data, ep.ctypes.data, fl.ctypes.data, m,
                                       C.byref(md), mode, None, out.ctypes.data, None) == E_INVALID
        assert native_lib.mrtx_thermal_scatter(ctx, pts.ctypes.data, 2, 16, None, hz.ctypes.data, ep.ctypes.data,
                                               fl.ctypes.data, m, C.byref(md), mode, None, None, 0, None, out.ctypes.data,
                                               None) == E_INVALID


def test_column_arguments_are_checked_before_any_device_call(native_lib, ctx):     # noqa: F811
    column_refusals(native_lib, ctx, E_STATE)
