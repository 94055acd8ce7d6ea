"""Regolith surface temperatures without a GPU: the grid and the stable step, the float64 model's
known answers (geothermal floor, constant flux, energy balance, step halving, the equator on the real ephemeris, the spin-up
drift at the chosen defaults), ephemeris.sun_flux, mrtx_thermal's argument checks and sunlight.surface_temperatures'
chunking and dates through thermal=."""
import ctypes as C
import math
from datetime import datetime, timedelta, timezone

import numpy as np
import pytest

import thermal_model as tm
from moonrtx_amd import _lib, sunlight, thermal
from moonrtx_amd import ephemeris as E
from moonrtx_amd.renderer import MoonRT

E_INVALID, E_STATE = -1, -3
T_GEO = (tm.Q_GEO / (tm.EPS * tm.SIGMA)) ** 0.25


def smooth_sun(lats, m, spacing_s=3600.0, S=1361.0):
    """Flat points at latitudes `lats` under a Sun on the equator: mu = cos(lat) cos(hour angle), f = 1, (P, m) Q_abs."""
    h = 2.0 * np.pi * np.arange(m) * spacing_s / tm.P_SYN
    mu = np.cos(np.radians(np.asarray(lats, float)))[:, None] * np.cos(h)[None, :]
    return tm.absorbed(np.ones_like(mu), mu, S)


def test_grid_and_stable_step():
    z, dz, rho, kc, zs, ref = tm.spec_grid()
    assert z.size == 22
    assert dz[0] == pytest.approx(zs / 10.0, rel=1e-12)
    assert np.allclose(dz[1:] / dz[:-1], 1.2, rtol=1e-12)
    assert z[-1] >= 20.0 * zs > z[-2]
    assert z[-1] == pytest.approx(0.68, abs=0.005)
    assert z[ref] >= 3.0 * zs > z[ref - 1]
    assert rho[0] == pytest.approx(tm.RHO_S) and kc[0] == pytest.approx(tm.K_S)
    g = thermal.grid()                                   # the library's grid is the spec's
    assert np.array_equal(g.z, z) and np.array_equal(g.rho, rho) and np.array_equal(g.kc, kc) and g.ref_node == ref
    assert tm.max_step() == pytest.approx(309.0, abs=0.5)
    assert thermal.max_step() == pytest.approx(tm.max_step(), rel=1e-12)
    md = MoonRT.thermal_grid()
    assert (md.n_nodes, md.n_sub, md.block, md.ref_node) == (22, 12, 709, ref)
    assert md.n_spin == thermal.SPINUP_LUNATIONS * 709 and md.n_reset == thermal.RESETS
    assert list(md.dz[:21]) == list(dz) and list(md.kc[:22]) == list(kc)
    assert MoonRT.thermal_grid(600.0).n_sub == 2 and MoonRT.thermal_grid(600.0).block == 4252


def test_never_lit_column_stays_at_the_geothermal_floor():
    assert T_GEO == pytest.approx(24.04, abs=0.005)
    r = tm.run(np.zeros((1, 300)), 3600.0, 12, 100, 50, 2)
    assert r["caps"] == 0 and r["coef_max"] <= 1.0
    assert np.abs(r["full"] - T_GEO).max() < 1e-3
    assert np.abs(r["summary"][0, :3] - T_GEO).max() < 1e-3


def test_constant_flux_converges_to_radiative_balance():
    F = np.array([[50.0], [500.0], [1100.0]])
    r = tm.run(np.repeat(F, 400, 1), 3600.0, 12, 200, 100, 1)
    assert r["caps"] == 0 and r["coef_max"] <= 1.0
    Ts = ((F[:, 0] + tm.Q_GEO) / (tm.EPS * tm.SIGMA)) ** 0.25
    assert np.abs(r["full"][:, -1] - Ts).max() < 0.01


def test_energy_balance_over_the_last_lunation():
    block, n_sub, sp = 709, 12, 3600.0
    z, dz, rho, kc, zs, ref = tm.spec_grid()
    V = 0.5 * (dz[:-1] + dz[1:])
    c0, c1, c2, c3, c4 = tm.C_POLY

    def enthalpy(T):       # J m^-2 in the interior nodes: rho V integral of c dT
        H = T * (c0 + T * (c1 / 2 + T * (c2 / 3 + T * (c3 / 4 + T * c4 / 5))))
        return (rho[1:-1] * V * H[:, 1:-1]).sum(1)
    cols = {}
    q = smooth_sun([0.0, 60.0], 8 * block)

    def probe(k, T):
        if k == 7 * block - 1:
            cols["a"] = T.copy()
        elif k == 8 * block - 1:
            cols["b"] = T.copy()
    # emitted from the surface temperature after each epoch's steps (a Riemann sum over one period), absorbed exactly
    r = tm.run(q, sp, n_sub, 6 * block, block, 6, probe=probe)
    assert r["caps"] == 0 and r["coef_max"] <= 1.0
    surf = r["full"][:, -block:]
    emitted = (tm.EPS * tm.SIGMA * surf ** 4).sum(1) * sp
    absorbed = q[:, -block:].sum(1) * sp
    stored = enthalpy(cols["b"]) - enthalpy(cols["a"])
    geo = tm.Q_GEO * block * sp
    assert np.all(np.abs(emitted - absorbed - geo + stored) < 0.01 * absorbed)


def test_halving_the_step_moves_the_extremes_by_less_than_0_1_K():
    q = smooth_sun([0.0], 3 * 709)
    a = tm.run(q, 3600.0, 12, 2 * 709, 709, 2)
    b = tm.run(q, 3600.0, 24, 2 * 709, 709, 2)
    for r in (a, b):
        assert r["caps"] == 0 and r["coef_max"] <= 1.0
    assert np.abs(a["summary"][0, :2] - b["summary"][0, :2]).max() < 0.1


def disc_fraction(alt_deg, alpha_deg=0.2666):
    r = np.clip(-np.asarray(alt_deg) / alpha_deg, -1.0, 1.0)
    return (np.arccos(r) - r * np.sqrt(1.0 - r * r)) / np.pi


def test_flat_equator_on_the_real_ephemeris_matches_diviner():
    t0 = datetime(2025, 1, 1, tzinfo=timezone.utc)
    n_spin, block, m = 6 * 709, 709, 7 * 709
    times = [t0 + timedelta(hours=k - n_spin) for k in range(m)]
    obs = E.Observer(52.2, 21.0, 0.0)
    alt = []
    for t in times:
        e = E.calculate_moon_ephemeris(t, False, obs)
        alt.append(E.sun_altitude_at(e.subsolar_lat, e.subsolar_lon, 0.0, 30.0))
    alt = np.array(alt)
    q = tm.absorbed(disc_fraction(alt), np.sin(np.radians(alt)), E.sun_flux(times))[None, :]
    r = tm.run(q, 3600.0, 12, n_spin, block, 5)
    assert r["caps"] == 0 and r["coef_max"] <= 1.0
    t_max, t_min = r["summary"][0, :2]
    assert 375.0 <= t_max <= 395.0 and 85.0 <= t_min <= 110.0, (t_max, t_min)


def test_spinup_drift_at_the_defaults():
    block = 709
    nsp, nres = thermal.SPINUP_LUNATIONS, thermal.RESETS
    q = smooth_sun([0.0, 60.0, 85.0], (nsp + 2) * block)
    r = tm.run(q, 3600.0, 12, nsp * block, block, nres)
    assert r["caps"] == 0 and r["coef_max"] <= 1.0
    b = r["bottom"]
    means = [b[:, i * block:(i + 1) * block].mean(1) for i in range(nsp + 2)]
    # the bottom node's lunation mean moves by under 0.25 K from the last spin-up lunation on
    assert np.abs(means[-2] - means[-3]).max() < 0.25
    assert np.abs(means[-1] - means[-2]).max() < 0.25


def test_the_model_read_from_the_struct_is_the_spec_model_at_the_defaults():
    """run(model=md) reads the grid, constants and schedule from the MrtxThermalModel the kernel receives; with the default
    model that is the spec's module constants exactly: the same bits as the schedule-argument call.  The pinned values are
    the parent's model's (the generalisation changed no number)."""
    q = smooth_sun([0.0, 60.0], 2 * 709)
    a = tm.run(q, 3600.0, 12, 709, 709, 1)
    md = MoonRT.thermal_grid(3600.0, 1, 1)
    b = tm.run(q, model=md)
    for k in ("full", "summary", "spin_surface", "bottom"):
        assert np.array_equal(a[k], b[k]), k
    assert a["caps"] == b["caps"] == 0 and a["coef_max"] == b["coef_max"] <= 1.0
    assert b["out_of_range"] == 0 and 20.0 < b["t_lo"] < b["t_hi"] < 450.0
    want = [[385.27134168829514, 97.10015556597574, 212.49605703456407, 276.81143893355227],
            [308.6550415915498, 86.41612675055936, 172.95906312411265, 220.0906013148095]]
    assert np.allclose(b["summary"], want, rtol=1e-12, atol=0.0), b["summary"].tolist()
    assert tm.max_step(md) == pytest.approx(tm.max_step(), rel=1e-15)
    assert np.array_equal(tm.absorbed(0.5, [0.1, 0.7], 1361.0, md), tm.absorbed(0.5, [0.1, 0.7], 1361.0))
    with pytest.raises(ValueError):
        tm.run(q, 3600.0, model=md)


def test_reset_at_the_last_interior_node_hangs_the_bottom_from_the_mean():
    """A 3-node grid has its reference node at N - 2 = 1.  The reset leaves node 1 as it is and sets the bottom to the
    steady step from the block's mean `top`: T2 = top + Q dz_1 / k_1(top) (the kernel's rule), not from node 1's old value.
    By hand: kc_1 = 2e-3, chi = 2.7, top = 175 K, so k_1 = 2e-3 (1 + 2.7 / 8) = 2.675e-3; Q dz_1 = 0.018 x 0.05 = 9e-4;
    T2 = 175 + 0.336448598... K."""
    T = np.array([[250.0, 180.0, 999.0]])
    tm.geotherm(T, 1, np.array([175.0]), np.array([1e-3, 2e-3, 3e-3]), np.array([0.01, 0.05]))
    assert T[0, 0] == 250.0 and T[0, 1] == 180.0
    assert T[0, 2] == pytest.approx(175.0 + 9e-4 / 2.675e-3, rel=1e-14)
    assert T[0, 2] == pytest.approx(175.336448598130841, abs=1e-12)


def test_model_diagnostics_on_a_step_onto_a_cold_column():
    """From the 24 K floor a step to 1600 W m^-2 at the default grid's 300 s step: node 1 is still cold (small c) when its
    link carries the hot surface's k, so the coefficient sum passes 1 (1.26); the column stays finite and in range.  2200 W m^-2
    at a step just under Delta_max diverges, and the diagnostics say so."""
    md = MoonRT.thermal_grid(3600.0, 1, 1)
    md.n_spin, md.block, md.n_reset = 24, 12, 2
    q = np.zeros((1, 84))
    q[0, 30:] = 1600.0
    r = tm.run(q, model=md)
    assert 1.2 < r["coef_max"] < 1.35 and r["caps"] == 0 and r["out_of_range"] == 0
    assert r["t_lo"] == pytest.approx(T_GEO, abs=1e-3) and 400.0 < r["t_hi"] < 450.0
    md.spacing_s, md.n_sub = 0.9999 * tm.max_step(md), 1
    q[0, 30:] = 2200.0
    r = tm.run(q, model=md)
    assert r["caps"] > 0 and r["out_of_range"] > 0 and not np.isfinite(r["full"][0, -1])


def test_sun_flux_at_perihelion_and_aphelion():
    peri = datetime(2025, 1, 4, 13, 28, tzinfo=timezone.utc)       # Earth at 0.983327 AU
    aph = datetime(2025, 7, 3, 19, 55, tzinfo=timezone.utc)        # Earth at 1.016644 AU
    s = E.sun_flux([peri, aph])
    for v, r, near in ((s[0], 0.983327, 1408.0), (s[1], 1.016644, 1316.0)):
        assert 1361.0 / (r + 0.0027) ** 2 <= v <= 1361.0 / (r - 0.0027) ** 2, (v, r)
        assert abs(v - near) < 8.0
    with pytest.raises(ValueError):
        E.sun_flux([datetime(2025, 1, 1)])


@pytest.fixture
def ctx(native_lib):
    c = C.c_void_p()
    rc = native_lib.mrtx_create(C.byref(_lib.MrtxConfig(0, 16, 16, 0, 1, 0, 0)), C.byref(c))
    assert rc in (0, -2) and c.value
    yield c
    native_lib.mrtx_destroy(c)


def good_epochs(m):
    s = E.scene_from_ephemeris(E.calculate_moon_ephemeris(datetime(2025, 3, 7, 21, 0, tzinfo=timezone.utc), False,
                                                          E.Observer(52.2, 21.0, 0.0)), 16, 16)
    return np.ascontiguousarray(np.stack([E.epoch_of_scene(s)] * m))


def thermal_refusals(native_lib, ctx, ok):
    """Every refusal section 3.10 lists; `ok` is the code a good call reaches (E_STATE without a DEM, 0 with one)."""
    f = native_lib.mrtx_thermal
    pts = np.array([[10.0, 20.0], [-89.5, 0.0]])
    hz = np.zeros((2, 16), np.float32)
    m = 8
    ep = good_epochs(m)
    fl = np.full(m, 1361.0)
    out = np.empty((2, m), np.float32)

    def model(**kw):
        md = MoonRT.thermal_grid(3600.0, 1, 1)
        md.n_spin, md.block, md.n_reset = 2, 1, 1
        for k, v in kw.items():
            setattr(md, k, v)
        return md

    def call(md=None, mode=1, fl=fl, m=m, dh=None, hh=hz.ctypes.data, dev=None, host=out.ctypes.data, e=ep, c=ctx):
        md = model() if md is None else md
        return f(c, pts.ctypes.data, 2, 16, dh, hh, None if e is None else e.ctypes.data,
                 None if fl is None else fl.ctypes.data, m, C.byref(md), mode, dev, host, None)
    assert call(c=None) == E_INVALID
    assert call(e=None) == E_INVALID and call(fl=None) == E_INVALID
    for mode in (-1, 3, 7):
        assert call(mode=mode) == E_INVALID, mode
    assert call(hh=None) == E_INVALID and call(dh=hz.ctypes.data) == E_INVALID
    assert call(host=None) == E_INVALID and call(dev=out.ctypes.data) == E_INVALID
    for n_nodes in (2, 0, 33, 64):
        assert call(model(n_nodes=n_nodes)) == E_INVALID, n_nodes
    for name in ("dz", "rho", "kc"):
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            md = model()
            getattr(md, name)[3] = bad
            assert call(md) == E_INVALID, (name, bad)
    for bad in (float("nan"), -1.0, float("inf")):
        g = fl.copy()
        g[5] = bad
        assert call(fl=g) == E_INVALID, bad
    assert call(model(n_spin=m)) == E_INVALID and call(model(n_spin=m + 3)) == E_INVALID
    assert call(model(n_spin=m), mode=2) == ok                # FLUX records every epoch
    assert call(model(block=0)) == E_INVALID and call(model(block=-2)) == E_INVALID
    assert call(model(n_reset=3)) == E_INVALID                # 3 blocks do not fit in 2 spin-up epochs
    assert call(model(ref_node=0)) == E_INVALID and call(model(ref_node=21)) == E_INVALID
    assert call(model(n_sub=0)) == E_INVALID
    assert call(model(n_sub=11)) == E_INVALID                 # 327 s per step: past the stable step
    assert call(model(spacing_s=0.0)) == E_INVALID and call(model(spacing_s=float("nan"))) == E_INVALID
    assert call(fl=np.full(m, 3000.0)) == E_INVALID           # radiative equilibrium above 450 K
    assert b"450" in native_lib.mrtx_last_error(ctx)
    assert call(model(emissivity=0.0)) == E_INVALID
    # the geothermal floor (q_geo / (eps sigma))^(1/4) must not lie below 20 K: q_geo >= eps sigma 20^4 = 8.62e-3 W m^-2
    q_floor = model().emissivity * model().sigma * 20.0 ** 4
    for q_geo in (0.0, 1e-3, q_floor * (1.0 - 1e-9)):
        assert call(model(q_geo=q_geo)) == E_INVALID, q_geo
        assert b"geothermal floor" in native_lib.mrtx_last_error(ctx) and b"20 K" in native_lib.mrtx_last_error(ctx)
    assert call(model(q_geo=q_floor * (1.0 + 1e-9)), mode=2) == ok
    assert call(model(q_geo=q_floor * 1.02)) == ok
    # the albedo law must stay a reflectance on [0, 90] deg: 0.2 + 0.1 + 0.3 = 1.3 at grazing incidence would absorb < 0
    for law in ((0.2, 0.1, 0.3), (0.12, -0.2, 0.0), (0.0, 0.0, 1.01)):
        md = model()
        md.albedo[:] = list(law)
        assert call(md) == E_INVALID and b"albedo" in native_lib.mrtx_last_error(ctx), law
    md = model()
    md.albedo[:] = [0.1, 0.05, 0.3]
    assert call(md) == ok
    assert call(m=(1 << 24) + 1) == E_INVALID
    for mode in (0, 1, 2):
        assert call(mode=mode) == ok, mode


def test_thermal_arguments_are_checked_before_any_device_call(native_lib, ctx):
    thermal_refusals(native_lib, ctx, E_STATE)
    assert b"displacement" in native_lib.mrtx_last_error(ctx)


class FakeRT:
    """The two device calls surface_temperatures makes, on the host: a flat horizon and the float64 model's thermal call."""
    thermal_grid = staticmethod(MoonRT.thermal_grid)
    horizon_azimuths = staticmethod(MoonRT.horizon_azimuths)

    def __init__(self):
        self.calls = []

    def horizon(self, la, lo, n_az=256, n_bis=14, stats=None, out=None):
        assert out is None
        stats["launches"] = stats.get("launches", 0) + 1
        return np.zeros((la.size, n_az), np.float32)

    def thermal(self, la, lo, hz, ep, fl, model=None, mode="summary", stats=None, n_az=None):
        self.calls.append((la.copy(), ep.shape[0], fl.copy(), model.n_spin, model.block, model.n_reset))
        assert hz.shape == (la.size, n_az) and mode == "summary"
        return np.stack([la, lo, la + lo, np.full(la.size, float(model.n_spin))], 1).astype(np.float32)


def test_surface_temperatures_chunks_and_dates_through_thermal():
    rt = FakeRT()
    t0 = datetime(2025, 6, 1, tzinfo=timezone.utc)
    la, lo = np.linspace(-89.0, -80.0, 7), np.linspace(0.0, 60.0, 7)
    r = sunlight.surface_temperatures(rt, la, lo, t0, 1.0, step_min=120, spinup_lunations=1, n_az=16, chunk=3,
                                      observer=E.Observer(52.2, 21.0, 0.0), thermal=rt.thermal)
    assert [c[0].size for c in rt.calls] == [3, 3, 1]
    assert np.array_equal(np.concatenate([c[0] for c in rt.calls]), la)
    block = int(round(29.530589 * 24 / 2))
    for _, m, fl, n_spin, blk, n_reset in rt.calls:
        assert (n_spin, blk, n_reset) == (block, block, 1) and m == block + 12
        assert fl.shape == (m,) and np.all((fl > 1300.0) & (fl < 1420.0))
    assert r.times[0] == t0 and len(r.times) == 12 and r.times[1] - r.times[0] == timedelta(hours=2)
    assert np.array_equal(r.t_max, la.astype(np.float32)) and np.array_equal(r.t_min, lo.astype(np.float32))
    assert np.all(r.t_bottom_mean == block) and r.stats["launches"] == 3
    assert np.array_equal(rt.calls[0][2], E.sun_flux([t0 + (k - block) * timedelta(hours=2) for k in range(block + 12)]))
