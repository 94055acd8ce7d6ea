"""The regolith column (thermal_kernel<WIDE, EXT>, DESIGN.md sections 3.10 and 3.11) against the float64 model over the
models and fluxes the ABI accepts, not only the default one: node counts 3, 4, 22, 31 and 32, the reference node at 1, in the
middle and at N - 2, one step per epoch at Delta_max, 12 at 1 h and 175 at 15 h, every spin-up shape (none, no reset, whole
blocks, a partial block after the last reset, blocks of one epoch, one recorded epoch), chi = 0, a constant heat capacity, a
non-default emissivity, sigma and albedo, q_geo just above the 20 K floor; 1 to 130 points; the production schedule; and
synthetic fluxes fed through mrtx_thermal_scatter's extra table, steps onto a cold column included.  Every case prints its
largest error against the model.  Then what the range checks refuse: q_geo = 0 before launch, and a 2200 W m^-2 step at a
step just under Delta_max, which the model says diverges, after it (the kernel's per-epoch range flag)."""
import math
import re
import time
from datetime import datetime, timedelta, timezone

import numpy as np
import pytest

import model_cases as mc
import thermal_model as tm
from common import assert_bit_equal
from moonrtx_amd import ephemeris as E
from moonrtx_amd import thermal
from moonrtx_amd.renderer import DeviceBuffer, MoonRT, MoonRTError
from moonrtx_amd.scene import named_scene
from test_gpu_illumination import make

pytestmark = pytest.mark.gpu

OBS = E.Observer(52.2, 21.0, 0.0)
T_TOL = 0.05              # test_gpu_thermal.T_TOL: the float32 rates and surface solve against the float64 model
RANGE_MSG = "left the model's range [20, 450] K"


def points(seed, n):
    rng = np.random.default_rng(seed)
    return np.degrees(np.arcsin(rng.uniform(-0.95, 0.95, n))), rng.uniform(-180.0, 180.0, n)


def epochs(m, spacing_s=3600.0):
    t0 = datetime(2025, 3, 1, tzinfo=timezone.utc)
    times = [t0 + timedelta(seconds=k * spacing_s) for k in range(m)]
    return E.sun_epochs(times, OBS), E.sun_flux(times)


def es_of(md):
    return md.emissivity * md.sigma


def custom_model(dz, ref, spacing_s, n_spin, block, n_reset, n_sub=None, **consts):
    """An MrtxThermalModel on the layer spacings `dz` (rho and kc from the spec's depth laws at the nodes' depths), the
    default constants unless `consts` names them (chi, c, emissivity, sigma, q_geo, albedo), and n_sub the fewest stable
    steps per epoch unless given."""
    md = MoonRT.thermal_grid(3600.0, 1, 1)
    dz = np.asarray(dz, np.float64)
    n = dz.size + 1
    z = np.concatenate([[0.0], np.cumsum(dz)])
    rho = thermal.RHO_D - (thermal.RHO_D - thermal.RHO_S) * np.exp(-z / thermal.H_RHO)
    kc = thermal.K_D - (thermal.K_D - thermal.K_S) * (thermal.RHO_D - rho) / (thermal.RHO_D - thermal.RHO_S)
    md.n_nodes, md.ref_node = n, ref
    for a in (md.dz, md.rho, md.kc):
        a[:] = [0.0] * len(a)
    md.dz[:n - 1], md.rho[:n], md.kc[:n] = list(dz), list(rho), list(kc)
    for k, v in consts.items():
        if k in ("c", "albedo"):
            getattr(md, k)[:] = list(v)
        else:
            setattr(md, k, v)
    md.spacing_s, md.n_spin, md.block, md.n_reset = float(spacing_s), n_spin, block, n_reset
    md.n_sub = int(math.ceil(spacing_s / tm.max_step(md))) if n_sub is None else n_sub
    assert md.spacing_s / md.n_sub <= tm.max_step(md)
    return md


def geometric(n, d0, g):
    return d0 * g ** np.arange(n - 1)


Q_FLOOR = 0.95 * 5.670374419e-8 * 20.0 ** 4     # the smallest q_geo the ABI accepts at the default emissivity and sigma


def sweep():
    """(id, model, m): the models of the real-Sun sweep.  Each axis value of the issue's table appears at least once."""
    cases = []
    # N = 3: ref = 1 = N - 2, one step per epoch at Delta_max, n_reset * block == n_spin, chi = 0
    md = custom_model([0.02, 0.1], 1, 3600.0, 300, 100, 3, chi=0.0)
    md.spacing_s, md.n_sub = 0.999 * tm.max_step(md), 1
    cases.append(("n3_ref1_one_step_at_dmax_chi0", md, 500))
    # N = 4: ref = 2 = N - 2, no spin-up at all (the column starts on the floor under the Sun), a constant heat capacity
    cases.append(("n4_ref2_no_spinup_const_c", custom_model([0.01, 0.03, 0.1], 2, 3600.0, 0, 1, 0, c=(600.0, 0, 0, 0, 0)),
                  400))
    # the default grid with ref = 1, 12 steps at 1 h, a partial block after the last reset, q_geo just above the floor and
    # another albedo law
    md = MoonRT.thermal_grid(3600.0, 1, 1)
    md.ref_node, md.n_spin, md.block, md.n_reset, md.q_geo = 1, 250, 100, 2, 1.02 * Q_FLOOR
    md.albedo[:] = [0.1, 0.05, 0.3]
    cases.append(("n22_ref1_partial_block_low_qgeo_albedo", md, 400))
    # N = 31: ref in the middle, spin-up without resets, a non-default emissivity and sigma
    cases.append(("n31_ref15_no_reset_eps_sigma",
                  custom_model(geometric(31, 0.004, 1.1), 15, 3600.0, 200, 200, 0, emissivity=0.9, sigma=5.6e-8), 350))
    # N = 32: ref = N - 2, blocks of one epoch, a reset after every spin-up epoch
    cases.append(("n32_ref30_block1", custom_model(geometric(32, 0.004, 1.095), 30, 3600.0, 40, 1, 40), 240))
    # the default grid at 15 h: the fewest stable steps (175), one lunation of spin-up, one recorded epoch
    md = MoonRT.thermal_grid(54000.0, 1, 1)
    assert md.n_sub == 175 and md.block == 47
    cases.append(("n22_ref11_15h_one_recorded", md, 48))
    return cases


@pytest.fixture(scope="module")
def rt():
    r = make(named_scene("S1", 16, 16), mc.crater_dem(), 0)
    yield r
    r.close()


def against_model(tag, full, summ, r, st):
    """FULL and SUMMARY against the model's run r; prints the margins and the model's diagnostics."""
    assert np.isfinite(full).all() and full.shape == r["full"].shape
    d = np.abs(full - r["full"])
    ds = np.abs(summ - r["summary"]).max(0)
    print(f"\n{tag}: FULL max err {d.max():.2e} K (mean {d.mean():.2e}); SUMMARY max err (max, min, mean, bottom) "
          f"{ds[0]:.1e} {ds[1]:.1e} {ds[2]:.1e} {ds[3]:.1e} K; range {full.min():.2f}-{full.max():.2f} K; model: coef_max "
          f"{r['coef_max']:.3f}, nodes in {r['t_lo']:.2f}-{r['t_hi']:.2f} K, caps {r['caps']}; device caps "
          f"{st.get('newton_cap_hits')}")
    assert d.max() < T_TOL, tag
    assert ds.max() < T_TOL, tag
    assert r["caps"] == 0 and st["newton_cap_hits"] == 0, tag
    assert r["out_of_range"] == 0


@pytest.mark.parametrize("case", sweep(), ids=lambda c: c[0])
def test_real_sun_over_the_model_sweep(native_lib, rt, case):
    """On crater_dem under the real Sun, per model: FLUX against the float64 absorbed flux with that model's albedo, FULL and
    SUMMARY against the model fed the device's FLUX, and EXT with an all-zero extra table equal to mrtx_thermal bit for bit."""
    tag, md, m = case
    lat, lon = points(17, 24)
    ep, fl = epochs(m, md.spacing_s)
    hz = rt.horizon(lat, lon, n_az=64, n_bis=12)
    st = {}
    flux = rt.surface_temperature(lat, lon, hz, ep, fl, md, mode="flux")
    full = rt.surface_temperature(lat, lon, hz, ep, fl, md, mode="full", stats=st)
    summ = rt.surface_temperature(lat, lon, hz, ep, fl, md, mode="summary", stats=st)
    f = rt.horizon_sun(lat, lon, hz, ep)
    mu = rt.illumination_series(lat, lon, ep, n_sun=1)[..., 2]
    dark = (f == 0.0) | (mu <= 0.0)
    assert np.all(flux[dark] == 0.0) and (~dark).mean() > 0.2
    want = tm.absorbed(f.astype(np.float64), mu.astype(np.float64), fl[None, :].astype(np.float32).astype(np.float64), md)
    assert np.all(np.abs(flux[~dark] - want[~dark]) <= 4e-6 * want[~dark] + 1e-4)
    t = time.process_time()
    r = tm.run(flux.astype(np.float64), model=md)
    print(f"\n{tag}: model {time.process_time() - t:.1f} s CPU for {lat.size} points x {m} epochs x {md.n_sub} steps")
    against_model(tag, full, summ, r, st)
    zero = np.zeros((lat.size, m), np.float32)
    for mode, want in (("full", full), ("summary", summ)):
        assert_bit_equal(rt.surface_temperature_scatter(lat, lon, hz, ep, fl, md, mode=mode, extra_flux=zero), want,
                         f"{tag}: EXT {mode} with a zero table")


SYN_P, SYN_SPIN, SYN_REC = 70, 24, 96
SYN_KINDS = ("constant", "zero", "square", "spike", "step 1244", "step 1600")


def synthetic_flux():
    """(70, m) float32: row p is history p % 6 of SYN_KINDS, phase-shifted by p // 6 epochs (a constant row's level by it),
    so a row stored in another row's place shows up."""
    m = SYN_SPIN + SYN_REC
    q = np.zeros((SYN_P, m), np.float32)
    k = np.arange(m)
    for p in range(SYN_P):
        kind, ph = p % 6, p // 6
        if kind == 0:
            q[p] = 100.0 + 90.0 * ph
        elif kind == 2:
            q[p] = np.where(((k + ph) // 12) % 2 == 0, 1000.0, 0.0)
        elif kind == 3:
            q[p, SYN_SPIN + 10 + ph] = 1244.0
        elif kind >= 4:
            q[p, SYN_SPIN + 5 + ph:] = 1244.0 if kind == 4 else 1600.0
    return q


def dark_points(n):
    """n points whose host horizon is 90 deg all round: f == 0, so Q_abs == 0 exactly and the extra table is the flux."""
    lat, lon = points(23, n)
    return lat, lon, np.full((n, 16), 90.0, np.float32)


def test_synthetic_flux_through_the_extra_table(native_lib, rt):
    """Constant, zero, square-wave, spike and step histories (steps from the floor to 1244 and 1600 W m^-2: node 1 is still
    cold when its link carries the hot surface's k, and the model's coefficient sum passes 1 -- 1.15 and 1.26 -- yet stays
    finite) on the default grid, 12 steps an hour: FULL, all four SUMMARY columns and EXITANCE's M_ir against the model,
    known answers for the constant and zero rows, host and device tables the same bits."""
    md = MoonRT.thermal_grid(3600.0, 1, 1)
    md.n_spin, md.block, md.n_reset = SYN_SPIN, 12, 2
    q = synthetic_flux()
    m = q.shape[1]
    lat, lon, hz = dark_points(SYN_P)
    ep, _ = epochs(m)
    fl = np.zeros(m)                  # no sunlight: the radiative-equilibrium check sees the table alone
    st = {}
    full = rt.surface_temperature_scatter(lat, lon, hz, ep, fl, md, mode="full", extra_flux=q, stats=st)
    summ = rt.surface_temperature_scatter(lat, lon, hz, ep, fl, md, mode="summary", extra_flux=q, stats=st)
    ex = rt.surface_temperature_scatter(lat, lon, hz, ep, fl, md, mode="exitance", extra_flux=q, stats=st)
    assert_bit_equal(rt.surface_temperature_scatter(lat, lon, hz, ep, fl, md, mode="flux", extra_flux=q), q, "FLUX = table")
    buf = DeviceBuffer(q.nbytes)
    buf.upload(q)
    assert_bit_equal(rt.surface_temperature_scatter(lat, lon, hz, ep, fl, md, mode="full", extra_flux=buf), full,
                     "device table")
    buf.free()
    t = time.process_time()
    r = tm.run(q.astype(np.float64), model=md)
    print(f"\nsynthetic: model {time.process_time() - t:.1f} s CPU")
    for kind in range(6):
        rows = np.arange(kind, SYN_P, 6)
        d = np.abs(full[rows] - r["full"][rows]).max()
        print(f"synthetic {SYN_KINDS[kind]}: FULL max err {d:.2e} K, range {full[rows].min():.2f}-{full[rows].max():.2f} K")
    against_model("synthetic", full, summ, r, st)
    assert r["coef_max"] > 1.2          # the steps onto the cold column: the bound's same-temperature premise fails
    es = es_of(md)
    const = np.arange(0, SYN_P, 6)
    t_eq = ((q[const, 0].astype(np.float64) + md.q_geo) / es) ** 0.25
    assert np.abs(full[const] - t_eq[:, None]).max() < T_TOL
    t_geo = (md.q_geo / es) ** 0.25
    assert np.abs(full[1::6] - t_geo).max() < T_TOL and np.abs(summ[1::6, :3] - t_geo).max() < T_TOL
    assert ex.shape == (SYN_P, SYN_REC, 2) and np.all(ex[..., 0] == 0.0)
    m_ir = es * r["full"] ** 4
    d_ir = np.abs(ex[..., 1] - m_ir)
    print(f"synthetic: M_ir max err {d_ir.max():.2e} W m^-2")
    assert np.all(d_ir <= 4.0 * es * r["full"] ** 3 * T_TOL + 1e-6 * m_ir)
    assert_bit_equal(ex[..., 1], (np.float32(es) * ((full * full) * (full * full))).astype(np.float32), "M_ir of FULL")


@pytest.fixture(scope="module")
def production(rt):
    """130 crater_dem points through the production schedule: 10 lunations of spin-up with 8 resets, 1 h, then 240 recorded
    epochs."""
    md = MoonRT.thermal_grid()
    assert (md.n_spin, md.n_reset, md.block, md.n_sub) == (7090, 8, 709, 12)
    m = md.n_spin + 240
    lat, lon = points(29, 130)
    ep, fl = epochs(m)
    hz = rt.horizon(lat, lon, n_az=64, n_bis=12)
    st = {}
    flux = rt.surface_temperature(lat, lon, hz, ep, fl, md, mode="flux")
    full = rt.surface_temperature(lat, lon, hz, ep, fl, md, mode="full", stats=st)
    summ = rt.surface_temperature(lat, lon, hz, ep, fl, md, mode="summary", stats=st)
    return dict(md=md, lat=lat, lon=lon, ep=ep, fl=fl, hz=hz, flux=flux, full=full, summ=summ, st=st)


def test_production_schedule_matches_the_model(native_lib, production):
    p = production
    t = time.process_time()
    r = tm.run(p["flux"].astype(np.float64), model=p["md"], record_all=False)
    print(f"\nproduction: model {time.process_time() - t:.1f} s CPU")
    assert (p["flux"] > 0).any(1).mean() > 0.5
    against_model("production schedule, 130 points", p["full"], p["summ"], r, p["st"])


def test_point_counts_are_rows_of_the_130_point_call(native_lib, rt, production):
    """1, 63, 64 and 65 points (one lane, a wave less one, a wave, a wave and one) are the matching rows of the 130-point
    (three-wave) call, bit for bit, in FULL and SUMMARY."""
    p = production
    for a, b in ((0, 1), (0, 63), (0, 64), (0, 65), (65, 130), (129, 130)):
        sl = slice(a, b)
        for mode, want in (("full", p["full"]), ("summary", p["summ"])):
            got = rt.surface_temperature(p["lat"][sl], p["lon"][sl], p["hz"][sl], p["ep"], p["fl"], p["md"], mode=mode)
            assert_bit_equal(got, want[sl], f"{mode}, points {a}:{b}")


def test_python_split_equals_one_call(native_lib, rt, production):
    """MoonRT.surface_temperature split into 3 calls by chunk_bytes, host and device horizons, equals one call bit for bit."""
    p = production
    md, m = p["md"], p["ep"].shape[0]
    buf = DeviceBuffer(p["hz"].nbytes)
    buf.upload(p["hz"])
    for mode, width, want in (("full", m - md.n_spin, p["full"]), ("flux", m, p["flux"])):
        for hz, n_az in ((p["hz"], None), (buf, 64)):
            st = {}
            got = rt.surface_temperature(p["lat"], p["lon"], hz, p["ep"], p["fl"], md, mode=mode, stats=st, n_az=n_az,
                                         chunk_bytes=4 * width * 50)
            assert st["launches"] == 3
            assert_bit_equal(got, want, f"{mode} in 3 calls, {'device' if n_az else 'host'} horizons")
    buf.free()


def test_q_geo_below_the_floor_is_refused_before_launch(native_lib, rt):
    lat, lon, hz = dark_points(3)
    md = MoonRT.thermal_grid(3600.0, 1, 1)
    md.n_spin, md.block, md.n_reset = 4, 2, 1
    ep, fl = epochs(8)
    for q_geo in (0.0, 0.999 * Q_FLOOR):
        md.q_geo = q_geo
        st = {}
        with pytest.raises(MoonRTError, match="geothermal floor"):
            rt.surface_temperature(lat, lon, hz, ep, fl, md, mode="full", stats=st)
        assert st == {}


def test_diverging_step_fails_with_the_range_message(native_lib, rt):
    """2200 W m^-2 onto a column at the 24 K floor, one step per epoch just under Delta_max: radiative equilibrium 449.6 K
    passes the 450 K check (the table's maximum included), so the call reaches the kernel, and the float64 model diverges
    (coefficient sum past 1, Newton caps, NaN).  The kernel's per-epoch range flag turns that into MRTX_E_INVALID with the
    range message, through a host table and through a device table, instead of garbage with MRTX_OK."""
    md = MoonRT.thermal_grid(3600.0, 1, 1)
    md.spacing_s, md.n_sub = 0.9999 * tm.max_step(md), 1
    md.n_spin, md.block, md.n_reset = 24, 12, 2
    m = 84
    q = np.zeros((3, m), np.float32)
    q[:, 30:] = 2200.0
    r = tm.run(q.astype(np.float64), model=md)
    print(f"\n2200 W m^-2 at Delta_max: model caps {r['caps']}, out-of-range epochs {r['out_of_range']}, coef_max "
          f"{r['coef_max']:.3g}, final {r['full'][0, -1]}")
    assert r["out_of_range"] > 0
    lat, lon, hz = dark_points(3)
    ep, _ = epochs(m, md.spacing_s)
    fl = np.zeros(m)
    out = DeviceBuffer(q.nbytes)
    with pytest.raises(MoonRTError, match=re.escape(RANGE_MSG)):
        rt.surface_temperature_scatter(lat, lon, hz, ep, fl, md, mode="full", extra_flux=q, out=out)
    got = out.download(np.float32, (3, m - md.n_spin))
    bad = ~((got >= 20.0) & (got <= 450.0))
    print(f"kernel FULL: {int(bad.sum())} of {got.size} surface values outside [20, 450] K or non-finite; first at "
          f"{np.argwhere(bad)[0] if bad.any() else None}; finite max {np.nanmax(np.where(np.isfinite(got), got, np.nan)):.1f} K")
    buf = DeviceBuffer(q.nbytes)
    buf.upload(q)
    with pytest.raises(MoonRTError, match=re.escape(RANGE_MSG)):
        rt.surface_temperature_scatter(lat, lon, hz, ep, fl, md, mode="summary", extra_flux=buf)
    buf.free()
    out.free()
    # the same table at the default step (300 s, 12 per epoch): the model stays finite and ends each epoch in range
    md2 = MoonRT.thermal_grid(3600.0, 1, 1)
    md2.n_spin, md2.block, md2.n_reset = 24, 12, 2
    ep2, _ = epochs(m)
    r2 = tm.run(q.astype(np.float64), model=md2)
    st = {}
    try:
        full2 = rt.surface_temperature_scatter(lat, lon, hz, ep2, fl, md2, mode="full", extra_flux=q, stats=st)
        print(f"2200 W m^-2 at 300 s: FULL max err {np.abs(full2 - r2['full']).max():.2e} K; model nodes up to "
              f"{r2['t_hi']:.1f} K within an epoch, {r2['out_of_range']} epochs out of range")
    except MoonRTError as e:
        print(f"2200 W m^-2 at 300 s: refused after the kernel ({e}); model out-of-range epochs {r2['out_of_range']}")
