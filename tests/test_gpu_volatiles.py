"""Subsurface temperature columns and volatile loss rates on the MI355X (DESIGN.md sections 3.16 and 4.17): the new entry's
old modes against mrtx_thermal_scatter, COLUMN against FULL and the float64 model, VOLATILE against the fold of the device's
own COLUMN and bracketed by the model, bit-exact invariances, the ABI's smallest and largest columns, the refusals and the
context state, a never-lit point, and sunlight.ice_stability against its staged calls."""
from datetime import datetime, timedelta, timezone

import numpy as np
import pytest

import bowl_dem as bd
import model_cases as mc
import thermal_model as tm
import volatile_model as vm
from common import assert_bit_equal
from moonrtx_amd import _lib, sunlight, volatiles
from moonrtx_amd import ephemeris as E
from moonrtx_amd.renderer import DeviceBuffer, MoonRT
from moonrtx_amd.scene import named_scene
from test_gpu_illumination import make
from test_gpu_thermal_domain import custom_model, geometric
from test_volatiles_host import column_refusals

pytestmark = pytest.mark.gpu

OBS = E.Observer(52.2, 21.0, 0.0)
BLOCK = 709                       # one lunation of hourly epochs
T_TOL = 0.05                      # the column against the float64 model (tests/test_gpu_thermal.py)
H2O = volatiles.H2O
B = list(volatiles.law(H2O).b)
COUNTS = (1, 40, 65)              # one point, less than a wave, one lane past a wave


def scene():
    return named_scene("S1", 16, 16)


def points(seed, n):
    rng = np.random.default_rng(seed)
    return np.degrees(np.arcsin(rng.uniform(-0.95, 0.95, n))), rng.uniform(-180.0, 180.0, n)


def epochs(m):
    t0 = datetime(2025, 3, 1, tzinfo=timezone.utc)
    times = [t0 + timedelta(hours=k) for k in range(m)]
    return E.sun_epochs(times, OBS), E.sun_flux(times)


def e_mean_bound(x_max, m_rec):
    """The relative error allowed between VOLATILE's E_mean and the float64 fold of the same COLUMN: log and exp are about an
    ulp each and the roundings of the exponent's terms are amplified by |x|, 8 max|x| units of 2^-53 in all, and a positive
    left fold of m_rec terms adds m_rec - 1 roundings."""
    return (8.0 * x_max + m_rec) * 2.0 ** -53


@pytest.fixture(scope="module")
def case():
    """65 points once per call size: the device's FLUX, FULL, COLUMN and VOLATILE, and the float64 model's columns fed that
    FLUX (one model run, shared)."""
    dem = mc.crater_dem()
    lat, lon = points(7, 65)
    ep, fl = epochs(2 * BLOCK)
    md = MoonRT.thermal_grid(3600.0, 1, 1)
    rt = make(scene(), dem, 0)
    hz = rt.horizon(lat, lon, n_az=64, n_bis=12)
    flux = rt.surface_temperature_scatter(lat, lon, hz, ep, fl, md, mode="flux")
    full = rt.surface_temperature_scatter(lat, lon, hz, ep, fl, md, mode="full")
    col, vol, st = {}, {}, {}
    for n in COUNTS:
        col[n] = rt.thermal_column(lat[:n], lon[:n], hz[:n], ep, fl, md, mode="column", stats=st)
        vol[n] = rt.thermal_column(lat[:n], lon[:n], hz[:n], ep, fl, md, mode="volatile", species=H2O, stats=st)
    rt.close()
    model_col, r = vm.columns(flux.astype(np.float64), md)
    assert r["caps"] == 0 and r["coef_max"] <= 1.0 and r["out_of_range"] == 0
    return dict(dem=dem, lat=lat, lon=lon, ep=ep, fl=fl, md=md, hz=hz, flux=flux, full=full, col=col, vol=vol, st=st,
                model_col=model_col)


def test_old_modes_through_the_new_entry_are_thermal_scatter(native_lib, case):
    """Modes 0-3 of mrtx_thermal_column equal mrtx_thermal_scatter's bit for bit, without an extra-flux table and with one on
    the host and on the device; the Newton-cap counter too."""
    lat, lon, hz, ep, fl, md = (case[k][:40] if k in ("lat", "lon", "hz") else case[k] for k in ("lat", "lon", "hz", "ep", "fl", "md"))
    extra = np.random.default_rng(11).uniform(0.0, 40.0, (40, 2 * BLOCK)).astype(np.float32)
    rt = make(scene(), case["dem"], 0)
    buf = DeviceBuffer(extra.nbytes)
    buf.upload(extra)
    for mode in ("full", "summary", "flux", "exitance"):
        for name, x in (("no table", None), ("host table", extra), ("device table", buf)):
            sa, sb = {}, {}
            a = rt.surface_temperature_scatter(lat, lon, hz, ep, fl, md, mode=mode, extra_flux=x, stats=sa)
            b = rt.thermal_column(lat, lon, hz, ep, fl, md, mode=mode, extra_flux=x, stats=sb)
            assert_bit_equal(b, a, f"{mode}, {name}")
            assert sa["newton_cap_hits"] == sb["newton_cap_hits"] and sa["launches"] == sb["launches"] == 1
    buf.free()
    rt.close()


def test_column_node_0_is_full(native_lib, case):
    for n in COUNTS:
        assert case["col"][n].shape == (n, BLOCK, 22) and case["col"][n].dtype == np.float32
        assert_bit_equal(case["col"][n][:, :, 0], case["full"][:n], f"COLUMN[:, :, 0] against FULL, {n} points")


def test_column_matches_the_model_at_every_node(native_lib, case):
    col = case["col"][65]
    assert np.isfinite(col).all() and case["st"]["newton_cap_hits"] == 0
    d = np.abs(col.astype(np.float64) - case["model_col"])
    per_node = d.max(axis=(0, 1))
    print(f"COLUMN against the model: max {d.max():.2e} K (node {int(per_node.argmax())}), surface {per_node[0]:.2e} K, "
          f"bottom {per_node[-1]:.2e} K; range {col.min():.1f}-{col.max():.1f} K")
    assert d.max() < T_TOL
    assert col.max() > 300.0 and col.min() < 120.0


def test_point_counts_are_rows_of_the_largest_call(native_lib, case):
    """1, 40 and 65 points: the lanes past the last point store nothing and change nothing."""
    for n in COUNTS[:-1]:
        assert_bit_equal(case["col"][n], case["col"][65][:n], f"COLUMN, {n} points")
        assert_bit_equal(case["vol"][n], case["vol"][65][:n], f"VOLATILE, {n} points")


def test_volatile_t_max_is_the_maximum_of_column(native_lib, case):
    for n in COUNTS:
        vol = case["vol"][n]
        assert vol.shape == (n, 22, 2) and vol.dtype == np.float64
        assert np.array_equal(vol[:, :, 1], case["col"][n].max(axis=1).astype(np.float64))


def test_e_mean_is_the_fold_of_column(native_lib, case):
    """E_mean against the float64 fold of exp(x) over the device's own COLUMN in the spec's order, within
    (8 max|x| + m_rec) 2^-53 relative, max|x| from the model: a derived bound (e_mean_bound).  numpy forms x without the
    spec's two fma, two more roundings of terms smaller than max|x|, which the 8 covers."""
    x_max = float(np.abs(vm.ln_rate(case["model_col"], B)).max())
    bound = e_mean_bound(x_max, BLOCK)
    for n in COUNTS:
        want, _ = vm.fold(case["col"][n], B)
        got = case["vol"][n][:, :, 0]
        assert np.all(got > 0.0) and np.isfinite(got).all()
        err = np.abs(got / want - 1.0).max()
        print(f"E_mean against the fold of COLUMN, {n} points: max relative error {err:.2e} (bound {bound:.2e}, "
              f"max|x| {x_max:.1f})")
        assert err <= bound


def test_e_mean_is_bracketed_by_the_model(native_lib, case):
    """E is monotone in T and COLUMN lies within T_TOL of the model, so per node
    mean E(T_model - 0.05) <= E_mean <= mean E(T_model + 0.05), the model run on its own."""
    lo = vm.rate(case["model_col"] - T_TOL, B).mean(axis=1)
    hi = vm.rate(case["model_col"] + T_TOL, B).mean(axis=1)
    got = case["vol"][65][:, :, 0]
    assert np.all(lo <= got) and np.all(got <= hi), (np.max(lo / got), np.min(hi / got))
    # the surface loses far more than the deep nodes where the Sun reaches, and a warm point more than 1 mm / Gyr
    assert (got[:, 0] / H2O.rho_solid > volatiles.RATE_MAX).any()


def test_invariances_and_horizon_sources(native_lib, case):
    """A point's COLUMN and VOLATILE do not depend on the other points of the call, their order or number; host and device
    horizons, the production build, F_FORCE_WIDE and F_COUNT_STATS give the same bits."""
    lat, lon, hz, ep, fl, md = (case[k] for k in ("lat", "lon", "hz", "ep", "fl", "md"))
    perm = np.random.default_rng(3).permutation(65)[:17]
    for flags in (0, _lib.F_FORCE_WIDE, _lib.F_COUNT_STATS):
        rt = make(scene(), case["dem"], flags)
        assert_bit_equal(rt.thermal_column(lat[perm], lon[perm], hz[perm], ep, fl, md, mode="column"), case["col"][65][perm],
                         f"COLUMN, permuted subset, flags {flags}")
        assert_bit_equal(rt.thermal_column(lat[perm], lon[perm], hz[perm], ep, fl, md, mode="volatile", species=H2O),
                         case["vol"][65][perm], f"VOLATILE, permuted subset, flags {flags}")
        buf = DeviceBuffer(hz.nbytes)
        buf.upload(hz)
        assert_bit_equal(rt.thermal_column(lat, lon, buf, ep, fl, md, mode="volatile", species=H2O, n_az=64), case["vol"][65],
                         f"VOLATILE, device horizons, flags {flags}")
        assert_bit_equal(rt.thermal_column(lat[:40], lon[:40], buf, ep, fl, md, mode="column", n_az=64), case["col"][40],
                         f"COLUMN, device horizons, flags {flags}")
        out = DeviceBuffer(65 * 22 * 16)
        assert rt.thermal_column(lat, lon, buf, ep, fl, md, mode="volatile", species=H2O, n_az=64, out=out) is out
        assert_bit_equal(out.download(np.float64, (65, 22, 2)), case["vol"][65], f"VOLATILE into a device buffer, flags {flags}")
        out.free()
        buf.free()
        rt.close()


@pytest.mark.parametrize("which", ["n3", "n32"])
def test_smallest_and_largest_columns(native_lib, which):
    """n_nodes 3 and 32, the ABI's limits, over 48 recorded epochs after 100 of spin-up: COLUMN against FULL and the model,
    VOLATILE against COLUMN, at 65 points."""
    md = (custom_model([0.02, 0.1], 1, 3600.0, 100, 100, 1) if which == "n3" else
          custom_model(geometric(32, 0.004, 1.095), 30, 3600.0, 100, 50, 2))
    n = int(md.n_nodes)
    lat, lon = points(21, 65)
    ep, fl = epochs(148)
    rt = make(scene(), mc.crater_dem(), 0)
    hz = rt.horizon(lat, lon, n_az=64, n_bis=12)
    flux = rt.thermal_column(lat, lon, hz, ep, fl, md, mode="flux")
    full = rt.thermal_column(lat, lon, hz, ep, fl, md, mode="full")
    col = rt.thermal_column(lat, lon, hz, ep, fl, md, mode="column")
    vol = rt.thermal_column(lat, lon, hz, ep, fl, md, mode="volatile", species=H2O)
    rt.close()
    assert col.shape == (65, 48, n) and vol.shape == (65, n, 2)
    assert_bit_equal(col[:, :, 0], full, "COLUMN[:, :, 0] against FULL")
    model_col, r = vm.columns(flux.astype(np.float64), md)
    assert r["caps"] == 0 and r["coef_max"] <= 1.0 and r["out_of_range"] == 0
    d = np.abs(col.astype(np.float64) - model_col).max()
    want, t_max = vm.fold(col, B)
    bound = e_mean_bound(float(np.abs(vm.ln_rate(model_col, B)).max()), 48)
    err = np.abs(vol[:, :, 0] / want - 1.0).max()
    print(f"{which}: COLUMN against the model max {d:.2e} K; E_mean against the fold {err:.2e} (bound {bound:.2e})")
    assert d < T_TOL
    assert np.array_equal(vol[:, :, 1], t_max)
    assert err <= bound


def test_never_lit_point_sits_on_the_steady_geotherm(native_lib):
    """A horizon of 90 deg all round: every node's T_max within 0.05 K of the model's steady geotherm through the default
    spin-up and a lunation, a loss rate far below the bar at every node, and depth 0."""
    rt = make(scene(), mc.crater_dem(), 0)
    lat, lon = np.array([-89.0, 10.0]), np.array([30.0, -40.0])
    md = MoonRT.thermal_grid()
    ep, fl = epochs(md.n_spin + BLOCK)
    hz = np.full((2, 16), 90.0, np.float32)
    vol = rt.thermal_column(lat, lon, hz, ep, fl, md, mode="volatile", species=H2O)
    rt.close()
    geo = vm.steady_geotherm(md)
    assert geo[0] == pytest.approx(24.04, abs=0.005) and np.all(np.diff(geo) > 0.0)
    assert np.abs(vol[:, :, 1] - geo[None, :]).max() < 0.05, vol[:, :, 1]
    depth = volatiles.stability_depth(vol[:, :, 0], MoonRT.thermal_depths(md), H2O)
    assert np.all(depth == 0.0) and np.all(vol[:, :, 0] / H2O.rho_solid < 1e-30 * volatiles.RATE_MAX)


def test_leaves_the_context_state_alone_and_refuses(native_lib):
    s = scene().with_size(48, 32, spp_per_launch=16)
    dem = mc.crater_dem()
    lat, lon = np.array([10.0, -20.0, 33.0]), np.array([20.0, 95.0, -80.0])
    ep, fl = epochs(BLOCK + 48)

    def run(with_columns):
        rt = make(s, dem, _lib.F_COUNT_STATS)
        st1 = rt.render(1)
        v0 = rt.config()
        if with_columns:
            hz = rt.horizon(lat, lon, n_az=32, n_bis=8)
            md = MoonRT.thermal_grid(3600.0, 1, 1)
            rt.thermal_column(lat, lon, hz, ep, fl, md, mode="column")
            rt.thermal_column(lat, lon, hz, ep, fl, md, mode="volatile", species=H2O)
        pt = rt.illumination_at(lat, lon, n_sun=16)
        st2 = rt.render(1)
        out = rt.read_linear(), rt.read_hits(), rt.samples_done(), st1, st2, pt, v0 == rt.config()
        rt.close()
        return out
    a, b = run(False), run(True)
    assert_bit_equal(b[0], a[0], "linear radiance")
    assert_bit_equal(b[1], a[1], "hit buffer")
    assert_bit_equal(b[5], a[5], "illumination_at after the column calls (the light and the Moon frame)")
    assert b[2] == a[2] == 32 and b[6]
    for k in ("primary_hits", "shadow_rays", "height_samples", "bounce_rays"):
        assert b[4][k] == a[4][k], k
    rt = make(s, dem, 0)
    column_refusals(native_lib, rt._ctx, 0)
    with pytest.raises(ValueError):
        rt.thermal_column(lat, lon, np.zeros((3, 16), np.float32), ep, fl, mode="volatile")
    with pytest.raises(ValueError):
        rt.thermal_column(lat, lon, np.zeros((3, 16), np.float32), ep, fl, mode="column", species=H2O)
    rt.close()


@pytest.mark.parametrize("which,scatter", [("crater", 0), ("crater", 16), ("bowl", 16)])
def test_ice_stability_end_to_end(native_lib, which, scatter):
    """sunlight.ice_stability (9 points, one lunation of spin-up, 2 days) equals its staged calls bit for bit -- the horizons,
    with scatter the view hits, the hits' EXITANCE and the gather, then thermal_column in VOLATILE -- its depth is
    stability_depth of its own rates, and it makes the launches those calls make.  crater_dem's craters are too shallow for a
    point to see terrain; in the bowl (d/D = 0.2, 6 deg in radius) the points do, and the extra flux reaches VOLATILE."""
    if which == "bowl":
        dem = bd.bowl_dem(720, 1440, 0.0, 0.0, 6.0, 0.2)
        lat, lon = (np.asarray(x, np.float64) for x in bd.bowl_points(0.0, 0.0, 6.0, [0.3, 0.6], n_az=4))
    else:
        dem = mc.crater_dem()
        lat, lon = points(5, 9)
    assert lat.size == 9
    rt = make(scene(), dem, 0)
    t0 = datetime(2025, 3, 1, tzinfo=timezone.utc)
    r = sunlight.ice_stability(rt, lat, lon, t0, 2.0, spinup_lunations=1, n_az=32, n_bis=8, observer=OBS, scatter=scatter)
    md = MoonRT.thermal_grid(3600.0, 1, 1)
    n_spin = int(md.n_spin)
    st = {}
    hz = rt.horizon(lat, lon, n_az=32, n_bis=8, stats=st)
    times = [t0 + timedelta(hours=k - 2 * n_spin) for k in range(2 * n_spin + 48)]
    ep_h, fl_h = E.sun_epochs(times, OBS), E.sun_flux(times)
    ep_t, fl_t = ep_h[n_spin:], fl_h[n_spin:]
    q, n_h = None, 0
    if scatter:
        hits, _ = rt.view_hits(lat, lon, k=scatter, stats=st)
        index, h_lat, h_lon = sunlight.compact_hits(hits)
        n_h = h_lat.size
        if n_h:
            hz_h = rt.horizon(h_lat, h_lon, n_az=32, n_bis=8, stats=st)
            ex = rt.surface_temperature_scatter(h_lat, h_lon, hz_h, ep_h, fl_h, model=md, mode="exitance", stats=st)
            from moonrtx_amd import thermal
            q = rt.scatter_flux(index, ex, thermal.albedo_hemispherical(), thermal.EMISSIVITY, stats=st)
    vol = rt.thermal_column(lat, lon, hz, ep_t, fl_t, model=md, mode="volatile", extra_flux=q, species=H2O, stats=st)
    rt.close()
    assert_bit_equal(r.e_mean, vol[:, :, 0], "e_mean against the staged calls")
    assert_bit_equal(r.t_max_nodes, vol[:, :, 1], "t_max_nodes against the staged calls")
    assert np.array_equal(r.z, MoonRT.thermal_depths(md)) and r.e_mean.shape == (9, 22)
    assert np.array_equal(r.depth_m, volatiles.stability_depth(r.e_mean, r.z, H2O))
    assert np.array_equal(r.loss_rate_surface, r.e_mean[:, 0] / H2O.rho_solid)
    assert len(r.times) == 48 and r.times[0] == t0
    # one chunk, one group: horizons and columns, and with scatter the view hits and, if any ray hit, three more calls
    want = 2 if not scatter else 3 + (3 if n_h else 0)
    assert (n_h > 0) == (which == "bowl")
    print(f"{which}, scatter = {scatter}: {n_h} hits, {r.stats['launches']} launches, depths {r.depth_m.tolist()}")
    assert r.stats["launches"] == st["launches"] == want
    assert np.all((r.depth_m >= 0.0) & ((r.depth_m <= r.z[-1]) | np.isinf(r.depth_m)))
