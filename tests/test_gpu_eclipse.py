"""The Earth's occultation of the Sun on the MI355X (DESIGN.md sections 3.18 and 4.20): mrtx_occultation FULL against the
float64 model on the 2025-03-14 eclipse, SUMMARY as the reduction of FULL on designed sequences at every 64-epoch chunk edge
and on the real tables, the idle-epoch skip, mrtx_thermal_occulted against mrtx_thermal_column, mrtx_occultation and the
float64 column, the context state, every refusal, and the sunlight drivers end to end."""
import ctypes as C
from datetime import datetime, timedelta, timezone

import numpy as np
import pytest

import eclipse_model as em
import epoch_patterns as ep
import model_cases as mc
import terrain_cases as tc
import thermal_model as tm
from common import assert_bit_equal
from moonrtx_amd import _lib, sunlight, volatiles
from moonrtx_amd import ephemeris as E
from moonrtx_amd._lib import MrtxStats
from moonrtx_amd.renderer import DeviceBuffer
from moonrtx_amd.scene import named_scene
from test_gpu_illumination import make
from test_gpu_thermal import T_TOL, small_model

pytestmark = pytest.mark.gpu

OBS = E.Observer(52.2, 21.0, 0.0)
UTC = timezone.utc
E_INVALID = -1
LAT, LON, SEED = 23.0, -57.0, 0         # the designed tables' site (tests/test_gpu_epoch_walks.py's)
NAN_FILL = 0x7FC12345


def scene():
    return named_scene("S1", 16, 16)


def tables(times):
    """(sun, far sun, earth) epoch tables of the dates."""
    sun, earth = E.sun_earth_epochs(times, OBS)
    return sun, E.far_sun_epochs(sun, times), earth


def globe(seed, n):
    rng = np.random.default_rng(seed)
    return np.degrees(np.arcsin(rng.uniform(-0.98, 0.98, n))), rng.uniform(-180.0, 180.0, n)


@pytest.fixture(scope="module")
def rt(native_lib):
    ctx = make(scene(), mc.crater_dem(), 0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def march(rt):
    """2025-03-14 from 03:40 UTC every 2 minutes, 200 epochs (three whole chunks and a ragged one), at 48 points over the
    globe: the tables, FULL, SUMMARY and the float64 model."""
    t0 = datetime(2025, 3, 14, 3, 40, tzinfo=UTC)
    times = [t0 + timedelta(minutes=2 * k) for k in range(200)]
    sun, far, earth = tables(times)
    lat, lon = globe(11, 48)
    st = {}
    full = rt.occultation(lat, lon, far, earth, stats=st)
    summ = rt.occultation(lat, lon, far, earth, summary=True, stats=st)
    g, info = em.occult_g(scene(), mc.crater_dem(), lat, lon, far, earth)
    return dict(times=times, sun=sun, far=far, earth=earth, lat=lat, lon=lon, full=full, summ=summ, g=g, info=info, st=st)


def test_full_matches_the_model(march):
    """Every (point, epoch) within em.g_tolerance (derived there: the three angles to 5e-5 deg each, |dg / d angle| <=
    2 / (pi alpha_s), plus float32 ulps); exactly 1 or exactly 0 wherever the model is farther than the angle errors from a
    case boundary on its g = 1 or g = 0 side, which holds for more than 0.99 of the entries whose model value is 1 or 0 (a
    partial entry has no exact value to be sure of; 38 % of this table is partial)."""
    full, g, info = march["full"], march["g"], march["info"]
    assert full.shape == g.shape == (48, 200) and full.dtype == np.float32
    assert np.all((full >= 0.0) & (full <= 1.0))
    err = np.abs(full.astype(np.float64) - g)
    tol = em.g_tolerance(info["a_s"])
    n_part_model, n_zero_model = int(((g > 0) & (g < 1)).sum()), int((g == 0).sum())
    n_part, n_zero = int(((full > 0) & (full < 1)).sum()), int((full == 0).sum())
    one, zero = em.sure(info)
    settled = (g == 1.0) | (g == 0.0)                           # the entries whose model value is a case's constant
    share = float((one | zero).sum() / settled.sum())           # ... and how many of them float32 cannot move across the boundary
    print(f"FULL against the model: max error {err.max():.2e} (tolerance {tol.min():.2e}), partial {n_part} / {n_part_model}, "
          f"zero {n_zero} / {n_zero_model}, sure share {share:.4f}")
    assert np.all(err <= tol), (err.max(), np.argwhere(err > tol)[:4])
    assert min(n_part, n_part_model) >= 200 and min(n_zero, n_zero_model) >= 200
    assert np.all(full[one] == 1.0) and np.all(g[one] == 1.0)
    assert np.all(full[zero] == 0.0) and np.all(g[zero] == 0.0)
    assert share > 0.99


def test_force_wide_gives_the_same_bits(native_lib, march):
    wide = make(scene(), mc.crater_dem(), _lib.F_FORCE_WIDE)
    try:
        for summary, key in ((False, "full"), (True, "summ")):
            got = wide.occultation(march["lat"], march["lon"], march["far"], march["earth"], summary=summary)
            assert_bit_equal(got, march[key], f"F_FORCE_WIDE, summary={summary}")
    finally:
        wide.close()


def check_summary(summ, full, what):
    """SUMMARY against the plain-loop reduction of FULL: the minimum, the two shares (as float32(count / m)), the three runs,
    the first index and the run count exactly, the mean to rtol 1e-6."""
    want = em.summarize(full)
    assert summ.shape == want.shape and summ.dtype == np.float32
    exact = [1, 2, 3, 4, 5, 6, 7]
    bad = np.argwhere(summ[:, exact] != want[:, exact].astype(np.float32))
    assert bad.size == 0, f"{what}: " + "; ".join(
        f"point {p} column {exact[j]}: {summ[p, exact[j]]!r} for {want[p, exact[j]]!r}" for p, j in bad[:4])
    assert np.allclose(summ[:, 0], want[:, 0], rtol=1e-6, atol=0.0), what


def test_summary_of_the_real_tables_is_the_reduction_of_full(march):
    check_summary(march["summ"], march["full"], "2025-03-14")
    summ = march["summ"]
    assert (summ[:, 7] == 1.0).sum() >= 40 and np.all(summ[:, 7] <= 1.0)      # one eclipse, where any
    assert summ[:, 6].max() >= 60.0                                           # more than two hours of totality somewhere


@pytest.mark.parametrize("m", ep.M)
def test_designed_sequences(rt, m):
    """Per call one designed sequence at one site (em.designed_tables): each epoch's body is concentric with the source and
    larger (exactly 0), 90 deg away (exactly 1, unmarked by the host) or five degrees wide with its limb through the
    source's centre (a robust partial).  FULL is the designed value; SUMMARY's counts, runs, first index, run count and
    minimum are the plain loops' over FULL, exactly."""
    s, dem = scene(), mc.crater_dem()
    lat, lon = np.array([LAT]), np.array([LON])
    for name, codes in em.designed_codes(m, SEED):
        src, body = em.designed_tables(s, dem, LAT, LON, codes)
        full = rt.occultation(lat, lon, src, body)
        assert np.all(full[0, codes == em.TOTAL] == 0.0) and np.all(full[0, codes == em.CLEAR] == 1.0), (m, name)
        part = full[0, codes == em.PARTIAL]
        assert np.all((part > 0.45) & (part < 0.55)), (m, name, part[:4])
        summ = rt.occultation(lat, lon, src, body, summary=True)
        check_summary(summ, full, f"m = {m}, {name}")
        truth = em.summarize(em.codes_as_g(codes)[None])
        assert np.array_equal(summ[0, 2:], truth[0, 2:].astype(np.float32)), (m, name, summ, truth)


def test_several_points_and_device_output(rt):
    """Seven designed points in one call (one site seven times and, from the third on, its neighbours): the rows of the
    one-point calls; SUMMARY into a device buffer 64 floats longer than its output leaves the tail alone."""
    s, dem = scene(), mc.crater_dem()
    m = 129
    codes = next(c for name, c in em.designed_codes(m, SEED) if name.startswith("run[60,130):total where"))
    src, body = em.designed_tables(s, dem, LAT, LON, codes)
    lat, lon = LAT + np.array([0, 0, 1e-3, -1e-3, 0, 2e-3, 0]), np.full(7, LON)
    one = [rt.occultation(lat[i:i + 1], lon[i:i + 1], src, body, summary=True) for i in range(7)]
    allp = rt.occultation(lat, lon, src, body, summary=True)
    assert_bit_equal(allp, np.concatenate(one), "seven points in one call")
    buf = DeviceBuffer((56 + 64) * 4)
    try:
        buf.upload(np.full(56 + 64, NAN_FILL, np.uint32))
        pts = np.ascontiguousarray(np.stack([lat, lon], -1))
        rt._check(rt._lib.mrtx_occultation(rt._ctx, pts.ctypes.data, 7, src.ctypes.data, body.ctypes.data, m, 1, buf.ptr, None,
                                           None), "mrtx_occultation")
        back = buf.download(np.uint32, (56 + 64,))
    finally:
        buf.free()
    assert np.array_equal(back[:56], allp.view(np.uint32).ravel())
    assert np.array_equal(back[56:], np.full(64, NAN_FILL, np.uint32))


def test_the_skip_changes_nothing(rt, march):
    """The eclipse tables preceded by a week of hourly epochs in which the host marks nothing: FULL's tail equals the
    eclipse-only call bit for bit, the week is exactly 1, and SUMMARY is the reduction of that FULL."""
    t0 = march["times"][0] - timedelta(hours=168)
    week = [t0 + timedelta(hours=k) for k in range(168)]
    assert E.eclipse_candidates(week, OBS) == []
    _, far_w, earth_w = tables(week)
    far, earth = np.concatenate([far_w, march["far"]]), np.concatenate([earth_w, march["earth"]])
    full = rt.occultation(march["lat"], march["lon"], far, earth)
    assert_bit_equal(full[:, 168:], march["full"], "the eclipse after an idle week")
    assert np.all(full[:, :168] == 1.0)
    summ = rt.occultation(march["lat"], march["lon"], far, earth, summary=True)
    check_summary(summ, full, "idle week + eclipse")
    seen = march["summ"][:, 4] > 0
    assert np.array_equal(summ[seen, 5], march["summ"][seen, 5] + 168.0)


# ---- the thermal column under occultation ----------------------------------------------------------------------------------
MODES = {"full": 0, "summary": 1, "flux": 2, "exitance": 3, "column": 4, "volatile": 5}


def occulted(rt, lat, lon, hz, ep_, fl, md, mode, occ):
    """mrtx_thermal_occulted called directly (host horizons and output), occ = (source, body) tables or (None, None)."""
    n, m = lat.size, ep_.shape[0]
    rec, nn = m - int(md.n_spin), int(md.n_nodes)
    shape = {"full": (n, rec), "summary": (n, 4), "flux": (n, m), "exitance": (n, rec, 2), "column": (n, rec, nn),
             "volatile": (n, nn, 2)}[mode]
    res = np.empty(shape, np.float64 if mode == "volatile" else np.float32)
    pts = np.ascontiguousarray(np.stack([lat, lon], -1))
    sp = volatiles.law(volatiles.H2O) if mode == "volatile" else None
    st = MrtxStats()
    hz = np.ascontiguousarray(hz, np.float32)
    rt._check(rt._lib.mrtx_thermal_occulted(
        rt._ctx, pts.ctypes.data, n, hz.shape[1], None, hz.ctypes.data, ep_.ctypes.data, fl.ctypes.data, m, C.byref(md),
        MODES[mode], None, None, 0, None if sp is None else C.byref(sp), None if occ[0] is None else occ[0].ctypes.data,
        None if occ[1] is None else occ[1].ctypes.data, None, res.ctypes.data, C.byref(st)), "mrtx_thermal_occulted")
    return res, int(st.reserved)


@pytest.fixture(scope="module")
def column(rt):
    """small_model()'s spin-up (one lunation of hourly epochs) placed so that the recorded block is the 24 hours of
    2025-03-14: the eclipse's seven hourly epochs 04:00 .. 10:00 are recorded."""
    md = small_model()
    t_rec = datetime(2025, 3, 14, tzinfo=UTC)
    times = [t_rec + timedelta(hours=k - int(md.n_spin)) for k in range(int(md.n_spin) + 24)]
    sun, far, earth = tables(times)
    fl = E.sun_flux(times)
    rng = np.random.default_rng(5)
    lat, lon = rng.uniform(-50.0, 50.0, 24), rng.uniform(-60.0, 60.0, 24)
    hz = rt.horizon(lat, lon, n_az=64, n_bis=12)
    plain = {mode: rt.thermal_column(lat, lon, hz, sun, fl, md, mode=mode, species=volatiles.H2O if mode == "volatile" else None)
             for mode in MODES}
    g = rt.occultation(lat, lon, far, earth)
    return dict(md=md, times=times, sun=sun, far=far, earth=earth, fl=fl, lat=lat, lon=lon, hz=hz, plain=plain, g=g)


def test_null_tables_are_thermal_column(rt, column):
    c = column
    for mode in MODES:
        got, _ = occulted(rt, c["lat"], c["lon"], c["hz"], c["sun"], c["fl"], c["md"], mode, (None, None))
        assert_bit_equal(got, c["plain"][mode], f"null tables, {mode}")


def test_a_body_90_degrees_off_changes_nothing(rt, column):
    """The Earth's table with the Earth moved 90 deg from the Sun (same distance, same radius): the occulted kernels run,
    every g is 1, and every mode gives mrtx_thermal_column's bits."""
    c = column
    off = c["earth"].copy()
    ray = c["far"][:, 0:3] - c["far"][:, 5:8]
    ray /= np.linalg.norm(ray, axis=1)[:, None]
    side = np.cross(ray, np.array([0.3, -0.5, 0.8]))
    side /= np.linalg.norm(side, axis=1)[:, None]
    dist = np.linalg.norm(c["earth"][:, 0:3] - c["earth"][:, 5:8], axis=1)
    off[:, 0:3] = off[:, 5:8] + dist[:, None] * side
    assert np.all(rt.occultation(c["lat"][:3], c["lon"][:3], c["far"], off) == 1.0)
    for mode in MODES:
        got, _ = occulted(rt, c["lat"], c["lon"], c["hz"], c["sun"], c["fl"], c["md"], mode, (c["far"], off))
        assert_bit_equal(got, c["plain"][mode], f"body 90 deg off, {mode}")
        via = rt.thermal_column(c["lat"], c["lon"], c["hz"], c["sun"], c["fl"], c["md"], mode=mode,
                                species=volatiles.H2O if mode == "volatile" else None, occultation=(c["far"], off))
        assert_bit_equal(via, c["plain"][mode], f"body 90 deg off through MoonRT.thermal_column, {mode}")


def test_flux_is_the_plain_flux_times_g(rt, column):
    """FLUX with the real tables: exactly the plain FLUX where mrtx_occultation gives 1, exactly 0 where it gives 0,
    elsewhere plain FLUX x g within 4e-6 relative + 1e-4 W m^-2 (tests/test_gpu_thermal.py's bound for FLUX)."""
    c = column
    occ = (c["far"], c["earth"])
    flux = rt.thermal_column(c["lat"], c["lon"], c["hz"], c["sun"], c["fl"], c["md"], mode="flux", occultation=occ)
    plain, g = c["plain"]["flux"], c["g"]
    assert flux.shape == plain.shape == g.shape
    one, zero = g == 1.0, g == 0.0
    assert np.array_equal(flux[one].view(np.uint32), plain[one].view(np.uint32))
    assert np.all(flux[zero] == 0.0)
    part = ~one & ~zero
    want = plain[part].astype(np.float64) * g[part].astype(np.float64)
    err = np.abs(flux[part] - want)
    assert np.all(err <= 4e-6 * want + 1e-4), err.max()
    # presence, over the recorded block
    n_spin = int(c["md"].n_spin)
    mu = rt.illumination_series(c["lat"], c["lon"], c["sun"][n_spin:], n_sun=1)[..., 2]
    n_part = int(part[:, n_spin:].sum())
    n_zero_lit = int((zero[:, n_spin:] & (mu > 0.5)).sum())
    print(f"recorded (point, epoch)s: {n_part} with 0 < g < 1, {n_zero_lit} with g == 0 at mu > 0.5")
    assert n_part >= 12 and n_zero_lit >= 6
    assert not part[:, :n_spin].any() and not zero[:, :n_spin].any()            # no eclipse in the spin-up lunation


def test_full_and_summary_match_the_model_fed_that_flux(rt, column):
    c, md = column, column["md"]
    occ = (c["far"], c["earth"])
    st = {}
    args = (c["lat"], c["lon"], c["hz"], c["sun"], c["fl"], md)
    flux = rt.thermal_column(*args, mode="flux", occultation=occ)
    full = rt.thermal_column(*args, mode="full", occultation=occ, stats=st)
    summ = rt.thermal_column(*args, mode="summary", occultation=occ, stats=st)
    r = tm.run(flux.astype(np.float64), md.spacing_s, md.n_sub, md.n_spin, md.block, md.n_reset)
    assert r["caps"] == 0 and st["newton_cap_hits"] == 0
    d = np.abs(full - r["full"])
    assert full.shape == (24, 24) and d.max() < T_TOL, d.max()
    assert np.abs(summ - r["summary"]).max() < T_TOL
    assert_bit_equal(summ[:, 0], full.max(1), "maximum")
    assert_bit_equal(summ[:, 1], full.min(1), "minimum")
    # the cooling: recorded epoch k is k:00 UTC; 04:00 precedes first contact everywhere, 07:00 is total everywhere
    n_spin = int(md.n_spin)
    lit = c["plain"]["flux"][:, n_spin + 7] > 300.0
    fall = full[:, 4] - full[:, 4:9].min(1)
    plain_fall = c["plain"]["full"][:, 4] - c["plain"]["full"][:, 4:9].min(1)
    p = int(np.argmax(np.where(lit, fall, -np.inf)))
    print(f"largest fall of the surface temperature through totality: {fall[p]:.1f} K at point {p} "
          f"({full[p, 4]:.1f} K at 04:00 to {full[p, 4:9].min():.1f} K; without the eclipse {plain_fall[p]:.1f} K); "
          f"against the model {d.max():.2e} K")
    assert np.all(fall[lit] > plain_fall[lit] + 50.0)                      # against the same column without the eclipse
    assert np.array_equal(full[:, :4], c["plain"]["full"][:, :4])           # and nothing before first contact


# ---- state and refusals --------------------------------------------------------------------------------------------------------
def test_leaves_the_context_state_alone(native_lib, march, column):
    s = scene().with_size(48, 32, spp_per_launch=16)
    dem = mc.crater_dem()
    lat, lon = column["lat"][:3], column["lon"][:3]

    def run(with_eclipse):
        ctx = make(s, dem, _lib.F_COUNT_STATS)
        st1 = ctx.render(1)
        v0 = ctx.config()
        if with_eclipse:
            ctx.occultation(lat, lon, march["far"], march["earth"])
            ctx.occultation(lat, lon, march["far"], march["earth"], summary=True)
            ctx.thermal_column(lat, lon, column["hz"][:3], column["sun"], column["fl"], column["md"], mode="summary",
                               occultation=(column["far"], column["earth"]))
        pt = ctx.illumination_at(lat, lon, n_sun=16)
        st2 = ctx.render(1)
        out = ctx.read_linear(), ctx.read_hits(), ctx.samples_done(), st1, st2, pt, v0 == ctx.config()
        ctx.close()
        return out
    a, b = run(False), run(True)
    assert_bit_equal(b[0], a[0], "linear radiance (the accumulation)")
    assert_bit_equal(b[1], a[1], "hit buffer")
    assert_bit_equal(b[5], a[5], "illumination_at: the light and the Moon frame")
    assert b[2] == a[2] == 32 and b[6]
    for k in ("primary_hits", "shadow_rays", "height_samples", "bounce_rays"):
        assert b[4][k] == a[4][k], k


def test_refusals(rt, march, column):
    """Every refusal of section 3.18 returns MRTX_E_INVALID without a launch: the output and the stats block stay as they
    were."""
    lib, ctx = rt._lib, rt._ctx
    m = 70
    far, earth = np.ascontiguousarray(march["far"][60:60 + m]), np.ascontiguousarray(march["earth"][60:60 + m])
    pts = np.array([[10.0, 20.0], [-60.0, 100.0]])
    out = np.full((2, m), np.nan, np.float32)
    dev = DeviceBuffer(2 * m * 4 + 64)
    base = tc.occult_base(pts, far, earth, out)

    def call(**kw):
        rc, st = tc.occult_call(lib, ctx, **dict(base, **kw))
        assert rc == 0 and st.launches == 1
        return rc

    def edit(table, col, value, k=5):
        t = table.copy()
        t[k, col] = value
        return t
    try:
        rc, st = tc.occult_call(lib, None, **base)
        assert rc == E_INVALID and st.launches == tc.LAUNCHES and np.isnan(out).all()
        for text, _, kw in tc.occult_refusals(pts, far, earth, out, scene().radius, dev.ptr):   # the list (tests/terrain_cases.py)
            rc, st = tc.occult_call(lib, ctx, **kw)
            tc.refused(lib, ctx, rc, st, text)
            assert np.isnan(out).all(), "a refused call wrote: " + text
        # the thermal entry: one table without the other, and the tables' own checks
        c = column
        pt3 = np.ascontiguousarray(np.stack([c["lat"][:3], c["lon"][:3]], -1))
        hz = np.ascontiguousarray(c["hz"][:3])
        res = np.full((3, 4), np.nan, np.float32)

        def thermal(occ_s, occ_b):
            return lib.mrtx_thermal_occulted(ctx, pt3.ctypes.data, 3, 64, None, hz.ctypes.data, c["sun"].ctypes.data,
                                             c["fl"].ctypes.data, c["sun"].shape[0], C.byref(c["md"]), 1, None, None, 0, None,
                                             None if occ_s is None else occ_s.ctypes.data,
                                             None if occ_b is None else occ_b.ctypes.data, None, res.ctypes.data, None)
        assert thermal(c["far"], None) == E_INVALID and thermal(None, c["earth"]) == E_INVALID
        assert thermal(c["far"], edit(c["earth"], 3, 0.0)) == E_INVALID
        assert thermal(edit(c["far"], 1, float("nan")), c["earth"]) == E_INVALID
        assert thermal(c["earth"], c["far"]) == E_INVALID
        assert np.isnan(res).all()
        assert call() == 0 and call(mode=1, host=out.ctypes.data) == 0           # and a good call goes through
    finally:
        dev.free()


# ---- sunlight, end to end ------------------------------------------------------------------------------------------------------
def test_lunar_eclipses_end_to_end(rt):
    lat, lon = np.array([0.0, 40.0, -30.0, 10.0, 0.0]), np.array([0.0, 30.0, -50.0, 80.0, 180.0])
    found = sunlight.lunar_eclipses(rt, lat, lon, datetime(2025, 3, 13, tzinfo=UTC), 3.0, step_min=2, observer=OBS)
    assert len(found) == 1
    e = found[0]
    assert e.times[0].date() == datetime(2025, 3, 14).date() and np.all(e.g_min == 0.0)
    lo, hi = datetime(2025, 3, 14, 5, 9, tzinfo=UTC), datetime(2025, 3, 14, 8, 48, tzinfo=UTC)
    for p in range(5):
        assert lo <= e.total_start[p] <= e.total_end[p] <= hi, (p, e.total_start[p], e.total_end[p])
        assert e.penumbral_start[p] < e.total_start[p] and e.total_end[p] < e.penumbral_end[p]
        assert e.totality_min[p] == (e.total_end[p] - e.total_start[p]).total_seconds() / 60.0 + 2.0
    assert np.all((e.totality_min > 60.0) & (e.totality_min < 220.0))
    assert sunlight.lunar_eclipses(rt, lat, lon, datetime(2025, 4, 1, tzinfo=UTC), 29.0, observer=OBS) == []


def test_surface_temperatures_with_eclipses(rt):
    """sunlight.surface_temperatures(eclipses=True) over 2025-03-14 differs from eclipses=False only at points that were
    sunlit during the eclipse: the far side's columns keep their bits."""
    lat = np.array([0.0, 20.0, -35.0, 5.0, -10.0, 30.0])
    lon = np.array([0.0, -30.0, 40.0, 178.0, -160.0, 150.0])
    t0 = datetime(2025, 3, 14, tzinfo=UTC)
    kw = dict(spinup_lunations=1, n_az=32, n_bis=8, observer=OBS)
    a = sunlight.surface_temperatures(rt, lat, lon, t0, 1.0, **kw)
    b = sunlight.surface_temperatures(rt, lat, lon, t0, 1.0, eclipses=True, **kw)
    near = np.array([True, True, True, False, False, False])
    for x, y in zip(a[:4], b[:4]):
        assert np.array_equal(x[~near].view(np.uint32), y[~near].view(np.uint32))
    assert np.all(b.t_min[near] < a.t_min[near] - 50.0), (a.t_min, b.t_min)
    assert np.all(b.t_max[near] <= a.t_max[near])
    with pytest.raises(ValueError):
        sunlight.surface_temperatures(rt, lat, lon, t0, 1.0, eclipses=True, thermal=rt.surface_temperature, **kw)
