"""The site power budget on the MI355X (DESIGN.md sections 3.17 and 4.19): power_budget_kernel driven with designed integer
series (tests/power_model.py) through forced visibility (tests/epoch_patterns.py), bitwise in all eight columns; SUMMARY as
the reduction of FULL on real relief; FULL against mrtx_horizon_sun's fractions and the float64 panel factors; and the
call's properties.  Both addressing builds (flags 0 and F_FORCE_WIDE) run the designed cases; no march runs in them."""
import ctypes as C
from datetime import datetime, timedelta, timezone

import numpy as np
import pytest

import epoch_patterns as ep
import horizon_model as hm
import model_cases as mc
import power_model as pm
from common import assert_bit_equal
from moonrtx_amd import _lib
from moonrtx_amd import ephemeris as E
from moonrtx_amd._lib import MrtxPowerModel, MrtxStats
from moonrtx_amd.renderer import DeviceBuffer, MoonRT
from moonrtx_amd.scene import named_scene
from test_gpu_illumination import make

pytestmark = pytest.mark.gpu

LAT, LON, N_AZ, SEED = 23.0, -57.0, 1024, 0
FILL = 0x7FC12345               # the guard band's word
OBS = E.Observer(52.2, 21.0, 0.0)


def scene():
    return named_scene("S1", 16, 16)


@pytest.fixture(scope="module", params=[0, _lib.F_FORCE_WIDE], ids=["narrow", "wide"])
def rt(request, native_lib):
    ctx = make(scene(), mc.crater_dem(), request.param)
    yield ctx
    ctx.close()


def site(P):
    return np.full(P, LAT), np.full(P, LON)


def same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} entries differ, e.g. " + "; ".join(
            f"row {p} column {j}: {got[p, j]} for {want[p, j]}" for p, j in bad[:4]))


# ---- designed integer series ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", ep.M)
def test_designed_series(rt, m):
    """Every sequence of power_model.sequences(m) under every battery of power_model.CONFIGS: visibility forced to 1, a
    tracking panel and one count per watt make e_k the designed integer, and all eight SUMMARY columns equal
    power_model.budget's bit for bit -- from host and from device horizons, in calls of 1 and of 7 points.  FULL returns
    max(e_k, 0)."""
    s, dem = scene(), mc.crater_dem()
    names, e = pm.stack(pm.sequences(m, SEED))
    lat, lon = site(7)
    ones = np.ones((7, m), bool)
    hz = ep.horizon_rows(ones, ones, N_AZ)
    lights = ep.lights(s, dem, LAT, LON, ep.sectors_of(m, N_AZ)[0], N_AZ)
    buf = DeviceBuffer(hz.nbytes)
    try:
        buf.upload(hz)
        for name, row in zip(names, e):
            gen, load = pm.split(row)
            kw = dict(panel="track", cpw_log2=0)
            full = rt.power_budget(lat, lon, hz, lights, gen, load, mode="full", **kw)
            same(full, np.tile(np.maximum(row, 0).astype(np.int32), (7, 1)), f"m = {m}, {name}: FULL")
            for cap, ini in pm.CONFIGS:
                want = np.array([pm.budget(row, cap, ini)], np.int64)
                what = f"m = {m}, {name}, capacity {cap}, initial {ini}"
                for n in (1, 7):
                    host = rt.power_budget(lat[:n], lon[:n], hz[:n], lights, gen, load, capacity=cap, initial=ini, **kw)
                    same(host, np.tile(want, (n, 1)), f"{what}: {n} point(s), host horizons")
                    dev = rt.power_budget(lat[:n], lon[:n], buf, lights, gen, load, capacity=cap, initial=ini, n_az=N_AZ, **kw)
                    same(dev, np.tile(want, (n, 1)), f"{what}: {n} point(s), device horizons")
    finally:
        buf.free()


@pytest.mark.parametrize("m", ep.M)
def test_structured_visibility(rt, m):
    """epoch_patterns.structured(m) as per-point visibility with 7 W generated and 3 W drawn on every date: FULL is 7 x the
    designed bit (f's bits reach G), SUMMARY the budget of 7 bit - 3 per point, all points in one call and in calls of 7."""
    s, dem = scene(), mc.crater_dem()
    seqs = ep.structured(m, SEED)
    bits = np.stack([q[1] for q in seqs])
    P = bits.shape[0]
    lat, lon = site(P)
    hz = ep.horizon_rows(bits, np.ones_like(bits), N_AZ)
    lights = ep.lights(s, dem, LAT, LON, ep.sectors_of(m, N_AZ)[0], N_AZ)
    g = 7 * bits.astype(np.int64)
    kw = dict(panel="track", cpw_log2=0, capacity=20, initial=9)
    want = pm.budgets(g - 3, 20, 9, g_rows=g)
    full = rt.power_budget(lat, lon, hz, lights, 7.0, 3.0, mode="full", **kw)
    same(full, g.astype(np.int32), f"m = {m}: FULL")
    same(rt.power_budget(lat, lon, hz, lights, 7.0, 3.0, **kw), want, f"m = {m}: SUMMARY")
    parts = range(0, P, 7)
    same(np.concatenate([rt.power_budget(lat[i:i + 7], lon[i:i + 7], hz[i:i + 7], lights, 7.0, 3.0, **kw) for i in parts]), want,
         f"m = {m}: SUMMARY in 7s")
    buf = DeviceBuffer(hz.nbytes)
    try:
        buf.upload(hz)
        same(rt.power_budget(lat, lon, buf, lights, 7.0, 3.0, n_az=N_AZ, **kw), want, f"m = {m}: SUMMARY from device horizons")
        same(rt.power_budget(lat, lon, buf, lights, 7.0, 3.0, n_az=N_AZ, mode="full", **kw), full, f"m = {m}: FULL, device horizons")
    finally:
        buf.free()


def test_writes_stay_inside_the_output(rt):
    """FULL (n = 3, m = 65) and SUMMARY into a device buffer 256 words longer than the output, filled with a known word: the
    tail comes back unchanged and the head equals the host-output call."""
    s, dem = scene(), mc.crater_dem()
    m, n, tail = 65, 3, 256
    bits = np.stack([q[1] for q in ep.structured(m, SEED) if q[0] in ("random0.5", "one1@64", "run[60,130)")])
    assert bits.shape == (n, m)
    lat, lon = site(n)
    hz = ep.horizon_rows(bits, np.ones_like(bits), N_AZ)
    lights = ep.lights(s, dem, LAT, LON, ep.sectors_of(m, N_AZ)[0], N_AZ)
    pts = np.ascontiguousarray(np.stack([lat, lon], -1))
    gen, load = np.full(m, 7.0), np.full(m, 3.0)
    md = MrtxPowerModel()
    md.panel, md.cpw_log2, md.capacity, md.initial = 0, 0, 20, 9
    md.normal_enu[:] = (0.0, 0.0, 1.0)
    for what, mode in (("FULL", 0), ("SUMMARY", 1)):
        host = rt.power_budget(lat, lon, hz, lights, gen, load, cpw_log2=0, capacity=20, initial=9, mode=what.lower())
        words = host.view(np.uint32).ravel()
        buf = DeviceBuffer((words.size + tail) * 4)
        try:
            buf.upload(np.full(words.size + tail, FILL, np.uint32))
            rt._check(rt._lib.mrtx_power_budget(rt._ctx, pts.ctypes.data, n, N_AZ, None, hz.ctypes.data, lights.ctypes.data,
                                                gen.ctypes.data, load.ctypes.data, m, C.byref(md), mode, buf.ptr, None,
                                                C.byref(MrtxStats())), what)
            back = buf.download(np.uint32, (words.size + tail,))
        finally:
            buf.free()
        assert np.array_equal(back[:words.size], words), f"{what}: device output differs from host output"
        assert np.array_equal(back[words.size:], np.full(tail, FILL, np.uint32)), f"{what}: wrote past its {words.size} words"


# ---- real relief ---------------------------------------------------------------------------------------------------------------
PANELS = (("track", None), ("fixed", (0.3, -0.5, 0.4)), ("azimuth", None))
RELIEF_N_AZ = 64


def f_tolerance(info, n_az):
    """tests/test_gpu_horizon.py's bound on |f - model| per (point, epoch), recomputed from horizon_model's info: 5e-5 deg on
    the Sun's elevation and azimuth, the azimuth error through the horizon's slope plus an ulp of h, and f's slope in
    r = (h - e_s) / alpha, which near r = +-1 goes as |dr|^1.5."""
    d_ang = 5e-5
    d_h = np.abs(info["h1"] - info["h0"]) * (n_az / 360.0) * d_ang + 1e-5
    r = (info["h"] - info["e_s"]) / info["alpha"]
    d_r = (d_ang + d_h) / info["alpha"] + np.abs(r) * 1e-6
    return (2 / np.pi) * (np.sqrt(np.maximum(0.0, 1.0 - r * r)) + np.sqrt(2 * d_r)) * d_r + 2e-6


@pytest.fixture(scope="module")
def relief(native_lib):
    """The crater DEM, 24 points (polar ones, where the Sun grazes the horizon, and mid-latitudes), a lunation at 4-hour
    steps, the kernel's own horizons and fractions, and FULL and SUMMARY of the three panels -- computed once."""
    s, dem = scene(), mc.crater_dem()
    rng = np.random.default_rng(51)
    lat = np.concatenate([rng.uniform(-89.0, -80.0, 12), rng.uniform(80.0, 89.0, 6), rng.uniform(-50.0, 50.0, 6)])
    lon = rng.uniform(-180.0, 180.0, lat.size)
    t0 = datetime(2025, 3, 1, tzinfo=timezone.utc)
    times = [t0 + timedelta(hours=4 * k) for k in range(int(29.6 * 24 / 4))]
    eps = E.sun_epochs(times, OBS)
    m = len(times)
    gen = E.sun_flux(times) * (2.0 * 0.29) + 0.37 * np.sin(np.arange(m))      # about 790 W, no round numbers
    load = 150.3 + 20.0 * (np.arange(m) % 5 == 0)
    cpw = MoonRT.power_scale(gen, load)
    cap = 40 * int(pm.quantise([150.3], cpw)[0])
    ctx = make(s, dem, 0)
    hz = ctx.horizon(lat, lon, n_az=RELIEF_N_AZ, n_bis=12)
    f = ctx.horizon_sun(lat, lon, hz, eps)
    runs = {}
    for panel, normal in PANELS:
        kw = dict(panel=panel, normal_enu=normal, capacity=cap, initial=cap // 3)
        runs[panel] = (ctx.power_budget(lat, lon, hz, eps, gen, load, mode="full", **kw),
                       ctx.power_budget(lat, lon, hz, eps, gen, load, **kw))
    yield dict(s=s, dem=dem, lat=lat, lon=lon, eps=eps, m=m, gen=gen, load=load, cpw=cpw, cap=cap, rt=ctx, hz=hz, f=f, runs=runs)
    ctx.close()


def test_summary_is_the_reduction_of_full(relief):
    """Each SUMMARY row equals power_model.budget of that row of FULL's G minus the host-quantised L, bit for bit, for the three
    panels; partial discs are present, and the battery runs empty somewhere."""
    r = relief
    assert r["m"] == 177 and r["cpw"] == 18
    partial = (r["f"] > 0) & (r["f"] < 1)
    print(f"{partial.sum()} partial discs of {partial.size}")
    assert partial.sum() >= 20
    L = pm.quantise(r["load"], r["cpw"])
    for panel, _ in PANELS:
        full, summ = r["runs"][panel]
        assert full.dtype == np.int32 and full.shape == (24, r["m"]) and full.min() >= 0
        e = full.astype(np.int64) - L[None, :]
        same(summ, pm.budgets(e, r["cap"], r["cap"] // 3, g_rows=full), f"{panel}: SUMMARY against the reduction of FULL")
        assert (summ[:, 6] > 0).any() and (summ[:, 2] > 0).any() and (summ[:, 5] >= 0).all() and (summ[:, 5] <= r["cap"] // 3).all()


def test_fractional_loads_round_to_even_on_the_host(relief):
    """The host's L_k = (int32)rintf((float)load_w[k] * 2^cpw_log2) on scaled loads with fractional bits: milliwatt loads
    beside the relief's 790 W of generation (1e-3 W is 262.144 counts at 2^18 counts per watt), and exact halves of a count,
    which must go to the even neighbour.  G does not depend on the load, so SUMMARY must be the budget of FULL's G minus
    power_model.quantise's counts, and [1] = sum G - sum L, bit for bit."""
    r = relief
    k = np.arange(r["m"])
    load = 1e-3 * (1.0 + 0.37 * (k % 11)) + 1e-5 * k
    load[::3] = (2 * (k[::3] % 9) + 1) / 2.0 * 2.0 ** -r["cpw"]            # 0.5, 3.5, 6.5 counts, exact in float32
    scaled = load.astype(np.float32).astype(np.float64) * 2.0 ** r["cpw"]
    assert (scaled[::3] % 1.0 == 0.5).all() and (np.abs(scaled % 1.0 - 0.5) > 1e-3)[k % 3 != 0].all() and (scaled % 1.0 != 0).all()
    L = pm.quantise(load, r["cpw"])
    assert (L[::3] % 2 == 0).all() and L[:7:3].tolist() == [0, 4, 6]
    full = r["runs"]["track"][0]
    cap = 1 << 16
    got = r["rt"].power_budget(r["lat"], r["lon"], r["hz"], r["eps"], r["gen"], load, cpw_log2=r["cpw"], capacity=cap, initial=7)
    assert (got[:, 1] == full.astype(np.int64).sum(1) - int(L.sum())).all()
    same(got, pm.budgets(full.astype(np.int64) - L[None, :], cap, 7, g_rows=full), "SUMMARY with fractional loads")


def test_full_against_its_inputs(relief):
    """TRACK: G_k is rint(float32(gen_w[k]) * f_k * 2^cpw_log2) formed in numpy float32 from mrtx_horizon_sun FULL's f, bit
    for bit.  FIXED and AZIMUTH: |G_k - model| <= 1 + gen_w[k] 2^cpw_log2 (tol_f + 32 * 2^-24) against the float64 model
    (horizon_model.sun_fraction on the kernel's horizons times power_model.panel_factor): tol_f is the project's bound on f,
    32 * 2^-24 twice the roundings of c's chain on values of at most 1, and 1 the rounding to a count."""
    r = relief
    scale = np.float32(2.0 ** r["cpw"])
    g32 = r["gen"].astype(np.float32)
    want = np.rint(((g32[None, :] * r["f"]) * np.float32(1.0)) * scale).astype(np.int32)
    same(r["runs"]["track"][0], want, "TRACK: FULL against float32(gen) * f")
    fm, info = hm.sun_fraction(r["s"], r["dem"], r["lat"], r["lon"], r["hz"], r["eps"])
    tol_f = f_tolerance(info, RELIEF_N_AZ)
    worst = 0.0
    for panel, normal in PANELS:
        c = pm.panel_factor(r["s"], r["dem"], r["lat"], r["lon"], r["eps"], pm.PANELS_BY_NAME[panel], normal)
        model = r["gen"][None, :] * fm * c * 2.0 ** r["cpw"]
        bound = 1.0 + r["gen"][None, :] * 2.0 ** r["cpw"] * (tol_f + 32 * 2.0 ** -24)
        err = np.abs(r["runs"][panel][0].astype(np.float64) - model)
        ratio = err / bound
        at = np.unravel_index(np.argmax(ratio), ratio.shape)
        print(f"{panel}: max |G - model| {err.max():.1f} counts, worst error / bound {ratio.max():.3f} at {at}; "
              f"{int(((c > 0) & (c < 1) & (fm > 0)).sum())} entries with 0 < c < 1 and f > 0")
        worst = max(worst, float(ratio.max()))
        assert ratio.max() <= 1.0, (panel, float(ratio.max()), at)
        if panel != "track":
            assert ((c > 0) & (c < 1) & (fm > 0)).sum() >= 100
    print(f"worst error / bound over the panels {worst:.3f}")


def test_point_order_batching_and_a_point_alone(relief):
    r = relief
    rt, lat, lon, hz = r["rt"], r["lat"], r["lon"], r["hz"]
    kw = dict(panel="fixed", normal_enu=(0.3, -0.5, 0.4), capacity=r["cap"], initial=r["cap"] // 3)
    full, summ = r["runs"]["fixed"]
    perm = np.random.default_rng(3).permutation(lat.size)
    same(rt.power_budget(lat[perm], lon[perm], hz[perm], r["eps"], r["gen"], r["load"], **kw), summ[perm], "permuted points")
    same(rt.power_budget(lat[perm], lon[perm], hz[perm], r["eps"], r["gen"], r["load"], mode="full", **kw), full[perm], "permuted FULL")
    st = {}
    same(rt.power_budget(lat, lon, hz, r["eps"], r["gen"], r["load"], stats=st, chunk_bytes=5 * (RELIEF_N_AZ + 16) * 4, **kw), summ,
         "SUMMARY in calls of 5")
    assert st["launches"] == 5
    st = {}
    same(rt.power_budget(lat, lon, hz, r["eps"], r["gen"], r["load"], mode="full", stats=st, chunk_bytes=7 * r["m"] * 4, **kw), full,
         "FULL in calls of 7")
    assert st["launches"] == 4
    for p in (0, 13, 23):
        same(rt.power_budget(lat[p], lon[p], hz[p:p + 1], r["eps"], r["gen"], r["load"], **kw), summ[p:p + 1], f"point {p} alone")


def test_ground_horizons_and_a_mast_of_height_zero(relief):
    r = relief
    rt = r["rt"]
    hz0 = rt.horizon(r["lat"], r["lon"], n_az=RELIEF_N_AZ, n_bis=12, height_m=0.0)
    assert_bit_equal(hz0, r["hz"], "horizon(height_m=0) against the ground call")
    kw = dict(panel="azimuth", capacity=r["cap"], initial=r["cap"] // 3)
    same(rt.power_budget(r["lat"], r["lon"], hz0, r["eps"], r["gen"], r["load"], **kw), r["runs"]["azimuth"][1], "SUMMARY")
    same(rt.power_budget(r["lat"], r["lon"], hz0, r["eps"], r["gen"], r["load"], mode="full", **kw), r["runs"]["azimuth"][0], "FULL")


def test_the_drawdown_is_the_battery_that_never_empties(relief):
    """capacity = D, starting full: the load is always met and the battery just touches 0, per point of the relief case."""
    r = relief
    summ = r["runs"]["track"][1]
    for p in range(r["lat"].size):
        D = int(summ[p, 2])
        got = r["rt"].power_budget(r["lat"][p], r["lon"][p], r["hz"][p:p + 1], r["eps"], r["gen"], r["load"], capacity=D)
        assert got[0, 2] == D and got[0, 6] == 0 and got[0, 7] == 0 and got[0, 5] == 0, (p, got[0].tolist())
        assert np.array_equal(got[0, :5], summ[p, :5])          # the battery does not enter the first five columns


def test_a_panel_facing_down_generates_nothing(relief):
    """A FIXED panel with normal -U: c = max(0, -xu), which is 0 whenever the Sun's centre is above the local horizontal.  On
    the relief's own horizons that is not every lit epoch -- they dip below 0 deg where the ground falls away, and a Sun seen
    from above lights the underside -- so the horizons are raised to at least 1 deg here: then f > 0 needs the centre above
    1 deg - alpha > 0, xu > 0, and G = 0 in every entry, exactly.  On the horizons as they are, G != 0 only where the float64
    model has the Sun's centre below the horizontal (xu < sin 5e-5 deg, the project's bound on the Sun's elevation in
    float32), and there the disc is partly up (f > 0): the deviation from "0 everywhere" is that set and nothing else."""
    r = relief
    hz = np.maximum(r["hz"], np.float32(1.0))
    kw = dict(cpw_log2=r["cpw"])
    full = r["rt"].power_budget(r["lat"], r["lon"], hz, r["eps"], r["gen"], r["load"], panel="fixed", normal_enu=(0, 0, -1),
                                mode="full", **kw)
    lit = r["rt"].power_budget(r["lat"], r["lon"], hz, r["eps"], r["gen"], r["load"], mode="full", **kw)
    print(f"{int((full != 0).sum())} entries with G != 0 facing down; {int((lit > 0).sum())} of {lit.size} lit for a tracking panel")
    assert (lit > 0).sum() >= 300
    assert (full == 0).all()
    summ = r["rt"].power_budget(r["lat"], r["lon"], hz, r["eps"], r["gen"], r["load"], panel="fixed", normal_enu=(0, 0, -1), **kw)
    L = pm.quantise(r["load"], r["cpw"])
    assert (summ[:, 0] == 0).all() and (summ[:, 1] == -int(L.sum())).all() and (summ[:, 2] == int(L.sum())).all()
    assert (summ[:, 3] == 0).all() and (summ[:, 4] == r["m"] - 1).all() and (summ[:, 6] == r["m"]).all()
    real = r["rt"].power_budget(r["lat"], r["lon"], r["hz"], r["eps"], r["gen"], r["load"], panel="fixed", normal_enu=(0, 0, -1),
                                mode="full", **kw)
    xu = pm.sun_direction(r["s"], r["dem"], r["lat"], r["lon"], r["eps"])[2]
    print(f"{int((real != 0).sum())} entries with G != 0 facing down on the horizons as they are; {int((xu < 0).sum())} with xu < 0, "
          f"{int(((xu < 0) & (r['f'] > 0)).sum())} of them with f > 0; lowest horizon {float(r['hz'].min()):.3f} deg")
    assert (real != 0).any() and r["hz"].min() < 0.0            # the relief does show the deviation
    assert (xu[real != 0] < np.sin(np.radians(5e-5))).all() and (r["f"][real != 0] > 0).all()


def test_leaves_the_context_state_alone(native_lib):
    s = scene().with_size(48, 32, spp_per_launch=16)
    dem = mc.crater_dem()
    lat, lon = np.array([10.0, -20.0, 33.0]), np.array([20.0, 95.0, -80.0])
    t0 = datetime(2025, 3, 1, tzinfo=timezone.utc)
    eps = E.sun_epochs([t0 + timedelta(hours=24 * k) for k in range(29)], OBS)

    def run(with_power):
        ctx = make(s, dem, _lib.F_COUNT_STATS)
        st1 = ctx.render(1)
        v0 = ctx.config()
        if with_power:
            hz = ctx.horizon(lat, lon, n_az=32, n_bis=8)
            ctx.power_budget(lat, lon, hz, eps, 500.0, 100.0, capacity=1 << 30)
            ctx.power_budget(lat, lon, hz, eps, 500.0, 100.0, panel="azimuth", mode="full")
        pt = ctx.illumination_at(lat, lon, n_sun=16)
        st2 = ctx.render(1)
        out = ctx.read_linear(), ctx.read_hits(), ctx.samples_done(), st1, st2, pt, v0 == ctx.config()
        ctx.close()
        return out
    a, b = run(False), run(True)
    assert_bit_equal(b[0], a[0], "linear radiance")
    assert_bit_equal(b[1], a[1], "hit buffer")
    assert_bit_equal(b[5], a[5], "illumination_at after the power budget")
    assert b[2] == a[2] == 32 and b[6]
    for k in ("primary_hits", "shadow_rays", "height_samples", "bounce_rays"):
        assert b[4][k] == a[4][k], k
