"""The epoch walkers' wave reductions on the MI355X at every 64-epoch chunk edge (DESIGN.md sections 3.9, 3.15 and 4.16):
horizon_sun_kernel (FULL and SUMMARY) and horizon_windows_kernel driven with designed bit patterns (tests/epoch_patterns.py),
a point light, the horizon row's seam, thresholds at equality and the extent of their writes.  Every comparison is bitwise
over every entry: the designed fractions are exactly 0 or 1 (tests/test_epoch_patterns_host.py shows the horizon 34.73 deg
from the disc's edge), so nothing is excluded and nothing carries a tolerance.  Both addressing builds (flags 0 and
F_FORCE_WIDE) run every case; no march runs."""
import ctypes as C

import numpy as np
import pytest

import epoch_patterns as ep
import mast_model as mm
import model_cases as mc
from common import assert_bit_equal
from moonrtx_amd import _lib
from moonrtx_amd._lib import MrtxStats
from moonrtx_amd.renderer import DeviceBuffer
from moonrtx_amd.scene import named_scene
from test_gpu_illumination import make

pytestmark = pytest.mark.gpu

LAT, LON, N_AZ, SEED = 23.0, -57.0, 1024, 0
NAN_FILL = 0x7FC12345           # a quiet NaN of known payload


def scene():
    return named_scene("S1", 16, 16)


@pytest.fixture(scope="module", params=[0, _lib.F_FORCE_WIDE], ids=["narrow", "wide"])
def rt(request, native_lib):
    ctx = make(scene(), mc.crater_dem(), request.param)
    yield ctx
    ctx.close()


def site(P):
    return np.full(P, LAT), np.full(P, LON)


def check_designed(rt, m, radius_b):
    """All patterns of patterns(m) in one call as P points: FULL, SUMMARY and the windows against the designed bits and their
    plain-loop reductions, then from device horizons and in calls of 7 points."""
    s, dem = scene(), mc.crater_dem()
    names, a, b = ep.stack(ep.patterns(m, SEED))
    P = len(names)
    lat, lon = site(P)
    hz = ep.horizon_rows(a, b, N_AZ)
    sa, sb = ep.sectors_of(m, N_AZ)
    ea = ep.lights(s, dem, LAT, LON, sa, N_AZ)
    eb = ep.lights(s, dem, LAT, LON, sb, N_AZ, radius_deg=radius_b)

    def where(got, want):
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        return f"m = {m}: {len(bad)} entries differ, e.g. " + "; ".join(
            f"pattern {names[p]} column {j}: {got[p, j]!r} for {want[p, j]!r}" for p, j in bad[:4])

    def same(got, want, what):
        assert got.shape == want.shape and got.dtype == want.dtype == np.float32
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{what}: {where(got, want)}"

    # FULL first: a later failure then points at the reduction
    full = [rt.horizon_sun(lat, lon, hz, e) for e in (ea, eb)]
    same(full[0], a.astype(np.float32), "FULL of A")
    same(full[1], b.astype(np.float32), "FULL of B")
    summ = [rt.horizon_sun(lat, lon, hz, e, summary=True) for e in (ea, eb)]
    same(summ[0], ep.expect_summary(a), "SUMMARY of A")
    same(summ[1], ep.expect_summary(b), "SUMMARY of B")
    want = ep.expect_windows(a, b)
    wins = [rt.horizon_windows(lat, lon, hz, ea, eb, min_a=t, min_b=t) for t in (1.0, 0.5)]
    same(wins[0], want, "windows at 1.0, 1.0")
    same(wins[1], want, "windows at 0.5, 0.5")
    # a DeviceBuffer of the same horizons
    buf = DeviceBuffer(hz.nbytes)
    try:
        buf.upload(hz)
        for e, f, q in zip((ea, eb), full, summ):
            same(rt.horizon_sun(lat, lon, buf, e, n_az=N_AZ), f, "FULL from device horizons")
            same(rt.horizon_sun(lat, lon, buf, e, summary=True, n_az=N_AZ), q, "SUMMARY from device horizons")
        for t, w in zip((1.0, 0.5), wins):
            same(rt.horizon_windows(lat, lon, buf, ea, eb, min_a=t, min_b=t, n_az=N_AZ), w, "windows from device horizons")
    finally:
        buf.free()
    # the points in calls of 7
    parts = range(0, P, 7)
    same(np.concatenate([rt.horizon_sun(lat[i:i + 7], lon[i:i + 7], hz[i:i + 7], eb) for i in parts]), full[1], "FULL in 7s")
    same(np.concatenate([rt.horizon_sun(lat[i:i + 7], lon[i:i + 7], hz[i:i + 7], ea, summary=True) for i in parts]), summ[0],
         "SUMMARY in 7s")
    same(np.concatenate([rt.horizon_windows(lat[i:i + 7], lon[i:i + 7], hz[i:i + 7], ea, eb, min_a=1.0, min_b=1.0)
                         for i in parts]), wins[0], "windows in 7s")


@pytest.mark.parametrize("m", ep.M)
def test_designed_patterns(rt, m):
    check_designed(rt, m, 0.27)


@pytest.mark.parametrize("m", [65, 129])
def test_point_light(rt, m):
    """Table B's lights have radius 0: disc_fraction's alpha == 0 branch through FULL, SUMMARY and the windows."""
    check_designed(rt, m, 0.0)


@pytest.mark.parametrize("fill", [80.0, -80.0])
@pytest.mark.parametrize("n_az", [4, 64])
def test_the_horizon_rows_seam(rt, n_az, fill):
    """Lights half a sample before north, at +10 and -10 deg; the row's last sample is +40 and its first -40, so the horizon
    there is 0 only if the upper neighbour of sample n_az - 1 is sample 0 of the SAME row (the point is the last of three);
    every other sample is `fill`, which hides the upper light or shows the lower one."""
    s, dem = scene(), mc.crater_dem()
    lat, lon = site(3)
    hz = np.full((3, n_az), fill, np.float32)
    hz[:, n_az - 1], hz[:, 0] = 40.0, -40.0
    x = [n_az - 0.5, n_az - 0.5]
    ea = ep.lights(s, dem, LAT, LON, x, n_az, elev_deg=[10.0, -10.0])
    eb = ep.lights(s, dem, LAT, LON, x, n_az, elev_deg=[-10.0, 10.0])
    a, b = np.tile([True, False], (3, 1)), np.tile([False, True], (3, 1))
    assert_bit_equal(rt.horizon_sun(lat, lon, hz, ea), a.astype(np.float32), "FULL of A")
    assert_bit_equal(rt.horizon_sun(lat, lon, hz, eb), b.astype(np.float32), "FULL of B")
    assert_bit_equal(rt.horizon_sun(lat, lon, hz, ea, summary=True), ep.expect_summary(a), "SUMMARY of A")
    assert_bit_equal(rt.horizon_sun(lat, lon, hz, eb, summary=True), ep.expect_summary(b), "SUMMARY of B")
    assert_bit_equal(rt.horizon_windows(lat, lon, hz, ea, eb, min_a=1.0, min_b=1.0), ep.expect_windows(a, b), "windows")
    assert_bit_equal(rt.horizon_windows(lat, lon, hz, ea, ea, min_a=0.5, min_b=0.5), ep.expect_windows(a, a), "windows of A, A")


def test_thresholds_at_equality(rt):
    """A flat horizon at 0 and 130 lights stepping from -0.4 to +0.4 deg with a radius of 0.27 deg: FULL sweeps 0 .. 1 through
    partial discs.  With min_a = a partial FULL value f, and then the next float32 above it, the windows equal
    mast_model.windows of the two FULL outputs bit for bit; the first call counts f's epoch, the second does not."""
    s, dem = scene(), mc.crater_dem()
    m, n_az = 130, 64
    lat, lon = site(3)
    hz = np.zeros((3, n_az), np.float32)
    sectors = np.arange(m) % n_az
    elev = np.linspace(-0.4, 0.4, m)
    ea = ep.lights(s, dem, LAT, LON, sectors, n_az, elev_deg=elev)
    eb = ep.lights(s, dem, LAT, LON, sectors, n_az, elev_deg=elev[::-1])
    fa, fb = rt.horizon_sun(lat, lon, hz, ea), rt.horizon_sun(lat, lon, hz, eb)
    assert fa[0, 0] == 0.0 and fa[0, -1] == 1.0 and fb[0, 0] == 1.0 and fb[0, -1] == 0.0
    partial = np.flatnonzero((fa[0] > 0) & (fa[0] < 1))
    assert partial.size >= 60, partial.size                     # |e| < 0.27 deg at 87 of the 130 steps
    for k in partial[np.linspace(0, partial.size - 1, 8).astype(int)]:
        f = np.float32(fa[0, k])
        up = np.nextafter(f, np.float32(2))
        counts = []
        for min_a in (float(f), float(up)):
            got = rt.horizon_windows(lat, lon, hz, ea, eb, min_a=min_a, min_b=0.5)
            want, cnt = mm.windows(fa, fb, min_a, 0.5)
            assert_bit_equal(got, want.astype(np.float32), f"epoch {k}: windows at min_a = {min_a!r}")
            counts.append(cnt[:, 0])
        at_f = (fa == f).sum(1)
        assert (at_f >= 1).all() and np.array_equal(counts[0] - counts[1], at_f), (k, f, counts)
        assert np.float32(counts[0][0] / float(m)) != np.float32(counts[1][0] / float(m))


def test_writes_stay_inside_the_output(rt):
    """FULL (n = 3, m = 65), SUMMARY and the windows into a device buffer 256 floats longer than the output, filled with a NaN
    of known payload: the tail comes back unchanged bit for bit and the head equals the host-output call."""
    s, dem = scene(), mc.crater_dem()
    m, n, tail = 65, 3, 256
    pats = [p for p in ep.patterns(m, SEED) if p[0] in ("A=random0.5,B=all1", "A=all1,B=run[60,130)", "A=one1@64,B=all1")]
    names, a, b = ep.stack(pats)
    assert len(names) == n
    lat, lon = site(n)
    hz = ep.horizon_rows(a, b, N_AZ)
    sa, sb = ep.sectors_of(m, N_AZ)
    ea, eb = ep.lights(s, dem, LAT, LON, sa, N_AZ), ep.lights(s, dem, LAT, LON, sb, N_AZ)
    pts = np.ascontiguousarray(np.stack([lat, lon], -1))
    lib, ctx = rt._lib, rt._ctx

    def sun(mode):
        return lambda dev: lib.mrtx_horizon_sun(ctx, pts.ctypes.data, n, N_AZ, None, hz.ctypes.data, ea.ctypes.data, m, mode, dev,
                                                None, C.byref(MrtxStats()))

    def windows(dev):
        return lib.mrtx_horizon_windows(ctx, pts.ctypes.data, n, N_AZ, None, hz.ctypes.data, ea.ctypes.data, eb.ctypes.data, m,
                                        1.0, 1.0, dev, None, C.byref(MrtxStats()))
    cases = (("FULL", sun(0), rt.horizon_sun(lat, lon, hz, ea), a.astype(np.float32)),
             ("SUMMARY", sun(1), rt.horizon_sun(lat, lon, hz, ea, summary=True), ep.expect_summary(a)),
             ("windows", windows, rt.horizon_windows(lat, lon, hz, ea, eb, min_a=1.0, min_b=1.0), ep.expect_windows(a, b)))
    for what, call, host, want in cases:
        assert_bit_equal(host, want, f"{what}: host output")
        size = host.size
        buf = DeviceBuffer((size + tail) * 4)
        try:
            buf.upload(np.full(size + tail, NAN_FILL, np.uint32))
            rt._check(call(buf.ptr), what)
            back = buf.download(np.uint32, (size + tail,))
        finally:
            buf.free()
        assert np.array_equal(back[:size], host.view(np.uint32).ravel()), f"{what}: device output differs from host output"
        assert np.array_equal(back[size:], np.full(tail, NAN_FILL, np.uint32)), f"{what}: wrote past its {size} floats"
