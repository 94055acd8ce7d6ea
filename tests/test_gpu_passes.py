"""Orbiter passes on the MI355X (DESIGN.md sections 3.27 and 4.33): FULL against the float64 model (tests/passes_model.py)
within the derived tolerance, SUMMARY and LIST as exact reductions of the kernel's own FULL table, the bit-exact properties,
consistency with horizon_sun's point-source rule, the refusals and the render state left alone."""
import ctypes as C

import numpy as np
import pytest

import epoch_patterns as ep
import model_cases as mc
import passes_model as pm
import terrain_cases as tc
from common import assert_bit_equal
from moonrtx_amd import _lib
from moonrtx_amd._lib import PASS_DTYPE, MrtxPasses, MrtxStats
from moonrtx_amd.renderer import DeviceBuffer, MoonRTError
from test_gpu_illumination import make

pytestmark = pytest.mark.gpu

NAN_FILL = 0x7FC12345           # a quiet NaN of known payload


@pytest.fixture(scope="module")
def rt(native_lib):
    ctx = make(pm.scene(), mc.crater_dem(), 0)
    yield ctx
    ctx.close()


def same_records(got, want, what):
    assert got.dtype == want.dtype == PASS_DTYPE and got.shape == want.shape, (what, got.shape, want.shape)
    for name in PASS_DTYPE.names:
        a, b = got[name], want[name]
        if a.dtype == np.float32:
            a, b = a.view(np.uint32), b.view(np.uint32)
        bad = np.flatnonzero(a != b)
        assert bad.size == 0, f"{what}: field {name} differs in {bad.size} records, e.g. {[(int(i), got[i], want[i]) for i in bad[:3]]}"


@pytest.mark.parametrize("rows", ["kernel", "random"])
def test_full_matches_the_model(rt, rows):
    """es within d_dir, the azimuth within d_az on the circle (below 89.9 deg), the range within range_tolerance, g within
    tol_g, and (g > 0) the model's wherever |g_model| > tol_g, of which at most 1 % are left out."""
    c = pm.case()
    lat, lon = c["lat"], c["lon"]
    hz = rt.horizon(lat, lon, n_az=pm.N_AZ, n_bis=10) if rows == "kernel" else c["hz"]
    st = {}
    got = rt.horizon_passes(lat, lon, hz, c["pos"], mode="full", stats=st)
    assert got.shape == (lat.size, 3, c["m"], 4) and got.dtype == np.float32 and st["launches"] == 1
    info = pm.look(c["scene"], c["dem"], lat, lon, hz, c["pos"])
    d_dir, d_az, tol_g = pm.tolerances(info, pm.N_AZ)
    tol_r = pm.range_tolerance(info, c["scene"])
    e_es = np.abs(got[..., 0] - info["es"])
    d = np.abs(got[..., 1] - info["az"])
    e_az = np.minimum(d, 360.0 - d)
    low = info["es"] <= 89.9
    e_r = np.abs(got[..., 2] - info["range_m"])
    e_g = np.abs(got[..., 3] - info["g"])
    sure = np.abs(info["g"]) > tol_g
    print(f"{rows} rows: worst error / tolerance: es {(e_es / d_dir).max():.3f}, azimuth {(e_az / d_az)[low].max():.3f}, "
          f"range {(e_r / tol_r).max():.3f}, g {(e_g / tol_g).max():.3f}; {(~sure).sum()} of {sure.size} margins within the "
          f"tolerance of zero; {(got[..., 3] > 0).mean():.3f} in view")
    assert (~sure).mean() <= 0.01
    assert ((got[..., 1] >= 0) & (got[..., 1] < 360)).all()
    assert (e_es <= d_dir).all(), (e_es / d_dir).max()
    assert (e_az <= d_az)[low].all(), (e_az / d_az)[low].max()
    assert (e_r <= tol_r).all(), (e_r / tol_r).max()
    assert (e_g <= tol_g).all(), (e_g / tol_g).max()
    assert ((got[..., 3] > 0) == (info["g"] > 0))[sure].all()


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("m", [1, 63, 64, 65, 129, 512])
def test_summary_and_list_are_reductions_of_full(rt, m, S):
    """Every SUMMARY column and every field of every LIST record equals the passes_model reduction of the kernel's own FULL
    table, the float32 fractions included; with and without an elevation mask."""
    c = pm.case()
    lat, lon, hz = c["lat"], c["lon"], c["hz"]
    pos = np.ascontiguousarray(c["pos"][3 - S:, :m])             # S = 1: the high orbit, whose passes span chunks
    n_rec = 0
    for mask in (0.0, 7.5):
        full = rt.horizon_passes(lat, lon, hz, pos, mode="full", min_elev_deg=mask)
        g, es, rm = full[..., 3], full[..., 0], full[..., 2]
        summ = rt.horizon_passes(lat, lon, hz, pos, mode="summary", min_elev_deg=mask)
        assert_bit_equal(summ, pm.summary(g, es), f"SUMMARY at m = {m}, S = {S}, mask {mask}")
        st = {}
        recs = rt.horizon_passes(lat, lon, hz, pos, mode="list", min_elev_deg=mask, stats=st)
        want = pm.passes(g, es, rm)
        same_records(recs, want, f"LIST at m = {m}, S = {S}, mask {mask}")
        assert st["launches"] == (3 if len(want) else 2)        # the counting call, then the count and the fill of the second
        n_rec += len(want)
    if m >= 63:
        assert n_rec > 0


def test_bit_exact_properties(native_lib):
    c = pm.case()
    lat, lon, hz, pos = c["lat"], c["lon"], c["hz"], c["pos"]
    ref = None
    for flags in (0, _lib.F_FORCE_WIDE):
        rt = make(pm.scene(), mc.crater_dem(), flags)
        out = {mode: rt.horizon_passes(lat, lon, hz, pos, mode=mode, min_elev_deg=2.0) for mode in ("full", "summary", "list")}
        if ref is None:
            ref = out
            call = lambda mode, la=lat, lo=lon, h=hz, p=pos, **kw: rt.horizon_passes(la, lo, h, p, mode=mode, min_elev_deg=2.0, **kw)   # noqa: E731
            # point order
            perm = np.random.default_rng(9).permutation(lat.size)
            for mode in ("full", "summary"):
                assert_bit_equal(call(mode, lat[perm], lon[perm], hz[perm]), out[mode][perm], f"{mode}: point order")
            inv = np.argsort(perm)
            lp = call("list", lat[perm], lon[perm], hz[perm])
            lp["point"] = perm[lp["point"]]
            same_records(lp[np.lexsort((lp["first"], lp["sat"], lp["point"]))], out["list"], "list: point order")
            assert inv.size == lat.size
            # batching, and one point alone
            for mode in ("full", "summary"):
                parts = [call(mode, lat[i:i + 7], lon[i:i + 7], hz[i:i + 7]) for i in range(0, lat.size, 7)]
                assert_bit_equal(np.concatenate(parts), out[mode], f"{mode}: batching")
                assert_bit_equal(call(mode, lat[5:6], lon[5:6], hz[5:6]), out[mode][5:6], f"{mode}: one point alone")
            parts = []
            for i in range(0, lat.size, 7):
                part = call("list", lat[i:i + 7], lon[i:i + 7], hz[i:i + 7])
                part["point"] += i
                parts.append(part)
            same_records(np.concatenate(parts), out["list"], "list: batching")
            small = rt.horizon_passes(lat, lon, hz, pos, mode="list", min_elev_deg=2.0, chunk_bytes=4096)
            same_records(small, out["list"], "list: small chunks")
            one = call("list", lat[5:6], lon[5:6], hz[5:6])
            one["point"] += 5
            same_records(one, out["list"][out["list"]["point"] == 5], "list: one point alone")
            # satellite order
            sp = np.array([2, 0, 1])
            assert_bit_equal(call("full", p=pos[sp]), out["full"][:, sp], "full: satellite order")
            ls = call("list", p=pos[sp])
            ls["sat"] = sp[ls["sat"]]
            same_records(ls[np.lexsort((ls["first"], ls["sat"], ls["point"]))], out["list"], "list: satellite order")
            summ_p = call("summary", p=pos[sp])
            assert_bit_equal(summ_p, out["summary"], "summary: satellite order")
            # no height is height zero; a raised point differs
            for mode in ("full", "summary"):
                assert_bit_equal(call(mode, height_m=np.zeros(lat.size)), call(mode, height_m=None), f"{mode}: zero heights")
                assert_bit_equal(call(mode, height_m=None), out[mode], f"{mode}: no heights")
            same_records(call("list", height_m=0.0), out["list"], "list: zero heights")
            assert (call("full", height_m=5000.0) != out["full"]).any()
            # device horizons
            buf = DeviceBuffer(hz.nbytes)
            try:
                buf.upload(hz)
                for mode in ("full", "summary"):
                    assert_bit_equal(rt.horizon_passes(lat, lon, buf, pos, mode=mode, min_elev_deg=2.0, n_az=pm.N_AZ), out[mode],
                                     f"{mode}: device horizons")
                same_records(rt.horizon_passes(lat, lon, buf, pos, mode="list", min_elev_deg=2.0, n_az=pm.N_AZ), out["list"],
                             "list: device horizons")
            finally:
                buf.free()
            # two runs
            same_records(call("list"), out["list"], "list: a second run")
        else:
            for mode in ("full", "summary"):
                assert_bit_equal(out[mode], ref[mode], f"{mode}: F_FORCE_WIDE")
            same_records(out["list"], ref["list"], "list: F_FORCE_WIDE")
        rt.close()
    assert len(ref["list"]) > 100


def raw_call(rt, k, lat, lon, hz, pos, dev_out, host_out, cap, total, st, heights=None, dev_hz=None):
    return tc.passes_call(rt._lib, rt._ctx, k, lat, lon, hz, pos, dev_out, host_out, cap, total, st, heights, dev_hz)


def test_list_sizing(rt):
    """A count-only call and an exact-cap call return the same total; a cap one short refuses the call, names the size and
    writes nothing to a sentinel-filled device table; the device table of a fitting call equals the host table."""
    c = pm.case()
    lat, lon, hz, pos = c["lat"], c["lon"], c["hz"], c["pos"]
    k = MrtxPasses(3, c["m"], _lib.PASSES_LIST, 0, pm.RADIUS_M, 0.0)
    total, st = C.c_uint64(0), MrtxStats()
    assert raw_call(rt, k, lat, lon, hz, pos, None, None, 0, total, st) == 0
    n = int(total.value)
    assert n > 100 and st.launches == 1
    host = np.zeros(n, PASS_DTYPE)
    total2 = C.c_uint64(0)
    assert raw_call(rt, k, lat, lon, hz, pos, None, host.ctypes.data, n, total2, st) == 0
    assert int(total2.value) == n and st.launches == 2
    same_records(host, rt.horizon_passes(lat, lon, hz, pos, mode="list"), "exact cap")
    words = 10 * n + 64
    buf = DeviceBuffer(words * 4)
    try:
        buf.upload(np.full(words, NAN_FILL, np.uint32))
        total3 = C.c_uint64(0)
        assert raw_call(rt, k, lat, lon, hz, pos, buf.ptr, None, n - 1, total3, st) == -1
        assert int(total3.value) == n
        assert str(n).encode() in rt._lib.mrtx_last_error(rt._ctx)
        assert np.array_equal(buf.download(np.uint32, (words,)), np.full(words, NAN_FILL, np.uint32))
        short = np.full(10 * n, NAN_FILL, np.uint32)
        assert raw_call(rt, k, lat, lon, hz, pos, None, short.ctypes.data, n - 1, total3, st) == -1
        assert (short == NAN_FILL).all()
        assert raw_call(rt, k, lat, lon, hz, pos, buf.ptr, None, n + 7, total3, st) == 0
        back = buf.download(np.uint32, (words,))
        assert np.array_equal(back[:10 * n], host.view(np.uint32)) and (back[10 * n:] == NAN_FILL).all()
    finally:
        buf.free()


def test_writes_stay_inside_the_output(rt):
    """FULL and SUMMARY into device buffers 256 words longer than the output, filled with a NaN of known payload."""
    c = pm.case()
    lat, lon, hz = c["lat"][:3], c["lon"][:3], c["hz"][:3]
    pos = np.ascontiguousarray(c["pos"][:, :65])
    for mode, code in (("full", _lib.PASSES_FULL), ("summary", _lib.PASSES_SUMMARY)):
        host = rt.horizon_passes(lat, lon, hz, pos, mode=mode)
        k = MrtxPasses(3, 65, code, 0, pm.RADIUS_M, 0.0)
        buf = DeviceBuffer((host.size + 256) * 4)
        try:
            buf.upload(np.full(host.size + 256, NAN_FILL, np.uint32))
            assert raw_call(rt, k, lat, lon, hz, pos, buf.ptr, None, 0, None, MrtxStats()) == 0
            back = buf.download(np.uint32, (host.size + 256,))
        finally:
            buf.free()
        assert np.array_equal(back[:host.size], host.view(np.uint32).ravel()), mode
        assert (back[host.size:] == NAN_FILL).all(), mode


def test_consistent_with_the_point_source_rule(rt):
    """One satellite with min_elev_deg = -90, and the same positions as zero-radius MrtxIllumEpoch rows through one Moon frame:
    horizon_sun FULL equals (g > 0) wherever |g| > tol_g."""
    c = pm.case()
    lat, lon, hz = c["lat"], c["lon"], c["hz"]
    pos = np.ascontiguousarray(c["pos"][1:2])
    g = rt.horizon_passes(lat, lon, hz, pos, mode="full", min_elev_deg=-90.0)[:, 0, :, 3]
    row = ep.frame_row()
    ez = row[8:11] / np.linalg.norm(row[8:11])
    v0 = row[11:14] - (row[11:14] @ ez) * ez
    v0 /= np.linalg.norm(v0)
    Mf = np.stack([np.cross(ez, v0), v0, ez])
    epochs = np.tile(row, (pos.shape[1], 1))
    epochs[:, 0:3] = row[5:8] + pm.scene_positions(c["scene"], pos)[0] @ Mf
    epochs[:, 3] = 0.0
    f = rt.horizon_sun(lat, lon, hz, epochs)
    info = pm.look(c["scene"], c["dem"], lat, lon, hz, pos, min_elev_deg=-90.0)
    tol_g = pm.tolerances(info, pm.N_AZ)[2][:, 0]
    sure = np.abs(g) > tol_g
    print(f"{(~sure).sum()} of {sure.size} margins within the tolerance of zero; {(g > 0).mean():.3f} in view")
    assert set(np.unique(f).tolist()) <= {0.0, 1.0} and sure.mean() > 0.99
    assert ((f == 1.0) == (g > 0))[sure].all()
    assert (g > 0).any() and (g <= 0).any()


def test_refusals(rt):
    """Each refused with MRTX_E_INVALID before any launch: the statistics block is not touched."""
    c = pm.case()
    lat, lon, hz = c["lat"][:4], c["lon"][:4], c["hz"][:4]
    pos = np.ascontiguousarray(c["pos"][:, :16])
    R_m = pm.RADIUS_M
    out = np.zeros((4, 8), np.float32)
    buf = DeviceBuffer(4 * 3 * 16 * 16 + 64)
    ok = MrtxPasses(3, 16, _lib.PASSES_SUMMARY, 0, R_m, 0.0)
    try:
        st = MrtxStats()
        assert raw_call(rt, ok, lat, lon, hz, pos, None, out.ctypes.data, 0, None, st) == 0 and st.launches == 1
        # 1.004 R is outside the bounding sphere; the list refuses it with a raise of 10 km
        near = pos.copy()
        near[1, 7] = pos[1, 7] / np.linalg.norm(pos[1, 7]) * (1.004 * R_m)
        assert raw_call(rt, ok, lat, lon, hz, near, None, out.ctypes.data, 0, None, MrtxStats()) == 0
        out[:] = 0.0
        for text, _, kw in tc.passes_refusals(pos, out, buf.ptr):       # the list (tests/terrain_cases.py)
            st = MrtxStats()
            st.launches = tc.LAUNCHES
            rc = tc.passes_call(rt._lib, rt._ctx, kw.pop("k"), lat, lon, hz, kw.pop("pos"), total=C.c_uint64(0), st=st, **kw)
            tc.refused(rt._lib, rt._ctx, rc, st, text)
            assert (out == 0.0).all(), "a refused call wrote: " + text
        inside = pos.copy()
        inside[1, 7] = pos[1, 7] / np.linalg.norm(pos[1, 7]) * (1.0005 * R_m)
        with pytest.raises(MoonRTError):
            rt.horizon_passes(lat, lon, hz, inside)
    finally:
        buf.free()


def test_leaves_the_context_state_alone(native_lib):
    s = pm.scene().with_size(48, 32, spp_per_launch=16)
    dem = mc.crater_dem()
    c = pm.case()
    lat, lon = np.array([10.0, -20.0, 33.0]), np.array([20.0, 95.0, -80.0])
    pos = np.ascontiguousarray(c["pos"][:, :130])

    def run(with_passes):
        rt = make(s, dem, _lib.F_COUNT_STATS)
        st1 = rt.render(1)
        v0 = rt.config()
        if with_passes:
            hz = rt.horizon(lat, lon, n_az=32, n_bis=8, height_m=[0.0, 2.0, 100.0])
            for mode in ("full", "summary", "list"):
                rt.horizon_passes(lat, lon, hz, pos, mode=mode, height_m=[0.0, 2.0, 100.0])
        pt = rt.illumination_at(lat, lon, n_sun=16)
        st2 = rt.render(1)
        out = rt.read_linear(), rt.read_hits(), rt.samples_done(), st1, st2, pt, v0 == rt.config()
        rt.close()
        return out
    a, b = run(False), run(True)
    assert_bit_equal(b[0], a[0], "linear radiance")
    assert_bit_equal(b[1], a[1], "hit buffer")
    assert_bit_equal(b[5], a[5], "illumination_at after the passes")
    assert b[2] == a[2] == 32 and b[6]
    for k in ("primary_hits", "shadow_rays", "height_samples", "bounce_rays"):
        assert b[4][k] == a[4][k], k
