"""Drive masks on the MI355X (DESIGN.md sections 3.19 and 4.22): mrtx_horizon_mask's bits against the predicate formed on the
host from horizon_sun FULL, bit for bit, the tail bits, the counts and runs of horizon_windows, one table alone, device and host
outputs, WIDE addressing and the counting build, ground and raised horizons, and the render state left alone."""
from datetime import datetime, timedelta, timezone

import numpy as np
import pytest

import horizon_model as hm
import model_cases as mc
from common import assert_bit_equal
from moonrtx_amd import _lib
from moonrtx_amd import ephemeris as E
from moonrtx_amd import traverse as tv
from moonrtx_amd.renderer import DeviceBuffer
from test_gpu_horizon import FLAG_SETS, OBS, points, scene
from test_gpu_illumination import make

pytestmark = pytest.mark.gpu

N_AZ = 32
MS = (1, 63, 64, 65, 200)
DEMS = {"craters": mc.crater_dem, "egg-crate": mc.corrugated_dem}
# The dates: 200 epochs 6 h apart from 2025-03-01 (50 days: every point of points(11, 24) sees a sunrise); the shorter tables
# are their first m.  Share of the 24 points whose mask is neither all 0 nor all 1, measured on the CPU from the model alone
# (horizon_model.horizon at 32 azimuths x 10 probes, then sun_fraction, min_a = 0.5, min_b = 1.0), per m = 63 / 64 / 65 / 200
# (a single epoch, m = 1, is all 0 or all 1 by itself):
#   Sun alone                 craters 1.00 / 1.00 / 1.00 / 1.00    egg-crate 0.92 / 0.92 / 0.92 / 1.00
#   Sun and Sun 5 days on     craters 0.83 / 0.83 / 0.83 / 1.00    egg-crate 0.75 / 0.75 / 0.75 / 1.00
#   Sun and Earth             craters 0.42 / 0.42 / 0.42 / 0.46    egg-crate 0.38 / 0.38 / 0.38 / 0.38
# The Earth stands still in the lunar sky: 13 (craters: its 0.46) of the 24 points lie on the far side and never see it on any
# date, so the joint Sun / Earth mask cannot be mixed at half of them.  The joint comparison therefore runs on two tables
# that are mixed nearly everywhere -- the Sun and the Sun five days later (a second body that rises and sets at every
# point) -- and on the Sun / Earth pair besides; the floor of one half is asserted for the first two rows.
T0 = datetime(2025, 3, 1, tzinfo=timezone.utc)
TIMES = [T0 + timedelta(hours=6 * k) for k in range(200)]


def tables(kind):
    if kind == "sun-earth":
        return E.sun_earth_epochs(TIMES, OBS)
    return E.sun_epochs(TIMES, OBS), E.sun_epochs([t + timedelta(days=5) for t in TIMES], OBS)


def mixed_share(bits):
    n = bits.sum(1)
    return float(((n > 0) & (n < bits.shape[1])).mean())


def longest_runs(bits):
    return np.array([hm.longest_run(row) for row in bits])


@pytest.mark.parametrize("name", sorted(DEMS))
def test_the_models_masks_are_mixed(name):
    """The condition above, from the model alone (no GPU work: it only guards the choice of dates)."""
    s, dem = scene(), DEMS[name]()
    lat, lon = points(11, 24)
    hz = hm.horizon(s, dem, lat, lon, N_AZ, 10)["elev"]
    ea, eb = tables("sun-sun")
    fa = hm.sun_fraction(s, dem, lat, lon, hz, ea)[0].astype(np.float32)
    fb = hm.sun_fraction(s, dem, lat, lon, hz, eb)[0].astype(np.float32)
    for m in MS[1:]:
        a, b = fa[:, :m] >= np.float32(0.5), fb[:, :m] >= np.float32(1.0)
        print(f"{name}, m = {m}: mixed at {mixed_share(a):.2f} (Sun alone), {mixed_share(a & b):.2f} (joint)")
        assert mixed_share(a) >= 0.5 and mixed_share(a & b) >= 0.5


@pytest.mark.parametrize("kind", ["sun-sun", "sun-earth"])
@pytest.mark.parametrize("name", sorted(DEMS))
def test_bits_are_the_predicate_of_full(native_lib, name, kind):
    s, dem = scene(), DEMS[name]()
    lat, lon = points(11, 24)
    ea, eb = tables(kind)
    rt = make(s, dem, 0)
    hz = rt.horizon(lat, lon, n_az=N_AZ, n_bis=10)
    fa, fb = rt.horizon_sun(lat, lon, hz, ea), rt.horizon_sun(lat, lon, hz, eb)
    assert fa.dtype == np.float32 and fa.shape == (24, 200)
    # thresholds: the defaults, the smallest, and a min that equals one of the f values exactly (equality counts as met)
    part = np.argwhere((fa > 0) & (fa < 1))
    assert len(part) > 0
    pa, ka = part[len(part) // 2]
    partb = np.argwhere((fb > 0) & (fb < 1))
    pb, kb = partb[len(partb) // 2] if len(partb) else (0, 0)
    exact_a, exact_b = float(fa[pa, ka]), float(fb[pb, kb]) if len(partb) else 1.0
    buf = DeviceBuffer(hz.nbytes)
    buf.upload(hz)
    for m in MS:
        W64 = (m + 63) // 64
        for min_a, min_b in ((0.5, 1.0), (1e-6, 1e-6), (exact_a, exact_b)):
            st = {}
            got = rt.horizon_mask(lat, lon, hz, ea[:m], eb[:m], min_a=min_a, min_b=min_b, stats=st)
            assert got.shape == (24, W64) and got.dtype == np.uint64 and st["launches"] == 1
            want = (fa[:, :m] >= np.float32(min_a)) & (fb[:, :m] >= np.float32(min_b))
            assert np.array_equal(got, tv.pack_mask(want)), (m, min_a, min_b, int((tv.unpack_mask(got, m) != want).sum()))
            if m % 64:
                assert not (got[:, -1] >> np.uint64(m % 64)).any()          # tail bits are zero
            bits = tv.unpack_mask(got, m)
            # popcount / m and the longest run of set bits: horizon_windows' columns 4 and 5
            win = rt.horizon_windows(lat, lon, hz, ea[:m], eb[:m], min_a=min_a, min_b=min_b)
            assert np.array_equal(win[:, 4], (bits.sum(1) / float(m)).astype(np.float32))
            assert np.array_equal(win[:, 5], longest_runs(bits).astype(np.float32))
            # one table alone: ok_a, whatever min_b says
            one = rt.horizon_mask(lat, lon, hz, ea[:m], None, min_a=min_a, min_b=min_b)
            assert np.array_equal(one, tv.pack_mask(fa[:, :m] >= np.float32(min_a)))
            assert np.array_equal(rt.horizon_mask(lat, lon, hz, ea[:m], min_a=min_a, min_b=7.0), one)
            # device horizons and a device output (behind an offset), batches of points
            out = DeviceBuffer(got.nbytes + 64)
            assert rt.horizon_mask(lat, lon, buf, ea[:m], eb[:m], min_a=min_a, min_b=min_b, n_az=N_AZ, out=out, out_offset=64) is out
            assert np.array_equal(out.download(np.uint64, (24 * W64 + 8,))[8:].reshape(24, W64), got)
            out.free()
            parts = [rt.horizon_mask(lat[i:i + 7], lon[i:i + 7], hz[i:i + 7], ea[:m], eb[:m], min_a=min_a, min_b=min_b)
                     for i in range(0, 24, 7)]
            assert np.array_equal(np.concatenate(parts), got)
        if m == 200:
            assert bits.shape == (24, 200)
            assert tv.unpack_mask(rt.horizon_mask(lat, lon, hz, ea, None, min_a=exact_a), 200)[pa, ka]      # equality is met
            print(f"{name}, {kind}: mixed at {mixed_share((fa >= np.float32(0.5)) & (fb >= np.float32(1.0))):.2f} of the points")
    buf.free()
    rt.close()


def test_flag_sets_and_raised_horizons_agree(native_lib):
    """F_FORCE_WIDE and the counting build give the default's bits; a raised horizon's mask is the predicate of its own FULL."""
    s, dem = scene(), mc.crater_dem()
    lat, lon = points(11, 24)
    ea, eb = tables("sun-earth")
    ref = None
    for flags in FLAG_SETS:
        rt = make(s, dem, flags)
        hz = rt.horizon(lat, lon, n_az=N_AZ, n_bis=10)
        got = [rt.horizon_mask(lat, lon, hz, ea[:m], eb[:m], min_a=0.5, min_b=0.5) for m in (65, 200)]
        if ref is None:
            ref = got
            hr = rt.horizon(lat, lon, n_az=N_AZ, n_bis=10, height_m=100.0)
            fa, fb = rt.horizon_sun(lat, lon, hr, ea), rt.horizon_sun(lat, lon, hr, eb)
            raised = rt.horizon_mask(lat, lon, hr, ea, eb, min_a=0.5, min_b=0.5)
            assert np.array_equal(raised, tv.pack_mask((fa >= np.float32(0.5)) & (fb >= np.float32(0.5))))
            assert (raised != got[1]).any()
        for a, b in zip(got, ref):
            assert np.array_equal(a, b), flags
        rt.close()


def test_leaves_the_render_state_alone(native_lib):
    s = scene().with_size(48, 32, spp_per_launch=16)
    dem = mc.crater_dem()
    lat, lon = np.array([10.0, -20.0, 33.0]), np.array([20.0, 95.0, -80.0])
    ea, eb = tables("sun-earth")

    def run(with_mask):
        rt = make(s, dem, _lib.F_COUNT_STATS)
        st1 = rt.render(1)
        v0 = rt.config()
        if with_mask:
            hz = rt.horizon(lat, lon, n_az=N_AZ, n_bis=8)
            rt.horizon_mask(lat, lon, hz, ea[:70], eb[:70])
            rt.horizon_mask(lat, lon, hz, ea[:70])
        pt = rt.illumination_at(lat, lon, n_sun=16)
        st2 = rt.render(1)
        out = rt.read_linear(), rt.read_hits(), rt.samples_done(), st1, st2, pt, v0 == rt.config()
        rt.close()
        return out
    a, b = run(False), run(True)
    assert_bit_equal(b[0], a[0], "linear radiance")
    assert_bit_equal(b[1], a[1], "hit buffer")
    assert_bit_equal(b[5], a[5], "illumination_at after the mask stage")
    assert b[2] == a[2] == 32 and b[6]
    for k in ("primary_hits", "shadow_rays", "height_samples", "bounce_rays"):
        assert b[4][k] == a[4][k], k
