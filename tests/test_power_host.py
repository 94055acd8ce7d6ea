"""The site power budget without a GPU (DESIGN.md sections 3.17 and 4.19): known answers of the model (tests/power_model.py),
the Python restatement of the kernel's chunk-and-carry walk against the model on every designed sequence, the sequences
against every named defect of that walk, mrtx_power_budget's argument checks, and the Python layer's quantisation and calls."""
import ctypes as C
import os
import re
from datetime import datetime, timedelta, timezone

import numpy as np
import pytest

import epoch_patterns as ep
import power_model as pm
from moonrtx_amd import _lib
from moonrtx_amd import ephemeris as E
from moonrtx_amd import renderer as rmod
from moonrtx_amd import sunlight
from moonrtx_amd.renderer import MoonRT

E_INVALID, E_STATE = -1, -3
INF, NAN = float("inf"), float("nan")
OBS = E.Observer(52.2, 21.0, 0.0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0


# ---- known answers -------------------------------------------------------------------------------------------------------------
def test_known_answers_of_the_model():
    # nothing happens: no drawdown, the battery stays where it was
    assert pm.budget([0] * 5, 10, 4) == [0, 0, 0, -1, -1, 4, 0, 0]
    # a single deficit of 7 at epoch 2: the drawdown is that epoch alone
    assert pm.budget([3, 0, -7, 1], 100, 100) == [4, -3, 7, 2, 2, 93, 0, 0]
    assert pm.budget([3, 0, -7, 1], 5, 5) == [4, -3, 7, 2, 2, 0, 1, 2]
    # two equal drawdowns: the earlier end wins
    assert pm.budget([5, -5, 5, -5], 100, 100)[2:5] == [5, 1, 1]
    # two equal peaks (S = 5 after epochs 0 and 2): the later one starts the shortest interval
    assert pm.budget([5, -2, 2, -4], 100, 100)[2:5] == [4, 3, 3]
    # S_-1 = 0 is a peak like any other, and S_1 = 0 is the later one
    assert pm.budget([-1, 1, -3], 100, 100)[2:5] == [3, 2, 2]
    # a deficit from the start: the interval starts at epoch 0
    assert pm.budget([-2, -2, 1], 100, 100)[2:5] == [4, 0, 1]
    # a night broken by one lit epoch is one drawdown, not two
    assert pm.budget([-3, -3, 1, -3, -3, 20], 100, 100)[2:5] == [11, 0, 4]
    # column [0] is the generated energy, given or max(e, 0)
    assert pm.budget([1, -1], 0, 0, g=[9, 4])[0] == 13 and pm.budget([1, -1], 0, 0)[0] == 1


@pytest.mark.parametrize("m", ep.M)
def test_the_drawdown_is_the_capacity_that_never_empties(m):
    """capacity = D starting full: the battery touches 0 and always carries the load; capacity = D - 1 does not; capacity = 0
    meets no deficit at all."""
    names, e = pm.stack(pm.sequences(m, SEED))
    for name, row in zip(names, e):
        D = pm.budget(row, 0, 0)[2]
        at_d = pm.budget(row, D, D)
        assert at_d[5:8] == [0, 0, 0], (m, name, at_d)
        if D >= 1:
            assert pm.budget(row, D - 1, D - 1)[6] >= 1, (m, name)
        none = pm.budget(row, 0, 0)
        neg = [-int(x) for x in row if x < 0]
        assert none[5:8] == [0, len(neg), sum(neg)], (m, name, none)


# ---- the chunk-and-carry walk ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", ep.M)
def test_the_chunked_walk_equals_the_truth(m):
    names, e = pm.stack(pm.sequences(m, SEED))
    for cap, ini in pm.CONFIGS:
        for name, row in zip(names, e):
            assert pm.chunked_budget(row, cap, ini) == pm.budget(row, cap, ini), (m, name, cap, ini)


def test_sequence_names_are_unique_and_cover_the_edges():
    for m in ep.M:
        names, e = pm.stack(pm.sequences(m, SEED))
        assert len(set(names)) == len(names) and e.shape == (len(names), m) and e.dtype == np.int64
        assert np.array_equal(e.astype(np.float32).astype(np.int64), e)        # float32 tables of watts hold every entry exactly
        pm.split(e)
    names, e = pm.stack(pm.sequences(512, SEED))
    for want in ("peak@63,trough@64", "drawdown-3-chunks", "equal-drawdowns:chunk0", "equal-drawdowns:chunks", "equal-peaks:chunk0",
                 "equal-peaks:chunks", "clamp:chunk0", "clamp:edge", "all-2^28", "last-epoch-trough", "random0.05", "random0.5",
                 "random0.95"):
        assert want in names, want
    # the designs do what their names say
    row = dict(zip(names, e))
    b = pm.budget(row["peak@63,trough@64"], 1000, 1000)
    assert b[3:5] == [64, 64]
    b = pm.budget(row["drawdown-3-chunks"], 1000, 1000)
    assert b[2:5] == [140, 10, 149]
    assert abs(pm.budget(row["all-2^28"], 0, 0)[1]) > 1 << 32
    for name in ("clamp:chunk0", "clamp:edge"):
        s, hit = 11, set()
        for x in row[name]:
            t = s + int(x)
            s = min(37, max(0, t))
            hit |= {"top"} if t > 37 else {"bottom"} if t < 0 else set()
        assert hit == {"top", "bottom"}, name
    assert 65 in ep.M and 129 in ep.M and 193 in ep.M          # a last chunk of one lane


# Two defects cannot show in an output.  carry_from_lane_63: the carries are read from `last` = min(64, m - k0) - 1, which
# differs from 63 only in a chunk that is not full, and only the final chunk can be that: its carries are never read.
# inactive_lanes_with_peak: a lane past m - 1 walked as an epoch with e = 0 repeats the last balance S_{m-1}, so its drawdown is
# max(peak, S_{m-1}) - S_{m-1}: the last epoch's own drawdown or 0, never strictly greater than the one held; the peak it may
# move to a later index is read by later lanes of the same kind only; its t = s_{m-1} + 0 >= 0 counts nothing and its s_k
# repeats a value the minimum already holds.  Both are asserted EQUAL on every sequence instead of killed.
UNOBSERVABLE = ("carry_from_lane_63", "inactive_lanes_with_peak")


def test_the_sequences_kill_every_observable_mutant():
    """Adequacy: for every named defect of the walk that can change an output there is an (m, sequence, battery) whose eight
    columns differ from the truth -- the first one found is printed with the columns that differ -- so a kernel with that
    defect fails tests/test_gpu_power.py."""
    cases = {m: pm.stack(pm.sequences(m, SEED)) for m in ep.M}
    killed = {}
    for mutant in pm.MUTANTS:
        kills = []
        for m, (names, e) in cases.items():
            for cap, ini in pm.CONFIGS:
                for name, row in zip(names, e):
                    got, want = pm.chunked_budget(row, cap, ini, mutant=mutant), pm.budget(row, cap, ini)
                    if got != want:
                        kills.append((m, name, (cap, ini), [j for j in range(8) if got[j] != want[j]]))
        killed[mutant] = kills
        if kills:
            m, name, cfg, cols = kills[0]
            print(f"{mutant}: killed by {len(kills)} (m, sequence, battery)s at {len({k[0] for k in kills})} epoch counts, "
                  f"first m = {m}, {name}, battery {cfg}, columns {cols}")
        else:
            print(f"{mutant}: equal to the truth on every (m, sequence, battery)")
    for mutant in pm.MUTANTS:
        if mutant in UNOBSERVABLE:
            assert not killed[mutant], (mutant, killed[mutant][:3])
        else:
            assert killed[mutant], f"{mutant} survives every sequence"
    # the tie rules are caught by the designed ties, in the interval's columns alone
    for mutant, name, cols in (("peak_tie_takes_earlier", "equal-peaks:chunk0", [3]), ("peak_tie_takes_earlier", "equal-peaks:chunks", [3]),
                               ("drawdown_tie_takes_later", "equal-drawdowns:chunk0", [3, 4]),
                               ("drawdown_tie_takes_later", "equal-drawdowns:chunks", [3, 4])):
        assert any(k[0] == 512 and k[1] == name and k[3] == cols for k in killed[mutant]), (mutant, name)
    # the carries matter from the second chunk on, the 32-bit sums from 2^28 x 16 epochs on
    assert {k[0] for k in killed["no_S_carry"]} >= {65, 127, 128, 129, 191, 192, 193, 512}
    assert {k[0] for k in killed["no_peak_carry"]} >= {65, 127, 128, 129, 191, 192, 193, 512}
    assert {k[0] for k in killed["accumulate_32_bit"]} >= {63, 64, 65, 512}
    assert {k[0] for k in killed["clamp_order_swapped"]} >= {2, 63, 64, 65, 512}


def test_the_unobservable_mutants_leave_the_same_carries():
    """Behind a final chunk of one lane the two defects that no output shows leave the carries of the correct walk as well:
    a lane past m - 1 holds e = 0, so lane 63 repeats the last balance, peak and state of charge."""
    for e in ([5] * 64 + [-9], [5] * 64 + [9]):
        good = pm.chunked_budget(e, 10, 10, carries=True)
        for mutant in UNOBSERVABLE:
            assert pm.chunked_budget(e, 10, 10, mutant=mutant, carries=True) == good, (mutant, e[-1])
    assert pm.chunked_budget([5] * 64 + [9], 10, 10, carries=True)[1] == (329, 329, 64, 10)


# ---- ABI and argument checks -------------------------------------------------------------------------------------------------
def test_the_entry_point_is_declared_exported_and_bound(native_lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "moonrt.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+mrtx_power_budget\s*\(", text)
    assert "mrtx_power_budget" in _lib.SIGNATURES and native_lib.mrtx_power_budget is not None
    assert native_lib.mrtx_abi_version() == 7 == _lib.ABI_VERSION
    # int32, 4 bytes of padding, 3 doubles, int32, 4 bytes of padding, 2 int64: the C layout of the header's struct
    assert C.sizeof(_lib.MrtxPowerModel) == 56
    assert [getattr(_lib.MrtxPowerModel, f).offset for f, _ in _lib.MrtxPowerModel._fields_] == [0, 8, 32, 40, 48]
    fields = re.search(r"typedef struct MrtxPowerModel \{(.*?)\} MrtxPowerModel;", text, flags=re.S).group(1)
    assert re.findall(r"\b(\w+)(?:\[\d+\])?;", fields) == [f for f, _ in _lib.MrtxPowerModel._fields_]


@pytest.fixture
def ctx(native_lib):
    """A context handle; without a GPU mrtx_create stops at its first HIP call but hands the context out."""
    c = C.c_void_p()
    rc = native_lib.mrtx_create(C.byref(_lib.MrtxConfig(0, 16, 16, 0, 1, 0, 0)), C.byref(c))
    assert rc in (0, -2) and c.value
    yield c
    native_lib.mrtx_destroy(c)


def year(step_h, n):
    t0 = datetime(2025, 1, 1, tzinfo=timezone.utc)
    return [t0 + timedelta(hours=step_h * k) for k in range(n)]


def model(panel=0, normal=(0.0, 0.0, 1.0), cpw=0, cap=100, ini=50):
    md = _lib.MrtxPowerModel()
    md.panel, md.cpw_log2, md.capacity, md.initial = panel, cpw, cap, ini
    md.normal_enu[:] = normal
    return md


def test_arguments_are_checked_before_any_device_call(native_lib, ctx):
    f = native_lib.mrtx_power_budget
    pts = np.array([[10.0, 20.0], [-5.0, 190.0]])
    hz = np.zeros((2, 8), np.float32)
    eps = E.sun_epochs(year(24, 5), OBS)
    gen, load = np.full(5, 120.0), np.full(5, 30.0)
    out = np.empty((2, 8), np.int64)
    O, H = out.ctypes.data, hz.ctypes.data

    def call(p=pts, n=2, n_az=8, dh=None, hh=H, e=eps, g=gen, l=load, m=5, md=model(), mode=1, dev=None, host=O, c=ctx):
        ptr = lambda a: None if a is None else a.ctypes.data     # noqa: E731
        return f(c, ptr(p), n, n_az, dh, hh, ptr(e), ptr(g), ptr(l), m, None if md is None else C.byref(md), mode, dev, host, None)

    def refused(word, **kw):
        assert call(**kw) == E_INVALID, kw
        msg = native_lib.mrtx_last_error(ctx)
        assert word in msg, (kw, msg)
    assert call(c=None) == E_INVALID
    for kw in (dict(p=None), dict(e=None)):
        refused(b"null", **kw)
    for kw in (dict(g=None), dict(l=None), dict(md=None)):
        refused(b"null", **kw)
    for kw in (dict(n=0), dict(m=0)):
        refused(b">= 1", **kw)
    refused(b"2^24", m=(1 << 24) + 1)
    for n_az in (6, 2, 8192):
        refused(b"n_az", n_az=n_az)
    for mode in (-1, 2):
        refused(b"mode", mode=mode)
    # both or neither of the horizon sources, and of the output
    for kw in (dict(hh=None), dict(dh=H)):
        refused(b"horizon", **kw)
    for kw in (dict(host=None), dict(dev=O)):
        refused(b"dev_out", **kw)
    refused(b"aligned", host=None, dev=8)
    refused(b"2^31", mode=0, n=1 << 15, m=(1 << 16) + 1)
    for panel in (-1, 3):
        refused(b"panel", md=model(panel=panel))
    for normal in ((0.0, 0.0, 0.0), (NAN, 0.0, 1.0), (INF, 0.0, 0.0)):
        refused(b"normal", md=model(panel=1, normal=normal))
    for cpw in (-21, 21):
        refused(b"cpw_log2", md=model(cpw=cpw))
    for cap in (-1, (1 << 52) + 1):
        refused(b"capacity", md=model(cap=cap, ini=0))
    for ini in (-1, 101):
        refused(b"initial", md=model(ini=ini))
    for name, word in (("g", b"gen_w[3]"), ("l", b"load_w[3]")):
        for bad in (NAN, INF, -INF, -1e-9, float(1 << 28) * 1.001):
            t = (gen if name == "g" else load).copy()
            t[3] = bad
            refused(word, **{name: t})
        t = (gen if name == "g" else load).copy()
        t[3] = 300.0                                            # 300 W at 2^20 counts per watt passes 2^28
        refused(word, md=model(cpw=20), **{name: t})
    bad_hz = hz.copy()
    bad_hz[1, 3] = NAN
    refused(b"horizon", hh=bad_hz.ctypes.data)
    bad_ep = eps.copy()
    bad_ep[2, 3] = -1.0
    refused(b"epoch", e=bad_ep)
    bad_pts = pts.copy()
    bad_pts[1] = [90.5, 0.0]
    assert call(p=bad_pts) == E_INVALID
    # good arguments: the missing DEM is next.  A zero normal is only read for a FIXED panel; 2^28 counts exactly are allowed
    top = gen.copy()
    top[0] = float(1 << 28)
    for kw in (dict(), dict(mode=0, host=np.empty((2, 5), np.int32).ctypes.data), dict(md=model(panel=2, normal=(0.0, 0.0, 0.0))),
               dict(md=model(panel=1, normal=(0.0, 3.0, 4.0))), dict(md=model(cap=1 << 52, ini=1 << 52)), dict(md=model(cap=0, ini=0)),
               dict(g=top), dict(md=model(cpw=-20)), dict(m=1), dict(g=np.zeros(5), l=np.zeros(5), md=model(cpw=20))):
        assert call(**kw) == E_STATE, kw
        assert b"displacement" in native_lib.mrtx_last_error(ctx)


# ---- the Python layer --------------------------------------------------------------------------------------------------------
def test_power_scale_picks_the_largest_exponent():
    two28 = np.float32(1 << 28)
    for gen, load in (([120.0, 80.5], 30.0), ([0.0], [1e-3]), ([1.0], [0.0]), ([256.0], [1.0]), ([255.99999], [0.0]), ([5e7], [2.0]),
                      ([float(1 << 28)], [0.0]), ([2.0e14], [1.0]), ([2.0 ** 48], [0.0])):
        e = MoonRT.power_scale(gen, load)
        top = max(np.float32(np.max(gen)), np.float32(np.max(load)))
        assert -20 <= e <= 20
        assert top * np.float32(2.0 ** e) <= two28, (gen, load, e)
        assert e == 20 or top * np.float32(2.0 ** (e + 1)) > two28, (gen, load, e)
        assert pm.quantise(gen, e).max() <= 1 << 28
    assert MoonRT.power_scale([256.0], [1.0]) == 20 and MoonRT.power_scale([256.5], [1.0]) == 19
    assert MoonRT.power_scale([0.0, 0.0], 0.0) == 20
    with pytest.raises(ValueError):
        MoonRT.power_scale([2.0 ** 48 * 1.01], [0.0])
    with pytest.raises(ValueError):
        MoonRT.power_scale([INF], [0.0])


def test_counts_and_watt_hours():
    # one count at cpw_log2 = 4 and 30-minute epochs is 1/16 W x 0.5 h
    assert sunlight.counts_to_wh(1, 4, 30) == 1.0 / 32.0
    assert sunlight.counts_to_wh(np.array([0, 16, -48], np.int64), 4, 60).tolist() == [0.0, 1.0, -3.0]
    assert sunlight.wh_to_counts(3.0, 4, 60) == 48 and sunlight.wh_to_counts(3.0, 4, 30) == 96
    assert sunlight.wh_to_counts(0.0, 20, 60) == 0 and sunlight.wh_to_counts(1e3, -2, 60) == 250
    for wh in (0.5, 1234.5678, 9.9e5):
        c = sunlight.wh_to_counts(wh, 10, 60)
        assert abs(sunlight.counts_to_wh(c, 10, 60) - wh) <= 0.5 * 2.0 ** -10
    # the host's float32 rounding of a table of watts: ties to even, like the kernel's rintf
    assert pm.quantise([0.5, 1.5, 2.5, 2.4999, 3.0], 0).tolist() == [0, 2, 2, 2, 3]
    assert pm.quantise([0.1], 20).tolist() == [int(np.rint(np.float32(0.1) * np.float32(2.0 ** 20)))]


class FakeBuffer:
    made = []

    def __init__(self, nbytes, device=0):
        self.nbytes, self.ptr, self.freed = int(nbytes), 1 << 20, False
        FakeBuffer.made.append(self)

    def free(self):
        self.freed = True


class FakeLib:
    def __init__(self):
        self.calls = []

    def mrtx_horizon_points(self, ctx, pts, n, n_az, n_bis, dev, host, st):
        self.calls.append(("points", n))
        return 0

    def mrtx_horizon_raised(self, ctx, pts, hts, radius_m, n, n_az, n_bis, dev, host, st):
        h = np.ctypeslib.as_array(C.cast(hts, C.POINTER(C.c_double)), (n,)).copy()
        self.calls.append(("raised", n, h.tolist()))
        return 0

    def mrtx_power_budget(self, ctx, pts, n, n_az, dh, hh, eps, gen, load, m, md, mode, dev, host, st):
        md = md._obj
        g = np.ctypeslib.as_array(C.cast(gen, C.POINTER(C.c_double)), (m,)).copy()
        l = np.ctypeslib.as_array(C.cast(load, C.POINTER(C.c_double)), (m,)).copy()
        self.calls.append(("power", n, n_az, m, mode, md.panel, list(md.normal_enu), md.cpw_log2, md.capacity, md.initial,
                           dh is not None, hh is not None, g, l))
        if mode == 1:
            vals = np.tile(np.array([64, -32, 16, 2, 5, 8, 3, 4], np.int64), (n, 1))
        else:
            vals = np.full((n, m), 7, np.int32)
        C.memmove(host, vals.ctypes.data, vals.nbytes)
        st._obj.launches = 1
        return 0

    def mrtx_get_config(self, ctx, cfg):
        return 0


def fake_rt(monkeypatch):
    FakeBuffer.made.clear()
    monkeypatch.setattr(rmod, "DeviceBuffer", FakeBuffer)
    rt = MoonRT.__new__(MoonRT)
    rt._lib = FakeLib()
    rt._ctx = None
    return rt


def test_power_budget_passes_its_model_and_chunks(monkeypatch):
    rt = fake_rt(monkeypatch)
    la, lo = np.linspace(-5, 5, 5), np.linspace(0, 4, 5)
    eps = E.sun_epochs(year(24, 3), OBS)
    hz = np.zeros((5, 8), np.float32)
    st = {}
    got = rt.power_budget(la, lo, hz, eps, [100.0, 120.0, 90.0], 30.0, capacity=500, stats=st, chunk_bytes=2 * (8 + 16) * 4)
    assert got.shape == (5, 8) and got.dtype == np.int64 and got[4].tolist() == [64, -32, 16, 2, 5, 8, 3, 4]
    calls = rt._lib.calls
    assert [c[1] for c in calls] == [2, 2, 1] and st["launches"] == 3 and len(MoonRT.POWER_COLUMNS) == 8
    # TRACK, the scale of 120 W (2^21 x 120 <= 2^28 < 2^22 x 120), full at the start, host horizons, the load on every date
    assert all(c[2:12] == (8, 3, 1, 0, [0.0, 0.0, 1.0], 20, 500, 500, False, True) for c in calls)
    assert calls[0][12].tolist() == [100.0, 120.0, 90.0] and calls[0][13].tolist() == [30.0] * 3
    calls.clear()
    full = rt.power_budget(la, lo, FakeBuffer(5 * 8 * 4), eps, [100.0] * 3, [1.0, 2.0, 3.0], panel="fixed", normal_enu=(0, 3, 4),
                           cpw_log2=-3, capacity=9, initial=2, mode="full", n_az=8)
    assert full.shape == (5, 3) and full.dtype == np.int32 and (full == 7).all()
    assert calls[0][1:12] == (5, 8, 3, 0, 1, [0.0, 3.0, 4.0], -3, 9, 2, True, False)
    calls.clear()
    rt.power_budget(la, lo, hz, eps, 1.0, 1.0, panel="azimuth")
    assert calls[0][5] == 2 and calls[0][8:10] == (0, 0)
    for kw in (dict(panel="sideways"), dict(mode="both"), dict(panel="fixed"), dict(normal_enu=(0, 0, 1))):
        with pytest.raises(ValueError):
            rt.power_budget(la, lo, hz, eps, 1.0, 1.0, **kw)
    with pytest.raises(ValueError):
        rt.power_budget(la, lo, hz, eps, [1.0, 2.0], 1.0)
    with pytest.raises(ValueError):
        rt.power_budget(la, lo, FakeBuffer(5 * 8 * 4), eps, 1.0, 1.0)


def test_sunlight_power_budget_streams_chunks(monkeypatch):
    rt = fake_rt(monkeypatch)
    la, lo = np.linspace(-88, -84, 5), np.linspace(0, 4, 5)
    t0 = datetime(2025, 1, 1, tzinfo=timezone.utc)
    r = sunlight.power_budget(rt, la, lo, t0, 0.25, step_min=30, height_m=2.0, area_m2=2.0, efficiency=0.25, load_w=40.0,
                              panel="azimuth", capacity_wh=100.0, n_az=8, n_bis=5, observer=OBS, chunk=2)
    assert len(r.times) == 12 and r.times[1] - r.times[0] == timedelta(minutes=30)
    calls = rt._lib.calls
    assert [c[0] for c in calls] == ["raised", "power"] * 3 and [c[1] for c in calls] == [2, 2, 2, 2, 1, 1]
    assert all(c[2] == [2.0] * c[1] for c in calls if c[0] == "raised")
    power = [c for c in calls if c[0] == "power"]
    flux = E.sun_flux(r.times)
    assert np.array_equal(power[0][12], flux * 0.5) and power[0][13].tolist() == [40.0] * 12
    cpw = MoonRT.power_scale(flux * 0.5, 40.0)
    assert r.cpw_log2 == cpw == 18                               # about 700 W: 2^18 x 700 <= 2^28 < 2^19 x 700
    cap = sunlight.wh_to_counts(100.0, cpw, 30)
    assert cap == 100 * 2 * 2 ** 18
    assert all(c[2:12] == (8, 12, 1, 2, [0.0, 0.0, 1.0], cpw, cap, cap, True, False) for c in power)
    assert len(FakeBuffer.made) == 1 and FakeBuffer.made[0].freed and FakeBuffer.made[0].nbytes == 2 * 8 * 4
    # counts to Wh (2^-18 W x 0.5 h each), epochs to hours, the dates as indices
    unit = 2.0 ** -18 * 0.5
    assert r.generated_wh.tolist() == [64 * unit] * 5 and r.net_wh.tolist() == [-32 * unit] * 5
    assert r.storage_wh.tolist() == [16 * unit] * 5 and r.min_charge_wh.tolist() == [8 * unit] * 5
    assert r.deficit_start.tolist() == [2] * 5 and r.deficit_end.tolist() == [5] * 5 and r.deficit_start.dtype == np.int64
    assert r.unmet_h.tolist() == [1.5] * 5 and r.unmet_wh.tolist() == [4 * unit] * 5 and r.stats["launches"] == 3
    # a load per date, a battery that starts empty
    calls.clear()
    sunlight.power_budget(rt, la, lo, t0, 0.25, step_min=30, area_m2=1.0, efficiency=0.3, load_w=np.arange(12.0), capacity_wh=1.0,
                          initial_wh=0.0, n_az=8, observer=OBS)
    power = [c for c in calls if c[0] == "power"]
    assert power[0][13].tolist() == list(range(12)) and power[0][9] == 0 and power[0][8] > 0 and power[0][5] == 0
    assert [c for c in calls if c[0] == "raised"][0][2] == [0.0] * 5
    with pytest.raises(ValueError):
        sunlight.power_budget(rt, la, lo, t0, 0.25, step_min=30, area_m2=1.0, efficiency=0.3, load_w=np.arange(5.0))
    with pytest.raises(ValueError):
        sunlight.power_budget(rt, la, lo[:4], t0, 0.25, area_m2=1.0, efficiency=0.3, load_w=1.0)
