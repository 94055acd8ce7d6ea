"""Sun illumination over many dates without a GPU: argument validation of mrtx_illum_series, the
ephemeris epochs of ephemeris.sun_epochs, and the event search of sunlight.terrain_sun_events over a fake series."""
import ctypes as C
from datetime import datetime, timedelta, timezone

import numpy as np
import pytest

import illum_model as im
from moonrtx_amd import _lib
from moonrtx_amd import ephemeris as E
from moonrtx_amd import sunlight

E_INVALID, E_STATE = -1, -3


@pytest.fixture
def ctx(native_lib):
    """A context handle; without a GPU mrtx_create stops at its first HIP call but hands the context out."""
    c = C.c_void_p()
    rc = native_lib.mrtx_create(C.byref(_lib.MrtxConfig(0, 16, 16, 0, 1, 0, 0)), C.byref(c))
    assert rc in (0, -2) and c.value
    yield c
    native_lib.mrtx_destroy(c)


def good_epoch():
    s = E.scene_from_ephemeris(E.calculate_moon_ephemeris(datetime(2025, 3, 7, 21, 0, tzinfo=timezone.utc), False,
                                                          E.Observer(52.2, 21.0, 0.0)), 16, 16)
    return E.epoch_of_scene(s)


def test_epoch_struct_matches_the_array_layout():
    assert C.sizeof(_lib.MrtxIllumEpoch) == 112 == 14 * 8
    row = np.arange(14, dtype=np.float64)
    e = _lib.MrtxIllumEpoch.from_buffer_copy(row.tobytes())
    assert list(e.light_pos) == [0, 1, 2] and (e.light_radius, e.light_radiance) == (3, 4)
    assert list(e.center) == [5, 6, 7] and list(e.u) == [8, 9, 10] and list(e.v) == [11, 12, 13]


def test_series_arguments_are_checked_before_any_device_call(native_lib, ctx):
    f = native_lib.mrtx_illum_series
    pts = np.array([[10.0, 20.0], [-5.0, 190.0], [0.0, 0.0]])
    ep = np.ascontiguousarray(np.stack([good_epoch()] * 4))
    out = np.empty((3, 4, 4), np.float32)
    O = out.ctypes.data

    def call(p=pts, n=3, e=None, m=4, first=None, count=4, n_sun=16, dev=None, host=O, c=ctx):
        e = ep if e is None else e
        fp = None if first is None else np.ascontiguousarray(first, np.int32).ctypes.data
        return f(c, None if p is None else p.ctypes.data, n, None if e is False else e.ctypes.data, m, fp, count, n_sun, dev,
                 host, None)
    # null pointers
    assert call(c=None) == E_INVALID
    assert call(p=None) == E_INVALID
    assert call(e=False) == E_INVALID
    assert call(host=None) == E_INVALID
    assert native_lib.mrtx_last_error(ctx)
    # sizes
    for kw in (dict(n=0), dict(n=-1), dict(m=0), dict(m=-2), dict(count=0), dict(count=-1)):
        assert call(**kw) == E_INVALID, kw
    # windows outside [0, n_epochs)
    assert call(count=5) == E_INVALID
    assert call(first=[0, 0, 1], count=4) == E_INVALID
    assert call(first=[-1, 0, 0], count=2) == E_INVALID
    assert call(first=[0, 2, 3], count=2) == E_INVALID
    # n_sun
    for n in (0, -4, 3, 12, 48, 128):
        assert call(n_sun=n) == E_INVALID, n
    # point coordinates
    for bad in ([90.5, 0.0], [-91.0, 0.0], [float("nan"), 0.0], [0.0, float("inf")], [0.0, 2e6]):
        p = pts.copy()
        p[1] = bad
        assert call(p=p) == E_INVALID, bad
    # epochs that mrtx_set_light / mrtx_set_moon_frame refuse
    def with_bad(i, x):
        e = ep.copy()
        e[2, i] = x
        return e
    for i, x in ((0, float("nan")), (2, float("inf")), (3, -1.0), (3, float("inf")), (4, -0.5), (4, float("nan")),
                 (5, float("nan")), (9, float("inf")), (13, float("nan"))):
        assert call(e=with_bad(i, x)) == E_INVALID, (i, x)
    e = ep.copy()
    e[1, 11:14] = 2.0 * e[1, 8:11]                  # v parallel to u
    assert call(e=e) == E_INVALID
    # more than 2^31 outputs (refused before the windows or the tables are read)
    assert call(m=1 << 30, count=1 << 30) == E_INVALID
    # well-formed, but no DEM: a state error (no light or moon frame is needed), still before any device call
    assert call() == E_STATE
    assert b"displacement" in native_lib.mrtx_last_error(ctx)
    assert call(first=[0, 2, 1], count=2, n=3) == E_STATE
    assert call(first=[3, 3, 3], count=1) == E_STATE
    for n in (1, 2, 4, 8, 32, 64):
        assert call(n_sun=n) == E_STATE
    assert call(host=None, dev=O) == E_STATE      # a device buffer alone is an output


def test_sun_epochs_rows_are_the_scene_and_the_subsolar_point():
    obs = E.Observer(-33.9, 18.4, 10)
    times = [datetime(2024, 1, 1, tzinfo=timezone.utc) + timedelta(days=2.61 * k, hours=3 * k) for k in range(16)]
    ep = E.sun_epochs(times, obs)
    assert ep.shape == (16, 14) and ep.dtype == np.float64
    for t, row in zip(times, ep):
        e = E.calculate_moon_ephemeris(t, False, obs)
        s = E.scene_from_ephemeris(e, 16, 16)
        assert row[0:3].tolist() == list(s.light_pos) and row[3] == s.light_radius and row[4] == s.light_radiance
        assert row[5:8].tolist() == list(s.center) and row[8:11].tolist() == list(s.u) and row[11:14].tolist() == list(s.v)
        # the body-frame Sun direction of the row lies at the date's subsolar point
        class S:
            light_pos, center, u, v = row[0:3], row[5:8], row[8:11], row[11:14]
        la, lo = im.subsolar_latlon(S)
        assert abs(la - e.subsolar_lat) < 2e-3 and abs((lo - e.subsolar_lon + 180.0) % 360.0 - 180.0) < 2e-3
    assert E.sun_epochs([], obs).shape == (0, 14)


# ---- terrain_sun_events over a fake series: the epochs carry their date (POSIX seconds in column 0), lit is a function of time
T0 = datetime(2025, 3, 1, tzinfo=timezone.utc)
STEP, REFINE = 10.0, 15
SUB = STEP * 60.0 / (REFINE + 1)          # 37.5 s


def at(minutes):
    return T0.timestamp() + minutes * 60.0


def ramp(t, a, b):
    return np.clip((t - a) / (b - a), 0.0, 1.0)


# point -> lit(t) (t in POSIX seconds) and the expected transitions (kind, time at which the new state begins)
def lit_of(p, t):
    if p == 0:      # rises from dark, full disc, cut, sets: each in a different coarse step
        return np.minimum(ramp(t, at(123.0), at(187.0)), 1.0 - ramp(t, at(611.0), at(707.0)))
    if p == 1:      # already fully lit at the first date: sets only
        return 1.0 - ramp(t, at(302.0), at(340.0))
    if p == 2:      # first light flickers inside one coarse step: on for 60 s, off for 60 s, then on (a point light: 0 / 1)
        a = at(400.0 + 100.0 / 60.0)
        return np.where((t >= a) & (t < a + 60.0) | (t >= a + 120.0), 1.0, 0.0)
    if p == 3:      # lit, shadowed by a ridge, lit again: every transition is reported
        return np.where((t >= at(205.0)) & (t < at(555.0)), 0.0, 1.0)
    return np.zeros_like(t)


EXPECTED = {0: [("first_light", at(123.0)), ("full_disc", at(187.0)), ("disc_cut", at(611.0)), ("last_light", at(707.0))],
            1: [("disc_cut", at(302.0)), ("last_light", at(340.0))],
            2: [("first_light", at(400.0 + 100.0 / 60.0)), ("full_disc", at(400.0 + 100.0 / 60.0))],
            3: [("disc_cut", at(205.0)), ("last_light", at(205.0)), ("first_light", at(555.0)), ("full_disc", at(555.0))]}


class FakeSeries:
    def __init__(self):
        self.calls = []

    def __call__(self, lat, lon, epochs, n_sun=16, first=None, count=None, stats=None):
        pid = np.rint(np.asarray(lat)).astype(int)      # the test's points sit at lat = their index
        m = epochs.shape[0]
        count = m if count is None else count
        starts = np.zeros(len(pid), int) if first is None else np.asarray(first)
        self.calls.append(dict(pid=pid, epochs=epochs.copy(), first=None if first is None else starts.copy(), count=count,
                               n_sun=n_sun))
        out = np.zeros((len(pid), count, 4), np.float32)
        for i, p in enumerate(pid):
            out[i, :, 0] = lit_of(p, epochs[starts[i]:starts[i] + count, 0])
        if isinstance(stats, dict):
            stats["launches"] = stats.get("launches", 0) + 1
        return out


@pytest.fixture
def events(monkeypatch):
    monkeypatch.setattr(E, "sun_epochs", lambda times, observer=None: np.array(
        [[t.timestamp()] + [0.0] * 13 for t in times], np.float64).reshape(-1, 14))
    fake = FakeSeries()
    res = sunlight.terrain_sun_events(None, [0.0, 1.0, 2.0, 3.0], [0.0, 10.0, 20.0, 30.0], T0, 0.5, step_min=STEP, n_sun=4,
                                      refine=REFINE, observer=E.Observer(52.2, 21.0, 0.0), series=fake)
    return res, fake


def test_events_kinds_and_brackets(events):
    res, _ = events
    assert len(res.times) == 73 and res.times[-1] == T0 + timedelta(hours=12)
    assert {e.kind for e in res.events} == {"first_light", "full_disc", "disc_cut", "last_light"}
    for p, want in EXPECTED.items():
        got = [e for e in res.events if e.point == p]
        assert sorted((e.kind, e.t_hi.timestamp()) for e in got) == sorted(
            (k, T0.timestamp() + np.ceil((t - T0.timestamp()) / SUB) * SUB) for k, t in want), p
        for e in got:
            assert (e.t_hi - e.t_lo).total_seconds() == SUB
            t_new = dict(want)[e.kind] if sum(k == e.kind for k, _ in want) == 1 else None
            if t_new is not None:
                assert e.t_lo.timestamp() < t_new <= e.t_hi.timestamp()
            # the old state at t_lo, the new one at t_hi
            lo, hi = lit_of(p, np.array([e.t_lo.timestamp(), e.t_hi.timestamp()]))
            if e.kind in ("first_light", "last_light"):
                assert (lo > 0) != (hi > 0) and (hi > 0) == (e.kind == "first_light")
            else:
                assert (lo == 1) != (hi == 1) and (hi == 1) == (e.kind == "full_disc")
            assert np.isfinite(e.sun_alt_sphere) and -90 <= e.sun_alt_sphere <= 90 and -90 <= e.moon_alt <= 90


def test_a_point_lit_at_the_first_date_has_no_first_light(events):
    res, _ = events
    kinds = [e.kind for e in res.events if e.point == 1]
    assert "first_light" not in kinds and "full_disc" not in kinds and kinds == ["disc_cut", "last_light"]


def test_flicker_is_flagged(events):
    res, _ = events
    for e in res.events:
        assert e.flicker == (e.point == 2), e
    p2 = [e for e in res.events if e.point == 2]
    assert len(p2) == 2 and all(e.flicker for e in p2)


def test_the_refinement_is_one_call_with_one_window_per_transition(events):
    res, fake = events
    assert len(fake.calls) == 2
    coarse, fine = fake.calls
    assert coarse["first"] is None and coarse["count"] == 73 and coarse["n_sun"] == 4
    assert fine["count"] == REFINE and fine["n_sun"] == 4
    assert len(fine["first"]) == len(res.events) == sum(len(v) for v in EXPECTED.values())
    # each window holds exactly the REFINE interior dates of its event's coarse step, for that event's point
    windows = sorted((int(p), float(fine["epochs"][f, 0])) for p, f in zip(fine["pid"], fine["first"]))
    want = sorted((e.point, e.t_hi.timestamp()) for e in res.events)
    for (p, t0), f in zip(zip(fine["pid"], fine["epochs"][fine["first"], 0]), fine["first"]):
        w = fine["epochs"][f:f + REFINE, 0]
        k = np.floor((t0 - T0.timestamp()) / (STEP * 60.0))
        assert np.array_equal(w, T0.timestamp() + k * STEP * 60.0 + (np.arange(REFINE) + 1) * SUB)
    assert [p for p, _ in windows] == [p for p, _ in want]
    # each coarse step's sub-dates are computed once
    assert fine["epochs"].shape[0] == REFINE * len({int(np.floor((e.t_lo.timestamp() - T0.timestamp()) / 600.0))
                                                    for e in res.events})


def test_no_transition_no_refinement(monkeypatch):
    monkeypatch.setattr(E, "sun_epochs", lambda times, observer=None: np.array(
        [[t.timestamp()] + [0.0] * 13 for t in times], np.float64).reshape(-1, 14))
    fake = FakeSeries()
    res = sunlight.terrain_sun_events(None, [7.0], [0.0], T0, 0.1, series=fake, observer=E.Observer(0, 0, 0))
    assert res.events == [] and len(fake.calls) == 1 and res.refine == {}
