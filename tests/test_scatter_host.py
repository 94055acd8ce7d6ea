"""Terrain-scattered flux, host side: the view-direction table, the diffuse albedo A_h, the hit
compaction and budget groups, the epoch tables and stage order of surface_temperatures(scatter=K) through injected fakes,
scatter=0 as today's call sequence, and the refusals of the three new entry points.  No GPU needed."""
import ctypes as C
import math
from datetime import datetime, timezone

import numpy as np
import pytest

import scatter_model as sm
from moonrtx_amd import sunlight, thermal
from moonrtx_amd import ephemeris as E
from moonrtx_amd.renderer import MoonRT
from test_thermal_host import E_INVALID, E_STATE, FakeRT, ctx, good_epochs  # noqa: F401 -- ctx is a fixture

OBS = E.Observer(52.2, 21.0, 0.0)


@pytest.mark.parametrize("k", [16, 32, 64, 256, 1024])
def test_view_direction_table_is_the_spec(native_lib, k):
    t = MoonRT.view_samples(k)
    assert t.dtype == np.float32 and t.shape == (k, 2)
    assert np.array_equal(t, sm.directions(k))
    assert np.all((t[:, 0] > 0) & (t[:, 0] < 1) & (t[:, 1] >= 0) & (t[:, 1] < 1))


@pytest.mark.parametrize("k", [0, 8, 48, 2048, -16])
def test_view_direction_table_refuses_a_bad_k(native_lib, k):
    with pytest.raises(ValueError):
        MoonRT.view_samples(k)


def test_diffuse_albedo_is_the_cosine_weighted_mean():
    """A_h against a midpoint rule on 200 000 cells in theta (error ~1e-11) and against the flat limit: A_h lies between A(0)
    and A(90 deg), above A0."""
    n = 200000
    th = (np.arange(n) + 0.5) * (math.pi / 2 / n)
    want = float(np.sum(thermal.albedo(np.degrees(th)) * 2 * np.sin(th) * np.cos(th)) * (math.pi / 2 / n))
    a_h = thermal.albedo_hemispherical()
    assert abs(a_h - want) < 1e-9, (a_h, want)
    assert thermal.ALBEDO[0] < a_h < thermal.albedo(90.0)
    assert math.isfinite(a_h) and abs(thermal.albedo_hemispherical(16) - a_h) < 1e-12


def test_compaction_numbers_the_hits_point_major():
    hits = np.full((3, 4, 2), np.nan, np.float32)
    hits[0, 1] = (1.0, 2.0)
    hits[2, 0] = (3.0, 4.0)
    hits[2, 3] = (5.0, 6.0)
    index, lat, lon = sunlight.compact_hits(hits)
    assert index.dtype == np.int32
    assert index.tolist() == [[-1, 0, -1, -1], [-1, -1, -1, -1], [1, -1, -1, 2]]
    assert lat.tolist() == [1.0, 3.0, 5.0] and lon.tolist() == [2.0, 4.0, 6.0]


def test_groups_keep_the_device_tables_within_the_budget():
    counts = np.array([3, 0, 5, 1, 7, 2])
    per_hit, per_pt = 8 * 10 + 4 * 16, 4 * 10 + 4 * 16
    budget = 6 * per_hit + 2 * per_pt
    groups = sunlight.scatter_groups(counts, 10, 10, 16, budget)
    assert groups[0][0] == 0 and groups[-1][1] == counts.size
    assert all(a < b for a, b in groups) and all(groups[i][1] == groups[i + 1][0] for i in range(len(groups) - 1))
    for a, b in groups:
        need = int(counts[a:b].sum()) * per_hit + (b - a) * per_pt
        assert need <= budget or b - a == 1, (a, b)
    assert groups == [(0, 2), (2, 4), (4, 5), (5, 6)]
    assert sunlight.scatter_groups(counts, 10, 10, 16, 1 << 40) == [(0, 6)]
    # a group's EXITANCE fits one call: at most 2^30 (M_vis, M_ir) pairs
    big = (1 << 30) // 8760
    assert sunlight.scatter_groups([big, 1, big - 1, 0], 8760, 8760, 16, 1 << 50) == [(0, 1), (1, 4)]


class FakeBuffer:
    def __init__(self, nbytes, log):
        self.nbytes, self.data, self.freed = int(nbytes), None, False
        log.append(self)

    def download(self, dtype, shape):
        return np.asarray(self.data, dtype).reshape(shape)

    def free(self):
        self.freed = True


class FakeScatterRT:
    """The device calls of the scatter path on the host: flat horizons; point p sees hits_per[p] terrain rays of K; a hit's
    EXITANCE is (epoch index, 1) per epoch; the gather is the model's; the points' column reports (n, m, max extra flux,
    n_spin)."""
    thermal_grid = staticmethod(MoonRT.thermal_grid)
    horizon_azimuths = staticmethod(MoonRT.horizon_azimuths)
    view_samples = staticmethod(MoonRT.view_samples)

    def __init__(self, hits_per):
        self.hits_per = hits_per
        self.calls = []

    def horizon(self, la, lo, n_az=256, n_bis=14, stats=None, out=None):
        self.calls.append(("horizon", la.size))
        out.data = np.zeros((la.size, n_az), np.float32)
        return out

    def view_hits(self, la, lo, k=64, stats=None):
        self.calls.append(("view_hits", la.size))
        hits = np.full((la.size, k, 2), np.nan, np.float32)
        for p in range(la.size):
            n = self.hits_per[int(round(la[p]))]
            hits[p, :n, 0] = la[p] + 0.25
            hits[p, :n, 1] = lo[p]
        return hits, (~np.isnan(hits[..., 0])).mean(1).astype(np.float32)

    def surface_temperature_scatter(self, la, lo, hz, ep, fl, model=None, mode="summary", extra_flux=None, stats=None,
                                    n_az=None, out=None):
        m = ep.shape[0]
        self.calls.append(("columns", mode, la.size, m, int(model.n_spin), ep.copy(), fl.copy(), extra_flux is not None))
        assert hz.data.shape == (la.size, n_az)
        if mode == "exitance":
            rec = m - int(model.n_spin)
            ex = np.zeros((la.size, rec, 2), np.float32)
            ex[..., 0] = np.arange(rec, dtype=np.float32)[None, :]
            ex[..., 1] = 1.0
            out.data = ex
            return out
        assert mode == "summary" and out is None
        x = 0.0 if extra_flux is None else float(np.max(extra_flux.data))
        return np.tile(np.array([[la.size, m, x, model.n_spin]], np.float32), (la.size, 1))

    def scatter_flux(self, index, exitance, albedo_h, emissivity, n_hits=None, m=None, out=None, stats=None):
        self.calls.append(("gather", index.shape, n_hits, m, albedo_h, emissivity))
        assert index.max() < n_hits and exitance.data.shape == (n_hits, m, 2)
        out.data = sm.gather(index, exitance.data, albedo_h, emissivity)
        return out


def test_scatter_driver_epoch_tables_groups_and_stages():
    t0 = datetime(2025, 6, 1, tzinfo=timezone.utc)
    hits_per = {0: 2, 1: 0, 2: 16, 3: 1, 4: 0}
    rt = FakeScatterRT(hits_per)
    bufs = []
    la = np.arange(5, dtype=np.float64)
    lo = np.zeros(5)
    K, n_az = 16, 8
    block = int(round(29.530589 * 24 / 2))
    m_rec = 12
    m_t = block + m_rec
    budget = 3 * (8 * m_t + 4 * n_az) + 2 * (4 * m_t + 4 * n_az)      # groups of at most 3 hits or so
    r = sunlight.surface_temperatures(rt, la, lo, t0, 1.0, step_min=120, spinup_lunations=1, n_az=n_az, chunk=4,
                                      observer=OBS, scatter=K, budget_bytes=budget, q_sec_mean=True,
                                      alloc=lambda n: FakeBuffer(n, bufs))
    # chunks of 4 then 1 points for the view hits; every group: horizons, [hit horizons, hit columns, gather,] columns
    kinds = [c[0] if c[0] != "columns" else "columns:" + c[1] for c in rt.calls]
    assert kinds[0] == "view_hits" and rt.calls[0][1] == 4
    assert kinds.count("view_hits") == 2 and kinds.count("columns:summary") == 4     # groups (0, 2), (2, 3), (3, 4), (4, 5)
    assert kinds.count("gather") == 3 and kinds.count("columns:exitance") == 3      # the groups that see terrain
    assert all(b.freed for b in bufs)
    # the epoch tables: the hits' [own spin-up | the points' spin-up | recorded], the points' [spin-up | recorded]
    ex_calls = [c for c in rt.calls if c[0] == "columns" and c[1] == "exitance"]
    pt_calls = [c for c in rt.calls if c[0] == "columns" and c[1] == "summary"]
    for c in ex_calls:
        assert c[3] == 2 * block + m_rec and c[4] == block
    for c in pt_calls:
        assert c[3] == m_t and c[4] == block
    assert np.array_equal(ex_calls[0][5][block:], pt_calls[0][5]) and np.array_equal(ex_calls[0][6][block:], pt_calls[0][6])
    times = [t0 + k * (r.times[1] - r.times[0]) for k in range(m_rec)]
    assert r.times == times and len(r.times) == m_rec
    want_ep = E.sun_epochs([t0 + (k - 2 * block) * (times[1] - times[0]) for k in range(2 * block + m_rec)], OBS)
    assert np.array_equal(ex_calls[0][5], want_ep)
    # a group that sees nothing runs with no extra flux; the others with the gathered one
    assert [c[2] for c in pt_calls] == [2, 1, 1, 1] and [c[7] for c in pt_calls] == [True, True, True, False]
    assert r.stats["scatter_hits"] == sum(hits_per.values())
    assert np.allclose(r.stats["view_factor"], np.array([2, 0, 16, 1, 0]) / K)
    # Q_sec of the fake: per terrain ray (1 - A_h) x epoch index + eps, over K; its max is at the last epoch
    a_h = thermal.albedo_hemispherical()
    peak = {p: n / K * ((1 - a_h) * (m_t - 1) + thermal.EMISSIVITY) for p, n in hits_per.items()}
    for p, want in zip(range(5), [peak[0], peak[0], peak[2], peak[3], 0.0]):       # the group's largest Q_sec
        assert abs(r.t_mean[p] - want) < 1e-3 * max(want, 1.0), (p, r.t_mean[p], want)
    for p, n in hits_per.items():
        qm = n / K * ((1 - a_h) * (block + (m_rec - 1) / 2) + thermal.EMISSIVITY) if n else 0.0
        assert abs(r.stats["q_sec_mean"][p] - qm) < 1e-3 * max(qm, 1.0)
    assert set(r.stats["stage_s"]) == {"view_hits", "compact", "horizons", "hit_horizons", "hit_columns", "gather", "columns"}
    # the gather got the budget's groups: no group but a single point holds more than the budget
    for c in rt.calls:
        if c[0] == "gather":
            assert c[2] <= 3 or c[1][0] == 1


def test_scatter_zero_is_todays_call_sequence():
    t0 = datetime(2025, 6, 1, tzinfo=timezone.utc)
    la, lo = np.linspace(-89.0, -80.0, 5), np.linspace(0.0, 60.0, 5)
    runs = []
    for kw in ({}, {"scatter": 0}):
        rt = FakeRT()
        r = sunlight.surface_temperatures(rt, la, lo, t0, 1.0, step_min=120, spinup_lunations=1, n_az=16, chunk=2,
                                          observer=OBS, thermal=rt.thermal, **kw)
        runs.append((rt.calls, r))
    (c0, r0), (c1, r1) = runs
    assert len(c0) == len(c1) == 3
    for a, b in zip(c0, c1):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert all(np.array_equal(x, y) for x, y in zip(r0[:4], r1[:4])) and r0.times == r1.times and r0.stats == r1.stats


def test_scatter_arguments_are_checked_before_any_device_call(native_lib, ctx):
    scatter_refusals(native_lib, ctx, E_STATE)


def scatter_refusals(native_lib, ctx, ok):
    """view_hits: a bad K; scatter_flux: an index outside the hit list, a non-finite or out-of-range A_h, a bad emissivity, a
    short exitance table; thermal_scatter: a bad mode, a short, negative or non-finite extra table.  `ok` is the code a good
    call that needs a DEM reaches (E_STATE without one, 0 with one); the gather needs none.  A host extra table whose largest
    entry takes the radiative equilibrium past 450 K is refused as well."""
    pts = np.array([[10.0, 20.0], [-89.5, 0.0]])
    vh = native_lib.mrtx_view_hits
    out = np.empty(2 * (2 * 64 + 1), np.float32)
    for k in (0, 8, 48, 2048):
        assert vh(ctx, pts.ctypes.data, 2, k, None, out.ctypes.data, None) == E_INVALID, k
    assert vh(ctx, pts.ctypes.data, 0, 64, None, out.ctypes.data, None) == E_INVALID
    assert vh(ctx, pts.ctypes.data, 2, 64, None, None, None) == E_INVALID
    assert vh(ctx, pts.ctypes.data, 2, 64, None, out.ctypes.data, None) == ok
    assert ok == 0 or b"displacement" in native_lib.mrtx_last_error(ctx)

    sf = native_lib.mrtx_scatter_flux
    m, n_hits = 8, 3
    ex = np.ones((n_hits, m, 2), np.float32)
    q = np.empty((2, m), np.float32)

    def gather(idx=None, a_h=0.2, eps=0.95, length=ex.size, host=ex, k=16):
        ix = np.full((2, k), -1, np.int32) if idx is None else idx
        return sf(ctx, ix.ctypes.data, 2, k, None, None if host is None else host.ctypes.data, length, n_hits, m, a_h, eps,
                  None, q.ctypes.data, None)
    bad = np.full((2, 16), -1, np.int32)
    bad[1, 5] = n_hits
    assert gather(bad) == E_INVALID and b"outside the hit list" in native_lib.mrtx_last_error(ctx)
    bad[1, 5] = -2
    assert gather(bad) == E_INVALID
    for a_h in (float("nan"), float("inf"), -0.1, 1.0):
        assert gather(a_h=a_h) == E_INVALID, a_h
    for eps in (0.0, 1.5, float("nan")):
        assert gather(eps=eps) == E_INVALID, eps
    assert gather(length=ex.size - 1) == E_INVALID
    assert gather(host=None) == E_INVALID
    assert gather(k=24) == E_INVALID
    neg = ex.copy()
    neg[1, 2, 0] = -1.0
    assert gather(host=neg) == E_INVALID
    assert gather() != E_INVALID and (ok != 0 or gather() == 0)

    ts = native_lib.mrtx_thermal_scatter
    hz = np.zeros((2, 16), np.float32)
    ep = good_epochs(m)
    fl = np.full(m, 1361.0)
    md = MoonRT.thermal_grid(3600.0, 1, 1)
    md.n_spin, md.block, md.n_reset = 2, 1, 1
    res = np.empty((2, m, 2), np.float32)

    def col(mode=1, extra=None, length=0):
        return ts(ctx, pts.ctypes.data, 2, 16, None, hz.ctypes.data, ep.ctypes.data, fl.ctypes.data, m, C.byref(md), mode,
                  None, None if extra is None else extra.ctypes.data, length, None, res.ctypes.data, None)
    for mode in (-1, 4, 7):
        assert col(mode) == E_INVALID, mode
    x = np.zeros((2, m), np.float32)
    assert col(extra=x, length=x.size - 1) == E_INVALID and b"extra-flux" in native_lib.mrtx_last_error(ctx)
    for v in (-1.0, float("nan"), float("inf")):
        y = x.copy()
        y[1, 3] = v
        assert col(extra=y, length=y.size) == E_INVALID, v
    # a host table's largest entry joins the 450 K check: 0.88 x 1361 + 1100 W m^-2 is past it, + 900 is not
    hot = x.copy()
    hot[1, 3] = 1100.0
    assert col(extra=hot, length=hot.size) == E_INVALID and b"450 K" in native_lib.mrtx_last_error(ctx)
    hot[1, 3] = 900.0
    assert col(extra=hot, length=hot.size) == ok
    for mode in (0, 1, 2, 3):
        assert col(mode, extra=x, length=x.size) == ok, mode
    assert col(3) == ok
    # mrtx_thermal itself still knows only its three modes
    assert native_lib.mrtx_thermal(ctx, pts.ctypes.data, 2, 16, None, hz.ctypes.data, ep.ctypes.data, fl.ctypes.data, m,
                                   C.byref(md), 3, None, res.ctypes.data, None) == E_INVALID
