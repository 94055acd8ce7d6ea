"""When does the Sun rise on a spot of the real terrain?  Sunrise / sunset times from the Sun illumination series (DESIGN.md
section 3.7): a coarse series over the sampled dates, then one refining series over every transition found.

The reference times these events on the smooth sphere only (astro.py: find_terminator_windows, find_clair_obscur_events,
whose catalogue tunes each window by hand for the relief); here the terrain decides, and each event also reports the
sphere's Sun altitude at its time -- the number that catalogue tunes."""
import math
from datetime import timedelta
from typing import NamedTuple

import numpy as np

from . import ephemeris

# (kind on a rise of the state, kind on a fall, the state of a (point, date) from its float4)
_STATES = (("first_light", "last_light", lambda o: o[..., 0] > 0.0),
           ("full_disc", "disc_cut", lambda o: o[..., 0] == 1.0))


class SunEvent(NamedTuple):
    point: int            # index into the point list
    kind: str             # first_light (0 -> > 0), full_disc (< 1 -> 1), disc_cut (1 -> < 1), last_light (> 0 -> 0)
    t_lo: object          # the last refined date in the old state before the first one in the new state
    t_hi: object          # that first new-state date
    flicker: bool         # the refined dates change state more than once inside the coarse step
    sun_alt_sphere: float  # the smooth sphere's Sun altitude at the point at (t_lo + t_hi) / 2, degrees
    moon_alt: float       # the observer's Moon altitude at (t_lo + t_hi) / 2, degrees


class SunEvents(NamedTuple):
    events: list          # SunEvent, ordered by point, then time
    times: list           # the coarse dates
    coarse: dict          # counters and kernel time of the coarse series
    refine: dict          # the same for the refining series (empty when nothing changed state)


def terrain_sun_events(rt, lat, lon, start, days, step_min=10, n_sun=16, refine=15, observer=None, series=None):
    """Every transition of `lit > 0` and of `lit == 1` at the points (lat, lon in degrees) from `start` (timezone-aware) over
    `days`, sampled every `step_min` minutes, each bracketed to step_min / (refine + 1).  `rt` is a MoonRT with a DEM;
    `series` replaces rt.illumination_series (same signature).  Returns SunEvents."""
    series = rt.illumination_series if series is None else series
    la = np.atleast_1d(np.asarray(lat, np.float64)).ravel()
    lo = np.atleast_1d(np.asarray(lon, np.float64)).ravel()
    if la.shape != lo.shape:
        raise ValueError("lat and lon must have the same number of points")
    refine = int(refine)
    if refine < 1:
        raise ValueError("refine must be >= 1")
    step = timedelta(minutes=float(step_min))
    m = int(round(float(days) * 1440.0 / float(step_min))) + 1
    times = [start + k * step for k in range(m)]
    coarse_st, refine_st = {}, {}
    out = series(la, lo, ephemeris.sun_epochs(times, observer), n_sun=n_sun, stats=coarse_st)
    # transitions between consecutive coarse dates: (point, k, state index, rising)
    found = []
    for si, (_, _, state) in enumerate(_STATES):
        s = state(out)
        p, k = np.nonzero(s[:, 1:] != s[:, :-1])
        found += [(int(a), int(b), si, not bool(s[a, b])) for a, b in zip(p, k)]
    found.sort(key=lambda x: (x[0], x[1], x[2]))
    if not found:
        return SunEvents([], times, coarse_st, refine_st)
    # refinement: `refine` interior dates per coarse step that holds a transition, computed once per step; one window each
    sub = [(j + 1) / (refine + 1) for j in range(refine)]
    steps = sorted({k for _, k, _, _ in found})
    at = {k: i * refine for i, k in enumerate(steps)}
    sub_times = [times[k] + f * step for k in steps for f in sub]
    first = np.array([at[k] for _, k, _, _ in found], np.int32)
    pts = np.array([p for p, _, _, _ in found])
    fine = series(la[pts], lo[pts], ephemeris.sun_epochs(sub_times, observer), n_sun=n_sun, first=first, count=refine,
                  stats=refine_st)
    events = []
    for i, (p, k, si, rising) in enumerate(found):
        rise, fall, state = _STATES[si]
        seq = np.concatenate([state(out[p, k:k + 1]), state(fine[i]), state(out[p, k + 1:k + 2])])
        dates = [times[k]] + [times[k] + f * step for f in sub] + [times[k + 1]]
        j = int(np.argmax(seq == rising))             # the first date in the new state (the last one is)
        t_lo, t_hi = dates[j - 1], dates[j]
        mid = t_lo + (t_hi - t_lo) / 2
        e = ephemeris.calculate_moon_ephemeris(mid, False, observer)
        events.append(SunEvent(p, rise if rising else fall, t_lo, t_hi, int((seq[1:] != seq[:-1]).sum()) > 1,
                               float(ephemeris.sun_altitude_at(e.subsolar_lat, e.subsolar_lon, la[p], lo[p])), float(e.alt)))
    events.sort(key=lambda ev: (ev.point, ev.t_hi, ev.kind))
    return SunEvents(events, times, coarse_st, refine_st)


class IlluminationStatistics(NamedTuple):
    mean_fraction: np.ndarray     # (N,) mean over the dates of the visible share of the Sun's disc
    lit_fraction: np.ndarray      # (N,) share of the dates with any of the disc above the horizon
    full_fraction: np.ndarray     # (N,) share of the dates with all of the disc above the horizon
    longest_dark_h: np.ndarray    # (N,) longest run of consecutive dates with none of the disc up, in hours (run x step)
    times: list                   # the dates used
    stats: dict                   # summed counters and kernel times of the horizon and the Sun calls


def _heights(height_m, radius_m, n):
    """kw(a, b): the keywords MoonRT.horizon takes for points [a, b) of n with mast tops height_m (None: the ground-only call;
    one height, or one per point) -- section 3.15."""
    if height_m is None:
        return lambda a, b: {}
    h = np.asarray(height_m, np.float64)
    h = np.full(n, float(h)) if h.ndim == 0 else h.ravel()
    if h.size != n:
        raise ValueError("height_m must be one height or one per point")
    return lambda a, b: {"height_m": h[a:b], "radius_m": radius_m}


def illumination_statistics(rt, lat, lon, start, days, step_min=60, n_az=256, n_bis=14, observer=None, chunk=65536,
                            height_m=None, radius_m=1737400.0):
    """Long-term Sun statistics of the points (lat, lon in degrees) from `start` (timezone-aware) over `days` at `step_min`
    minutes (DESIGN.md sections 3.8 and 3.9): each point's horizon is computed once (MoonRT.horizon, n_az azimuths, n_bis
    probes), then compared with the Sun on every date (MoonRT.horizon_sun, SUMMARY).  Points are streamed `chunk` at a time;
    their horizons stay in a device buffer.  height_m (one height or one per point, metres): the statistics of a mast top
    that high above each point (section 3.15; radius_m = the metres of D = 1).  Returns IlluminationStatistics."""
    from .renderer import DeviceBuffer
    la = np.atleast_1d(np.asarray(lat, np.float64)).ravel()
    lo = np.atleast_1d(np.asarray(lon, np.float64)).ravel()
    if la.shape != lo.shape:
        raise ValueError("lat and lon must have the same number of points")
    m = int(round(days * 1440.0 / step_min))
    if m < 1:
        raise ValueError("days / step_min gives no date")
    times = [start + timedelta(minutes=k * step_min) for k in range(m)]
    ep = ephemeris.sun_epochs(times, observer)
    rt.horizon_azimuths(n_az)       # checks n_az
    chunk = max(1, min(int(chunk), la.size, (1 << 31) // int(n_az)))
    out = np.empty((la.size, 4), np.float32)
    stats = {}
    raised = _heights(height_m, radius_m, la.size)
    buf = DeviceBuffer(chunk * int(n_az) * 4, rt.config()["device"])
    try:
        for a in range(0, la.size, chunk):
            b = min(a + chunk, la.size)
            rt.horizon(la[a:b], lo[a:b], n_az=n_az, n_bis=n_bis, stats=stats, out=buf, **raised(a, b))
            out[a:b] = rt.horizon_sun(la[a:b], lo[a:b], buf, ep, summary=True, stats=stats, n_az=n_az)
    finally:
        buf.free()
    return IlluminationStatistics(out[:, 0], out[:, 1], out[:, 2], out[:, 3].astype(np.float64) * (step_min / 60.0), times, stats)


class SiteWindows(NamedTuple):
    times: list                   # the dates used
    sun_share: np.ndarray         # (N,) share of the dates with at least min_sun of the Sun's disc above the horizon
    longest_no_sun_h: np.ndarray  # (N,) longest run of consecutive dates without that, hours (run x step)
    earth_share: np.ndarray       # (N,) share of the dates with at least min_earth of the Earth's disc above the horizon
    longest_no_earth_h: np.ndarray  # (N,) longest run of consecutive dates without that, hours
    both_share: np.ndarray        # (N,) share of the dates with both
    longest_both_h: np.ndarray    # (N,) the longest unbroken working window: consecutive dates with both, hours
    best_start: np.ndarray        # (N,) int: index into `times` of that window's first date (the earliest such; -1: none)
    longest_outage_h: np.ndarray  # (N,) longest run of consecutive dates without both, hours
    stats: dict                   # summed counters and kernel times of the horizon and the windows calls


def site_windows(rt, lat, lon, start, days, step_min=60, height_m=0.0, min_sun=0.5, min_earth=1.0, n_az=256, n_bis=14,
                 observer=None, chunk=65536, radius_m=1737400.0):
    """For how long can a lander work at the points (lat, lon in degrees) without a break -- Sun on the panel AND the Earth in
    view -- from `start` (timezone-aware) over `days` at `step_min` minutes?  Each point's horizon
    is computed once from a mast top height_m above it (one height or one per point; MoonRT.horizon), then held against the
    Sun (ephemeris.sun_epochs) and the Earth (ephemeris.earth_epochs) on every date and reduced on the device
    (MoonRT.horizon_windows): a date counts for the Sun when at least min_sun of its disc is above the horizon, for the Earth
    when at least min_earth of its disc is.  Points are streamed `chunk` at a time; their horizons stay in a device buffer
    and no (points x dates) table is ever formed.  Returns SiteWindows."""
    from .renderer import DeviceBuffer
    la = np.atleast_1d(np.asarray(lat, np.float64)).ravel()
    lo = np.atleast_1d(np.asarray(lon, np.float64)).ravel()
    if la.shape != lo.shape:
        raise ValueError("lat and lon must have the same number of points")
    m = int(round(days * 1440.0 / step_min))
    if m < 1:
        raise ValueError("days / step_min gives no date")
    times = [start + timedelta(minutes=k * step_min) for k in range(m)]
    ep_sun, ep_earth = ephemeris.sun_earth_epochs(times, observer)
    rt.horizon_azimuths(n_az)       # checks n_az
    raised = _heights(0.0 if height_m is None else height_m, radius_m, la.size)
    chunk = max(1, min(int(chunk), la.size, (1 << 31) // int(n_az)))
    out = np.empty((la.size, 8), np.float32)
    stats = {}
    buf = DeviceBuffer(chunk * int(n_az) * 4, rt.config()["device"])
    try:
        for a in range(0, la.size, chunk):
            b = min(a + chunk, la.size)
            rt.horizon(la[a:b], lo[a:b], n_az=n_az, n_bis=n_bis, stats=stats, out=buf, **raised(a, b))
            out[a:b] = rt.horizon_windows(la[a:b], lo[a:b], buf, ep_sun, ep_earth, min_a=min_sun, min_b=min_earth, n_az=n_az,
                                          stats=stats)
    finally:
        buf.free()
    hours = step_min / 60.0
    run = lambda j: out[:, j].astype(np.float64) * hours     # noqa: E731
    return SiteWindows(times, out[:, 0], run(1), out[:, 2], run(3), out[:, 4], run(5), out[:, 6].astype(np.int64), run(7), stats)


class PowerBudget(NamedTuple):
    times: list                   # the dates used
    generated_wh: np.ndarray      # (N,) energy the array generated over the dates, Wh
    net_wh: np.ndarray            # (N,) generated minus drawn, Wh
    storage_wh: np.ndarray        # (N,) the least battery which, starting full, never empties: the worst cumulative deficit, Wh
    deficit_start: np.ndarray     # (N,) int: index into `times` of that deficit's first date (-1: the balance never falls)
    deficit_end: np.ndarray       # (N,) int: index of its last date (-1: none)
    min_charge_wh: np.ndarray     # (N,) lowest state of charge of the capacity_wh battery, Wh
    unmet_h: np.ndarray           # (N,) hours during which that battery could not carry the load
    unmet_wh: np.ndarray          # (N,) energy the load asked for and did not get, Wh
    cpw_log2: int                 # counts per watt = 2^cpw_log2 (section 3.17)
    stats: dict                   # summed counters and kernel times of the horizon and the budget calls


def counts_to_wh(counts, cpw_log2, step_min):
    """Counts of 2^-cpw_log2 W x one epoch as Wh, float64: exact up to the one rounding of the
    product with the epoch's hours."""
    return np.asarray(counts, np.float64) * 2.0 ** -int(cpw_log2) * (float(step_min) / 60.0)


def wh_to_counts(wh, cpw_log2, step_min):
    """The whole number of counts nearest to `wh` (a battery's capacity, say)."""
    return int(round(float(wh) * 2.0 ** int(cpw_log2) / (float(step_min) / 60.0)))


def power_budget(rt, lat, lon, start, days, step_min=60, height_m=0.0, *, area_m2, efficiency, load_w, panel="track",
                 normal_enu=None, capacity_wh=0.0, initial_wh=None, n_az=256, n_bis=14, observer=None, chunk=65536,
                 radius_m=1737400.0, cpw_log2=None, eclipses=False):
    """Does a solar-powered asset survive at the points (lat, lon in degrees), and on how much battery, from `start`
    (timezone-aware) over `days` at `step_min` minutes?  Each point's horizon is computed once from
    a panel height_m above it (MoonRT.horizon), the Sun's epochs and flux once (ephemeris.sun_epochs, sun_flux); the array
    delivers flux x area_m2 x efficiency W facing the whole Sun, scaled per date by the visible share of the disc and the
    panel's cosine ("track", "fixed" with normal_enu, "azimuth").  load_w is the power drawn: one value, or one per date (an
    (awake, hibernating) rule would depend on each point's own Sun and is not offered).  The balance is reduced on the
    device (MoonRT.power_budget): points are streamed `chunk` at a time, their horizons stay in a device buffer and no
    (points x dates) table is formed.  capacity_wh is the battery whose state of charge is followed (initial_wh=None:
    full).  eclipses=True multiplies the array's output by ephemeris.eclipse_factor, the Earth's cover of the Sun seen from
    the Moon's centre (section 3.18): one factor for the whole Moon, so near a contact a site's own cover differs from it;
    a per-point term in the budget kernel does not exist.  Returns PowerBudget."""
    from .renderer import DeviceBuffer
    la = np.atleast_1d(np.asarray(lat, np.float64)).ravel()
    lo = np.atleast_1d(np.asarray(lon, np.float64)).ravel()
    if la.shape != lo.shape:
        raise ValueError("lat and lon must have the same number of points")
    m = int(round(days * 1440.0 / step_min))
    if m < 1:
        raise ValueError("days / step_min gives no date")
    times = [start + timedelta(minutes=k * step_min) for k in range(m)]
    load = np.asarray(load_w, np.float64)
    if load.ndim > 1 or (load.ndim == 1 and load.size != m):
        raise ValueError("load_w must be one value or one per date")
    load = np.ascontiguousarray(np.broadcast_to(load, (m,)))
    ep = ephemeris.sun_epochs(times, observer)
    gen = ephemeris.sun_flux(times) * (float(area_m2) * float(efficiency))
    if eclipses:
        gen = gen * ephemeris.eclipse_factor(times, observer)
    cpw = rt.power_scale(gen, load) if cpw_log2 is None else int(cpw_log2)
    cap = wh_to_counts(capacity_wh, cpw, step_min)
    ini = cap if initial_wh is None else wh_to_counts(initial_wh, cpw, step_min)
    rt.horizon_azimuths(n_az)       # checks n_az
    raised = _heights(0.0 if height_m is None else height_m, radius_m, la.size)
    chunk = max(1, min(int(chunk), la.size, (1 << 31) // int(n_az)))
    out = np.empty((la.size, 8), np.int64)
    stats = {}
    buf = DeviceBuffer(chunk * int(n_az) * 4, rt.config()["device"])
    try:
        for a in range(0, la.size, chunk):
            b = min(a + chunk, la.size)
            rt.horizon(la[a:b], lo[a:b], n_az=n_az, n_bis=n_bis, stats=stats, out=buf, **raised(a, b))
            out[a:b] = rt.power_budget(la[a:b], lo[a:b], buf, ep, gen, load, panel=panel, normal_enu=normal_enu, cpw_log2=cpw,
                                       capacity=cap, initial=ini, n_az=n_az, stats=stats)
    finally:
        buf.free()
    wh = lambda j: counts_to_wh(out[:, j], cpw, step_min)     # noqa: E731
    return PowerBudget(times, wh(0), wh(1), wh(2), out[:, 3].copy(), out[:, 4].copy(), wh(5),
                       out[:, 6].astype(np.float64) * (step_min / 60.0), wh(7), cpw, stats)


class SurfaceTemperatures(NamedTuple):
    t_max: np.ndarray             # (N,) highest surface temperature over the recorded dates, K
    t_min: np.ndarray             # (N,) lowest, K
    t_mean: np.ndarray            # (N,) mean, K
    t_bottom_mean: np.ndarray     # (N,) mean of the column's bottom node over the recorded dates, K
    times: list                   # the recorded dates (the spin-up dates precede them)
    stats: dict                   # summed counters and kernel times of the horizon and the thermal calls


def surface_temperatures(rt, lat, lon, start, days, step_min=60, spinup_lunations=None, n_az=256, n_bis=14, observer=None,
                         chunk=65536, thermal=None, scatter=0, budget_bytes=8 << 30, q_sec_mean=False, alloc=None,
                         eclipses=False):
    """Regolith surface temperatures of the points (lat, lon in degrees) from `start` (timezone-aware) over `days` at
    `step_min` minutes.  The column is spun up over `spinup_lunations` lunations of dates before
    `start` (default thermal.SPINUP_LUNATIONS), stepped but not recorded.  Each point's horizon is computed once
    (MoonRT.horizon); points are streamed `chunk` at a time and their horizons stay in a device buffer.  `thermal` replaces
    rt.surface_temperature (same signature; it then receives the horizons as a host array).  Returns SurfaceTemperatures.

    scatter = K > 0 adds the sunlight and infrared the surrounding terrain sends (section 3.11): K view rays per point, the
    hits' own columns in EXITANCE mode, the gather and the points' columns with that extra flux.  Device tables stay under
    about `budget_bytes` per group of points; `q_sec_mean` also returns each point's mean extra flux over the recorded dates
    (stats["q_sec_mean"]; it downloads the flux).  `alloc(nbytes)` replaces the device allocation (tests).

    eclipses=True lets the Earth cover the Sun (section 3.18): every column call, the scatter path's hit columns included,
    runs MoonRT.thermal_column with the occultation tables (ephemeris.far_sun_epochs, earth_epochs) of its dates.  A
    `thermal` replacement keeps today's signature, which has no place for them: the two together raise ValueError."""
    out, times, stats, _ = _columns(rt, lat, lon, start, days, step_min, spinup_lunations, n_az, n_bis, observer, chunk, thermal,
                                    scatter, budget_bytes, q_sec_mean, alloc, None, eclipses)
    return SurfaceTemperatures(out[:, 0], out[:, 1], out[:, 2], out[:, 3], times, stats)


def _occultation_tables(times, observer):
    """(sun_epochs, (far_sun_epochs, earth_epochs)) of the dates, from one pass over them."""
    ep, earth = ephemeris.sun_earth_epochs(times, observer)
    return ep, (ephemeris.far_sun_epochs(ep, times), earth)


def _columns(rt, lat, lon, start, days, step_min, spinup_lunations, n_az, n_bis, observer, chunk, thermal, scatter, budget_bytes,
             q_sec_mean, alloc, species, eclipses=False):
    """The flow surface_temperatures and ice_stability share: the dates, the model, and per chunk of points the horizons and
    the columns.  species = None: the points' columns run in SUMMARY, (N, 4) float32; a species: in VOLATILE
    (MoonRT.thermal_column, section 3.16), (N, n_nodes, 2) float64.  eclipses: every column call goes through
    MoonRT.thermal_column with the occultation tables of its dates (section 3.18).  Returns (out, the recorded dates, stats,
    model)."""
    from . import thermal as th
    if eclipses and thermal is not None:
        raise ValueError("thermal= keeps its signature, which has no occultation tables: it cannot be combined with eclipses=True")
    la = np.atleast_1d(np.asarray(lat, np.float64)).ravel()
    lo = np.atleast_1d(np.asarray(lon, np.float64)).ravel()
    if la.shape != lo.shape:
        raise ValueError("lat and lon must have the same number of points")
    m_rec = int(round(days * 1440.0 / step_min))
    if m_rec < 1:
        raise ValueError("days / step_min gives no date")
    spin = th.SPINUP_LUNATIONS if spinup_lunations is None else int(spinup_lunations)
    model = rt.thermal_grid(step_min * 60.0, spin, min(th.RESETS, spin))
    n_spin = int(model.n_spin)
    step = timedelta(minutes=float(step_min))
    all_times = [start + (k - n_spin) * step for k in range(n_spin + m_rec)]
    rt.horizon_azimuths(n_az)       # checks n_az
    chunk = max(1, min(int(chunk), la.size, (1 << 31) // int(n_az)))
    out = _columns_out(la.size, model, species)
    stats = {}
    if scatter:
        times, stats = _scatter_temperatures(rt, la, lo, start, step, m_rec, model, n_az, n_bis, observer, chunk, int(scatter),
                                             budget_bytes, q_sec_mean, alloc, species, out, eclipses)
        return out, times, stats, model
    occ = None
    if eclipses:
        ep, occ = _occultation_tables(all_times, observer)
    else:
        ep = ephemeris.sun_epochs(all_times, observer)
    fl = ephemeris.sun_flux(all_times)
    if thermal is not None:
        if species is not None:
            raise ValueError("thermal= replaces the SUMMARY call only")
        for a in range(0, la.size, chunk):
            b = min(a + chunk, la.size)
            hz = rt.horizon(la[a:b], lo[a:b], n_az=n_az, n_bis=n_bis, stats=stats)
            out[a:b] = thermal(la[a:b], lo[a:b], hz, ep, fl, model=model, mode="summary", stats=stats, n_az=n_az)
    else:
        from .renderer import DeviceBuffer
        buf = DeviceBuffer(chunk * int(n_az) * 4, rt.config()["device"])
        try:
            for a in range(0, la.size, chunk):
                b = min(a + chunk, la.size)
                rt.horizon(la[a:b], lo[a:b], n_az=n_az, n_bis=n_bis, stats=stats, out=buf)
                if occ is not None:
                    out[a:b] = rt.thermal_column(la[a:b], lo[a:b], buf, ep, fl, model=model,
                                                 mode="summary" if species is None else "volatile", species=species,
                                                 stats=stats, n_az=n_az, occultation=occ)
                elif species is None:
                    out[a:b] = rt.surface_temperature(la[a:b], lo[a:b], buf, ep, fl, model=model, mode="summary", stats=stats,
                                                      n_az=n_az)
                else:
                    out[a:b] = rt.thermal_column(la[a:b], lo[a:b], buf, ep, fl, model=model, mode="volatile", species=species,
                                                 stats=stats, n_az=n_az)
        finally:
            buf.free()
    return out, all_times[n_spin:], stats, model


def _columns_out(n, model, species):
    """The array the points' final column call fills: SUMMARY's, or with a species VOLATILE's."""
    if species is None:
        return np.empty((n, 4), np.float32)
    return np.empty((n, int(model.n_nodes), 2), np.float64)


def compact_hits(hits):
    """The hit list of view_hits' (N, K, 2) output: (index (N, K) int32 into the list, -1 for sky; the hits' lat, lon as
    float64), the hits numbered point-major."""
    hit = ~np.isnan(hits[..., 0])
    index = np.full(hit.shape, -1, np.int32)
    index[hit] = np.arange(int(hit.sum()), dtype=np.int32)
    return index, hits[..., 0][hit].astype(np.float64), hits[..., 1][hit].astype(np.float64)


def scatter_groups(hit_counts, m_hits, m_targets, n_az, budget_bytes):
    """Split the points of a chunk into consecutive groups [a, b) whose device tables stay within budget_bytes: per hit its
    EXITANCE row (m_hits x 8 bytes) and horizon, per point its extra-flux row (m_targets x 4 bytes) and horizon -- and whose
    hits' EXITANCE fits one call (at most 2^30 (M_vis, M_ir) pairs).  A group holds at least one point."""
    per_hit = 8 * m_hits + 4 * n_az
    per_pt = 4 * m_targets + 4 * n_az
    max_hits = max(1, (1 << 30) // max(int(m_hits), 1))
    groups, a, used, hits = [], 0, 0, 0
    for i, h in enumerate(np.asarray(hit_counts, np.int64)):
        need = int(h) * per_hit + per_pt
        if i > a and (used + need > budget_bytes or hits + int(h) > max_hits):
            groups.append((a, i))
            a, used, hits = i, 0, 0
        used += need
        hits += int(h)
    if a < len(hit_counts):
        groups.append((a, len(hit_counts)))
    return groups


def _scatter_temperatures(rt, la, lo, start, step, m_rec, model, n_az, n_bis, observer, chunk, k, budget_bytes, q_sec_mean,
                          alloc, species, out, eclipses=False):
    """_columns with scatter = K (section 3.11).  Per chunk of points: their view hits; per group of points that fits the
    budget: their horizons, the hits' horizons, the hits' columns in EXITANCE mode over [own spin-up | the points' spin-up |
    recorded], the gather, and the points' columns with the extra flux (SUMMARY, or with a species VOLATILE) into `out`.
    Returns (the recorded dates, stats)."""
    import time
    from . import thermal as th
    rt.view_samples(k)              # checks K
    n_spin = int(model.n_spin)
    m_t = n_spin + m_rec
    # the hits' epochs: their own spin-up, then the points' epochs (spin-up and recorded), which the hits record
    times = [start + (i - 2 * n_spin) * step for i in range(2 * n_spin + m_rec)]
    occ_h = occ_t = None
    if eclipses:                    # section 3.18: the hits' columns and the points' columns both under the Earth's cover
        ep_h, occ_h = _occultation_tables(times, observer)
        occ_t = (occ_h[0][n_spin:], occ_h[1][n_spin:])
    else:
        ep_h = ephemeris.sun_epochs(times, observer)
    fl_h = ephemeris.sun_flux(times)
    ep_t, fl_t = ep_h[n_spin:], fl_h[n_spin:]
    a_h = th.albedo_hemispherical()
    if alloc is None:
        from .renderer import DeviceBuffer
        device = rt.config()["device"]
        alloc = lambda nbytes: DeviceBuffer(max(int(nbytes), 4), device)     # noqa: E731
    stats = {"scatter_hits": 0, "view_factor": np.empty(la.size, np.float32), "stage_s": {}}
    if q_sec_mean:
        stats["q_sec_mean"] = np.zeros(la.size, np.float64)
    stage = stats["stage_s"]

    def timed(name, fn):
        t0 = time.perf_counter()
        r = fn()
        stage[name] = stage.get(name, 0.0) + time.perf_counter() - t0
        return r

    chunk = max(1, min(int(chunk), la.size, (1 << 31) // (2 * k + 1)))
    for a in range(0, la.size, chunk):
        b = min(a + chunk, la.size)
        hits, share = timed("view_hits", lambda: rt.view_hits(la[a:b], lo[a:b], k=k, stats=stats))
        stats["view_factor"][a:b] = share
        index, h_lat, h_lon = timed("compact", lambda: compact_hits(hits))
        counts = (index >= 0).sum(axis=1)
        first = np.concatenate([[0], np.cumsum(counts)])
        for ga, gb in scatter_groups(counts, m_t, m_t, n_az, budget_bytes):
            p0, p1 = a + ga, a + gb
            h0, h1 = int(first[ga]), int(first[gb])
            n_h = h1 - h0
            stats["scatter_hits"] += n_h
            bufs = []
            try:
                hz_t = alloc((p1 - p0) * n_az * 4)
                bufs.append(hz_t)
                timed("horizons", lambda: rt.horizon(la[p0:p1], lo[p0:p1], n_az=n_az, n_bis=n_bis, stats=stats, out=hz_t))
                q = None
                if n_h:
                    hz_h = alloc(n_h * n_az * 4)
                    bufs.append(hz_h)
                    timed("hit_horizons", lambda: rt.horizon(h_lat[h0:h1], h_lon[h0:h1], n_az=n_az, n_bis=n_bis, stats=stats,
                                                             out=hz_h))
                    ex = alloc(n_h * m_t * 8)
                    bufs.append(ex)
                    if occ_h is not None:
                        timed("hit_columns", lambda: rt.thermal_column(
                            h_lat[h0:h1], h_lon[h0:h1], hz_h, ep_h, fl_h, model=model, mode="exitance", stats=stats, n_az=n_az,
                            out=ex, occultation=occ_h))
                    else:
                        timed("hit_columns", lambda: rt.surface_temperature_scatter(
                            h_lat[h0:h1], h_lon[h0:h1], hz_h, ep_h, fl_h, model=model, mode="exitance", stats=stats, n_az=n_az,
                            out=ex))
                    q = alloc((p1 - p0) * m_t * 4)
                    bufs.append(q)
                    idx = np.where(index[ga:gb] >= 0, index[ga:gb] - h0, -1).astype(np.int32)
                    timed("gather", lambda: rt.scatter_flux(idx, ex, a_h, th.EMISSIVITY, n_hits=n_h, m=m_t, out=q,
                                                            stats=stats))
                    if q_sec_mean:
                        qs = q.download(np.float32, (p1 - p0, m_t))
                        stats["q_sec_mean"][p0:p1] = qs[:, n_spin:].astype(np.float64).mean(axis=1)
                if occ_t is not None:
                    out[p0:p1] = timed("columns", lambda: rt.thermal_column(
                        la[p0:p1], lo[p0:p1], hz_t, ep_t, fl_t, model=model, mode="summary" if species is None else "volatile",
                        extra_flux=q, species=species, stats=stats, n_az=n_az, occultation=occ_t))
                elif species is None:
                    out[p0:p1] = timed("columns", lambda: rt.surface_temperature_scatter(
                        la[p0:p1], lo[p0:p1], hz_t, ep_t, fl_t, model=model, mode="summary", extra_flux=q, stats=stats,
                        n_az=n_az))
                else:
                    out[p0:p1] = timed("columns", lambda: rt.thermal_column(
                        la[p0:p1], lo[p0:p1], hz_t, ep_t, fl_t, model=model, mode="volatile", extra_flux=q, species=species,
                        stats=stats, n_az=n_az))
            finally:
                for buf in bufs:
                    buf.free()
    return times[2 * n_spin:], stats


class IceStability(NamedTuple):
    depth_m: np.ndarray           # (N,) the shallowest depth at which buried ice is stable, m (0: at the surface; inf: nowhere)
    loss_rate_surface: np.ndarray  # (N,) the retreat rate of exposed ice at the surface, m s^-1 (E_mean_0 / rho_solid)
    e_mean: np.ndarray            # (N, n_nodes) time-mean free sublimation rate at every node, kg m^-2 s^-1
    t_max_nodes: np.ndarray       # (N, n_nodes) highest temperature of every node over the recorded dates, K
    z: np.ndarray                 # (n_nodes,) node depths, m
    times: list                   # the recorded dates (the spin-up dates precede them)
    stats: dict                   # summed counters and kernel times of every call made


def ice_stability(rt, lat, lon, start, days, step_min=60, spinup_lunations=None, n_az=256, n_bis=14, observer=None,
                  chunk=65536, species=None, scatter=0, rate_max=None, barrier_m=None, budget_bytes=8 << 30, alloc=None,
                  eclipses=False):
    """How deep must ice of `species` (default volatiles.H2O) be buried at the points (lat, lon in degrees) to survive
    ?  The run is surface_temperatures' -- the same dates, spin-up, horizons, chunks and, with
    scatter = K, scatter groups -- with the points' final columns in VOLATILE mode: per node the mean over the recorded dates
    of the free sublimation rate and the highest temperature.  volatiles.stability_depth turns the rates into a depth: the
    shallowest at which the retreat rate E_mean / rho_solid is at most rate_max (default 1 mm per 10^9 years), with
    barrier_m the diffusion length of an overlying dry lag (None: the exposed-ice criterion).  One species per call.  The
    regolith's properties are the dry ones throughout: ice changes neither its conductivity nor its heat capacity, and the
    rate is the time mean of the free rate, without pumping or recondensation.  eclipses as for surface_temperatures.
    Returns IceStability."""
    from . import volatiles
    species = volatiles.H2O if species is None else species
    rate_max = volatiles.RATE_MAX if rate_max is None else float(rate_max)
    out, times, stats, model = _columns(rt, lat, lon, start, days, step_min, spinup_lunations, n_az, n_bis, observer, chunk,
                                        None, scatter, budget_bytes, False, alloc, species, eclipses)
    z = rt.thermal_depths(model)
    e_mean = out[:, :, 0]
    depth = volatiles.stability_depth(e_mean, z, species, rate_max=rate_max, barrier_m=barrier_m)
    return IceStability(depth, e_mean[:, 0] / species.rho_solid, e_mean, out[:, :, 1], z, times, stats)


class LunarEclipse(NamedTuple):
    times: list                   # the finely sampled dates of this eclipse
    penumbral_start: np.ndarray   # (N,) object: the first date at which the point has g < 1 (None: the point saw nothing)
    penumbral_end: np.ndarray     # (N,) object: the last such date
    total_start: np.ndarray       # (N,) object: the first date with g == 0 (None: no totality at the point)
    total_end: np.ndarray         # (N,) object: the last such date
    g_min: np.ndarray             # (N,) float32: the least uncovered share of the Sun's disc
    totality_min: np.ndarray      # (N,) minutes with g == 0
    stats: dict                   # summed counters and kernel time of the occultation call


def lunar_eclipses(rt, lat, lon, start, days, step_min=1, observer=None, coarse_min=10):
    """The lunar eclipses the points (lat, lon in degrees) see from `start` (timezone-aware) over `days` (DESIGN.md section
    3.18): the span is scanned every coarse_min minutes by ephemeris.eclipse_candidates on the host; each range it finds,
    widened by one coarse step on either side, is sampled every step_min minutes and handed to MoonRT.occultation (FULL,
    points x the few hundred dates of one eclipse; nothing is sampled finely outside the candidates).  Returns a list of
    LunarEclipse, one per candidate range in which some point has g < 1, in date order.  g is the geometric discs' -- no
    atmosphere -- and counts whether or not the terrain or the point's own horizon lets it see the Sun."""
    la = np.atleast_1d(np.asarray(lat, np.float64)).ravel()
    lo = np.atleast_1d(np.asarray(lon, np.float64)).ravel()
    if la.shape != lo.shape:
        raise ValueError("lat and lon must have the same number of points")
    n_coarse = int(math.ceil(days * 1440.0 / coarse_min))
    if n_coarse < 1:
        raise ValueError("days / coarse_min gives no date")
    coarse = [start + timedelta(minutes=k * coarse_min) for k in range(n_coarse)]
    out = []
    for a, b in ephemeris.eclipse_candidates(coarse, observer):
        t0 = max(coarse[a] - timedelta(minutes=coarse_min), start)
        t1 = min(coarse[b - 1] + timedelta(minutes=coarse_min), start + timedelta(days=days))
        m = int((t1 - t0).total_seconds() // (60.0 * step_min)) + 1
        times = [t0 + timedelta(minutes=k * step_min) for k in range(m)]
        sun, earth = ephemeris.sun_earth_epochs(times, observer)
        stats = {}
        g = rt.occultation(la, lo, ephemeris.far_sun_epochs(sun, times), earth, stats=stats)
        part, tot = g < 1.0, g == 0.0
        if not part.any():
            continue

        def ends(mask):
            first = np.array([times[int(np.argmax(r))] if r.any() else None for r in mask], object)
            last = np.array([times[m - 1 - int(np.argmax(r[::-1]))] if r.any() else None for r in mask], object)
            return first, last
        p0, p1 = ends(part)
        u0, u1 = ends(tot)
        out.append(LunarEclipse(times, p0, p1, u0, u1, g.min(axis=1), tot.sum(axis=1) * float(step_min), stats))
    return out
