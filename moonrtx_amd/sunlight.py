"""When does the Sun rise on a spot of the real terrain?  Sunrise / sunset times from the Sun illumination series (DESIGN.md
section 3.7): a coarse series over the sampled dates, then one refining series over every transition found.

The reference times these events on the smooth sphere only (astro.py: find_terminator_windows, find_clair_obscur_events,
whose catalogue tunes each window by hand for the relief); here the terrain decides, and each event also reports the
sphere's Sun altitude at its time -- the number that catalogue tunes."""
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
