#!/usr/bin/env python3
"""Measure the occultation stage on one GPU, on a polar window of the full-size DEM:
mrtx_occultation SUMMARY and FULL over a year of hourly epochs (kernel time from the library's HIP events, and wall time per
call, read-back included); the same SUMMARY over the eclipses of the year at 1-minute steps, found by
ephemeris.eclipse_candidates; and the thermal column in SUMMARY through mrtx_thermal_column, through mrtx_thermal_occulted
without tables (the same kernel) and with them, on the same inputs, --repeat runs each, alternating, so that the spread
between runs of one path is seen beside the difference between paths.  The three thermal outputs are compared: the first two
bit for bit, the third wherever the year's g is 1 throughout.

  python tools/eclipse_bench.py --dem-size 23040 46080 --size 256 256 --days 365 --out profiles/eclipse_bench.json
"""
import argparse, ctypes as C, json, os, sys, time
from datetime import datetime, timedelta, timezone
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
from moonrtx_amd import ephemeris, thermal
from moonrtx_amd._lib import MrtxStats
from moonrtx_amd.renderer import DeviceBuffer, MoonRT, synth_ldem, dem_from_ldem
from moonrtx_amd.scene import named_scene

ap = argparse.ArgumentParser()
ap.add_argument("--dem-size", type=int, nargs=2, default=(23040, 46080))
ap.add_argument("--window", type=float, nargs=4, default=(-84.0, -90.0, -180.0, 180.0), metavar=("N", "S", "W", "E"))
ap.add_argument("--size", type=int, nargs=2, default=(256, 256))
ap.add_argument("--n-az", type=int, default=256)
ap.add_argument("--n-bis", type=int, default=14)
ap.add_argument("--days", type=float, default=365.0)
ap.add_argument("--spinup-lunations", type=int, default=thermal.SPINUP_LUNATIONS)
ap.add_argument("--repeat", type=int, default=3)
ap.add_argument("--skip-full", action="store_true", help="leave out FULL over the year (points x epochs x 4 bytes read back)")
ap.add_argument("--out", default=None, help="write the numbers as JSON here")
a = ap.parse_args()

dh, dw = a.dem_size
src = synth_ldem(dh, dw)
dem, _ = dem_from_ldem(src, dh, dw, 1)
src.free()
rt = MoonRT(16, 16)
rt.bind_dem(dem, dh, dw)
rt.apply_scene(named_scene("S1", 16, 16))      # march parameters and Moon radius of S1 (step 5e-3, scene_epsilon 1e-4, R 10)
rt.set_params(flags=0)
la, lo = MoonRT.grid_nodes(lat=tuple(a.window[:2]), lon=tuple(a.window[2:]), shape=tuple(a.size))
LA, LO = [g.ravel() for g in np.meshgrid(la, lo, indexing="ij")]
P = LA.size
obs = ephemeris.Observer(52.2, 21.0, 0.0)
md = MoonRT.thermal_grid(3600.0, a.spinup_lunations)
m_rec = int(round(a.days * 24))
t0 = datetime(2025, 1, 1, tzinfo=timezone.utc)
times = [t0 + timedelta(hours=k - md.n_spin) for k in range(md.n_spin + m_rec)]
t = time.perf_counter()
sun, earth = ephemeris.sun_earth_epochs(times, obs)
far = ephemeris.far_sun_epochs(sun, times)
fl = ephemeris.sun_flux(times)
res = dict(points=P, n_az=a.n_az, epochs_year=m_rec, epochs_thermal=len(times), spin_epochs=int(md.n_spin),
           ephemeris_s=time.perf_counter() - t)
year = slice(int(md.n_spin), None)
t = time.perf_counter()
ranges = ephemeris.eclipse_candidates(times[year], obs)
res["candidates_s"] = time.perf_counter() - t
res["candidate_ranges"] = [[times[year][i].isoformat(), times[year][j - 1].isoformat()] for i, j in ranges]
res["marked_hours_of_the_year"] = int(sum(j - i for i, j in ranges))

# the eclipses of the year at 1-minute steps: each candidate range, widened by an hour either side
fine = []
for i, j in ranges:
    f0, f1 = times[year][i] - timedelta(hours=1), times[year][j - 1] + timedelta(hours=1)
    fine += [f0 + timedelta(minutes=k) for k in range(int((f1 - f0).total_seconds() // 60) + 1)]
if fine:
    sun_f, earth_f = ephemeris.sun_earth_epochs(fine, obs)
    far_f = ephemeris.far_sun_epochs(sun_f, fine)
res["epochs_fine"] = len(fine)


def timed(key, fn):
    st = {}
    t = time.perf_counter()
    r = fn(st)
    res.setdefault(key + "_wall_s", []).append(time.perf_counter() - t)
    res.setdefault(key + "_ms", []).append(st["kernel_ms"])
    res[key + "_launches"] = st["launches"]
    return r


rt.occultation(LA[:1024], LO[:1024], far[year], earth[year], summary=True)          # warm-up: code objects
rt.occultation(LA[:1024], LO[:1024], far[year][:64], earth[year][:64])
first = None
for rep in range(a.repeat):
    s_year = timed("summary_year", lambda st: rt.occultation(LA, LO, far[year], earth[year], summary=True, stats=st))
    if fine:
        s_fine = timed("summary_fine", lambda st: rt.occultation(LA, LO, far_f, earth_f, summary=True, stats=st))
    if not a.skip_full:
        g = timed("full_year", lambda st: rt.occultation(LA, LO, far[year], earth[year], stats=st, chunk_bytes=1 << 30))
        if rep == 0:
            res["full_equals_summary_counts"] = bool(
                np.array_equal((g < 1).sum(1), np.rint(s_year[:, 2].astype(np.float64) * m_rec).astype(np.int64)))
        del g
    if first is None:
        first = s_year
    elif not np.array_equal(first, s_year):
        sys.exit(f"run {rep}: SUMMARY differs from run 0")
res["full_output_bytes"] = P * m_rec * 4
res["year_least_g"] = float(s_year[:, 1].min())
res["year_eclipses_per_point"] = [int(s_year[:, 7].min()), int(s_year[:, 7].max())]
if fine:
    res["fine_longest_total_min"] = float(s_fine[:, 6].max())

# the thermal column: mrtx_thermal_column, mrtx_thermal_occulted without tables, and with them
buf = DeviceBuffer(P * a.n_az * 4)
st = {}
rt.horizon(LA, LO, n_az=a.n_az, n_bis=a.n_bis, stats=st, out=buf)
res["horizon_ms"] = st["kernel_ms"]
pts = np.ascontiguousarray(np.stack([LA, LO], -1))


def occulted_null(st):
    """mrtx_thermal_occulted with both tables NULL (the facade calls mrtx_thermal_column for that)."""
    out = np.empty((P, 4), np.float32)
    s_ = MrtxStats()
    rt._check(rt._lib.mrtx_thermal_occulted(rt._ctx, pts.ctypes.data, P, a.n_az, buf.ptr, None, sun.ctypes.data, fl.ctypes.data,
                                            len(times), C.byref(md), 1, None, None, 0, None, None, None, None, out.ctypes.data,
                                            C.byref(s_)), "mrtx_thermal_occulted")
    rt._add_stats(st, s_)
    return out


kw = dict(mode="summary", n_az=a.n_az)
rt.thermal_column(LA[:64], LO[:64], buf, sun, fl, md, **kw)                          # warm-up: code objects
rt.thermal_column(LA[:64], LO[:64], buf, sun, fl, md, occultation=(far, earth), **kw)
for rep in range(a.repeat):
    c0 = timed("thermal_column", lambda st: rt.thermal_column(LA, LO, buf, sun, fl, md, stats=st, **kw))
    c1 = timed("thermal_occulted_null", occulted_null)
    c2 = timed("thermal_occulted", lambda st: rt.thermal_column(LA, LO, buf, sun, fl, md, stats=st, occultation=(far, earth), **kw))
    if not np.array_equal(c0.view(np.uint32), c1.view(np.uint32)):
        sys.exit(f"run {rep}: mrtx_thermal_occulted without tables differs from mrtx_thermal_column")
res["thermal_points_changed_by_the_eclipses"] = int((c0.view(np.uint32) != c2.view(np.uint32)).any(1).sum())
res["thermal_t_min_change_K"] = float((c2[:, 1] - c0[:, 1]).min())
for k in ("thermal_column", "thermal_occulted_null", "thermal_occulted"):
    v = res[k + "_ms"]
    res[k + "_spread_ms"] = max(v) - min(v)
res["occulted_minus_column_ms"] = float(np.median(res["thermal_occulted_ms"]) - np.median(res["thermal_column_ms"]))
buf.free()
rt.close()
dem.free()
print(json.dumps(res))
if a.out:
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
