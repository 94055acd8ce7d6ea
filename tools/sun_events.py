#!/usr/bin/env python3
"""Sunrise / sunset times on the real terrain at a list of points (moonrtx_amd.sunlight.terrain_sun_events, DESIGN.md
section 3.7): first light, full disc, disc cut and last light, each bracketed to step / (refine + 1), with the smooth
sphere's Sun altitude at that time.

  python tools/sun_events.py --time 2025-03-01T00:00:00+00:00 --lat 52.2 --lon 21.0 --days 30 --step-min 10 \\
      --point -25.3 1.1 --point -14.0 -1.5 --out events.csv
(synthetic LOLA-like DEM unless --elevation-file is given; the DEM options are tools/illumination_map.py's).  Prints the
events and the kernel time and counters of the coarse and the refining series (--count adds the deterministic ones)."""
import argparse, csv, os, sys, time
from datetime import datetime
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
from moonrtx_amd import ephemeris, _lib
from moonrtx_amd.renderer import MoonRT, synth_ldem, dem_from_ldem
from moonrtx_amd.sunlight import terrain_sun_events

ap = argparse.ArgumentParser()
ap.add_argument("--time", required=True, help="start, ISO 8601 with UTC offset")
ap.add_argument("--lat", type=float, required=True, help="observer latitude")
ap.add_argument("--lon", type=float, required=True, help="observer longitude")
ap.add_argument("--elevation-m", type=float, default=0.0)
ap.add_argument("--days", type=float, default=30.0)
ap.add_argument("--step-min", type=float, default=10.0)
ap.add_argument("--refine", type=int, default=15)
ap.add_argument("--n-sun", type=int, default=16)
ap.add_argument("--point", type=float, nargs=2, action="append", default=[], metavar=("LAT", "LON"))
ap.add_argument("--points-file", default=None, help="text file of 'lat lon' lines (selenographic degrees)")
ap.add_argument("--downscale", type=int, default=8)
ap.add_argument("--dem-size", type=int, nargs=2, default=None, help="synthetic DEM (h, w); default 46080/downscale x 92160/downscale")
ap.add_argument("--elevation-file", default=None)
ap.add_argument("--count", action="store_true", help="maintain the deterministic counters (the counting kernel)")
ap.add_argument("--out", default=None, help="events as CSV")
a = ap.parse_args()

pts = list(a.point)
if a.points_file:
    pts += [tuple(r) for r in np.loadtxt(a.points_file, ndmin=2)[:, :2]]
if not pts:
    ap.error("give at least one --point or a --points-file")
pts = np.asarray(pts, np.float64)
obs = ephemeris.Observer(a.lat, a.lon, a.elevation_m)
t0 = datetime.fromisoformat(a.time)
if a.elevation_file:
    from moonrtx_amd.ingest import load_elevation_data
    dem, _ = load_elevation_data(a.elevation_file, a.downscale, device=0)
    dh, dw = dem.shape
    dem_buf = None
else:
    dh, dw = a.dem_size or (46080 // a.downscale, 92160 // a.downscale)
    src = synth_ldem(dh, dw, device=0)
    dem_buf, _ = dem_from_ldem(src, dh, dw, 1, device=0)
    src.free()
rt = MoonRT(16, 16, device=0)
if dem_buf is None:
    rt.upload_dem(dem)
else:
    rt.bind_dem(dem_buf, dh, dw)
rt.set_params(flags=_lib.F_COUNT_STATS if a.count else 0)
w0 = time.perf_counter()
res = terrain_sun_events(rt, pts[:, 0], pts[:, 1], t0, a.days, step_min=a.step_min, n_sun=a.n_sun, refine=a.refine, observer=obs)
wall = time.perf_counter() - w0
print(f"{'point':>5} {'lat':>8} {'lon':>9} {'event':<11} {'t_lo (UTC)':<20} {'t_hi (UTC)':<20} {'sphere alt':>10} {'moon alt':>8} flicker")
rows = []
for e in res.events:
    la, lo = pts[e.point]
    lo_s, hi_s = (t.astimezone(t0.tzinfo).strftime("%Y-%m-%d %H:%M:%S") for t in (e.t_lo, e.t_hi))
    print(f"{e.point:5d} {la:8.3f} {lo:9.3f} {e.kind:<11} {lo_s:<20} {hi_s:<20} {e.sun_alt_sphere:10.3f} {e.moon_alt:8.2f} "
          f"{'yes' if e.flicker else ''}")
    rows.append([e.point, la, lo, e.kind, e.t_lo.isoformat(), e.t_hi.isoformat(), e.sun_alt_sphere, e.moon_alt, int(e.flicker)])
for name, st in (("coarse", res.coarse), ("refine", res.refine)):
    rays = st.get("shadow_rays", 0)
    rate = f", {rays / st['kernel_ms'] / 1e6:.2f} G shadow rays/s" if rays and st.get("kernel_ms") else ""
    print(f"{name} series: {st.get('kernel_ms', 0.0):.3f} ms in {st.get('launches', 0)} launch(es); counters {st}{rate}")
print(f"{len(pts)} points x {len(res.times)} dates: {len(res.events)} events, {wall:.2f} s end to end (ephemeris included)")
if a.out:
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(["point", "lat", "lon", "kind", "t_lo", "t_hi", "sun_alt_sphere", "moon_alt", "flicker"])
        w.writerows(rows)
    print(f"wrote {a.out}")
rt.close()
if dem_buf is not None:
    dem_buf.free()
