#!/usr/bin/env python3
"""Timed rover traverses, headless: when does the rover get there, and which way must it go so that it
only drives while its panel is lit (and, with --min-earth, while its antenna sees the Earth)?

  python tools/timed_traverse.py --window 21515 0 127 3840 12 1 --start -89.4 -137 --to -86 40 --time 2025-03-01T00:00 \\
      --days 30 --step-min 60 --speed 0.2 --min-sun 0.5 --min-earth 0.5 --height 2 --out arrival.npy --route route.csv
--window ROW0 COL0 ROWS COLS [STRIDE [WRAP]] as tools/traverse_map.py takes it.  The drive mask holds one epoch per --step-min
minutes from --time (UTC) over --days days: a node is available in an epoch when at least --min-sun of the Sun's disc (and
--min-earth of the Earth's) stands above its horizon, seen from --height metres above the ground.  Time is counted in seconds;
an edge lasts its effort (metres, as traverse_map.py's) divided by --speed.  The rover may wait at any node; an edge is driven
only while both of its ends are available.  The .npy holds the (rows, cols) float64 arrival times in hours after --time (+inf:
not reached before the mask ends); the CSV the route with arrival, departure and wait per node, in hours."""
import argparse, os, sys
from datetime import datetime, timedelta, timezone
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
from moonrtx_amd import traverse as tv
from moonrtx_amd.renderer import MoonRT, synth_ldem, dem_from_ldem
from moonrtx_amd.scene import named_scene

ap = argparse.ArgumentParser()
ap.add_argument("--window", type=int, nargs="+", required=True, metavar="N", help="ROW0 COL0 ROWS COLS [STRIDE [WRAP]] in DEM texels")
ap.add_argument("--start", type=float, nargs=2, required=True, metavar=("LAT", "LON"))
ap.add_argument("--to", type=float, nargs=2, required=True, metavar=("LAT", "LON"))
ap.add_argument("--time", required=True, metavar="T0", help="UTC, ISO 8601: the first epoch and the start of the drive")
ap.add_argument("--days", type=float, required=True)
ap.add_argument("--step-min", type=float, default=60.0, help="minutes per epoch of the drive mask")
ap.add_argument("--speed", type=float, default=0.2, metavar="MPS", help="metres of effort per second")
ap.add_argument("--min-sun", type=float, default=0.5)
ap.add_argument("--min-earth", type=float, default=None)
ap.add_argument("--height", type=float, default=0.0, help="panel / antenna height above the ground, metres")
ap.add_argument("--max-slope", type=float, default=20.0, help="degrees")
ap.add_argument("--climb", type=float, default=8.0, help="metres of effort per metre climbed")
ap.add_argument("--descent", type=float, default=0.0, help="metres of effort per metre descended")
ap.add_argument("--n-az", type=int, default=256)
ap.add_argument("--downscale", type=int, default=2)
ap.add_argument("--dem-size", type=int, nargs=2, default=None, help="synthetic DEM (h, w); default 46080/downscale x 92160/downscale")
ap.add_argument("--elevation-file", default=None)
ap.add_argument("--out", default="arrival.npy")
ap.add_argument("--route", default=None, help="CSV of the route to --to")
a = ap.parse_args()
if not 4 <= len(a.window) <= 6:
    ap.error("--window takes ROW0 COL0 ROWS COLS [STRIDE [WRAP]]")
if not a.speed > 0 or not a.step_min > 0 or not a.days > 0:
    ap.error("--speed, --step-min and --days must be > 0")
tpe = int(round(a.step_min * 60.0))         # 1 s ticks
if tpe < 1 or abs(tpe - a.step_min * 60.0) > 1e-9:
    ap.error("--step-min must be a whole number of seconds")
t0 = datetime.fromisoformat(a.time)
t0 = t0.replace(tzinfo=timezone.utc) if t0.tzinfo is None else t0
times = [t0 + timedelta(seconds=tpe * k) for k in range(max(1, int(a.days * 86400.0 / tpe)))]

if a.elevation_file:
    from moonrtx_amd.ingest import load_elevation_data
    dem, radius_scale = load_elevation_data(a.elevation_file, a.downscale, device=0)
    dh, dw = dem.shape
    dem_buf = None
else:
    dh, dw = a.dem_size or (46080 // a.downscale, 92160 // a.downscale)
    src = synth_ldem(dh, dw, device=0)
    dem_buf, radius_scale = dem_from_ldem(src, dh, dw, 1, device=0)
    src.free()
rt = MoonRT(16, 16, device=0)
if dem_buf is None:
    rt.upload_dem(dem)
else:
    rt.bind_dem(dem_buf, dh, dw)
rt.apply_scene(named_scene("S1", 16, 16))      # the march parameters of the horizons
rt.set_params(flags=0)
radius_m = 1737400.0 * float(radius_scale)
window = tuple(a.window)
mask = tv.drive_mask(rt, window, times, height_m=a.height, min_sun=a.min_sun, min_earth=a.min_earth, n_az=a.n_az)
w = tv.window_dict(window)
bits = tv.unpack_mask(mask.download(np.uint64, (w["rows"], w["cols"], tv.mask_words(len(times)))), len(times))
print(f"drive mask: {len(times)} epochs of {a.step_min:g} min; nodes are available in {float(bits.mean()):.4f} of their epochs, "
      f"{float(bits.any(-1).mean()):.4f} of the nodes at some time")
st = {}
f = rt.traverse_timed(window, sources=np.array([a.start], np.float64), avail=mask, n_epochs=len(times), ticks_per_epoch=tpe,
                      ticks_per_cost=1.0 / a.speed, max_slope_deg=a.max_slope, climb_cost=a.climb, descent_cost=a.descent,
                      radius_m=radius_m, stats=st)
mask.free()
os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
np.save(a.out, f.cost / 3600.0)
print(f"{f.cost.shape[0]}x{f.cost.shape[1]} nodes: {float(np.isfinite(f.cost).mean()):.4f} reached; {st['kernel_ms']:.2f} ms of "
      f"kernels, {st['launches']} relaxation launches, {st['tile_visits']} tile visits; wrote {a.out}")
ij = rt.snap_to_nodes(window, [a.to[0]], [a.to[1]])[0]
try:
    r = tv.timed_route(f, ij)
except tv.RouteError as e:
    sys.exit(f"no route to node ({ij[0]}, {ij[1]}): {e}")
trip = int(r["arrive_tick"][-1]) - int(r["arrive_tick"][0])
print(f"route to node ({ij[0]}, {ij[1]}): {len(r['i'])} nodes, {r['length_m'][-1] / 1000.0:.2f} km; trip {trip / 3600.0:.2f} h, of "
      f"which {r['total_wait_ticks'] / 3600.0:.2f} h waiting; longest single wait {r['longest_wait_ticks'] / 3600.0:.2f} h")
if a.route:
    tv.timed_route_csv(r, a.route, ticks_per_hour=3600.0)
    print(f"wrote {a.route}")
rt.close()
if dem_buf is not None:
    dem_buf.free()
