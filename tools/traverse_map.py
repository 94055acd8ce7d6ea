#!/usr/bin/env python3
"""Least-cost rover traverses over the terrain, headless: the cost field over a window of the DEM's
texel lattice from one or more starts, and the route to one target.

  python tools/traverse_map.py --window 20000 30000 1024 1024 --start -68 56 --to -72 60 --max-slope 20 --climb 8 \\
      --out cost.npy --route route.csv
  python tools/traverse_map.py --window 21515 0 127 3840 12 1 --start -89.4 -137 --to -80 40 --out cost.npy
  python tools/traverse_map.py --window 19400 0 256 1024 --start -62 -179 --to -63 -175 --sight -62 -179 20000 \\
      --out cost.npy --route route.csv
--window ROW0 COL0 ROWS COLS [STRIDE [WRAP]] is a block of DEM texels (rows from the north, columns from -180), every STRIDE-th
one; WRAP 1 (with COLS x STRIDE = the DEM's width) joins its last column to its first, for caps around a pole.  Starts and the
target snap to their nearest node.  --sight OBS_LAT OBS_LON OBS_H closes every node that does not see an observer raised
OBS_H metres (a viewshed over the same nodes).  --footprint M closes every node whose slope over a vehicle footprint M metres
across (MoonRT.relief) exceeds --max-slope and makes steeper ground dearer; with it, --max-rms M does the same for the
roughness about the footprint's plane.  The .npy holds the (rows, cols) float64 costs (+inf: unreachable); the CSV the
route, one node per line.  Synthetic LOLA-like DEM unless --elevation-file is given; heights are metres on the DEM's own
radius (1737.4 km x its radius_scale)."""
import argparse, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
from moonrtx_amd import traverse as tv
from moonrtx_amd.renderer import MoonRT, synth_ldem, dem_from_ldem
from moonrtx_amd.scene import named_scene

ap = argparse.ArgumentParser()
ap.add_argument("--window", type=int, nargs="+", required=True, metavar="N",
                help="ROW0 COL0 ROWS COLS [STRIDE [WRAP]] in DEM texels")
ap.add_argument("--start", type=float, nargs=2, action="append", required=True, metavar=("LAT", "LON"))
ap.add_argument("--to", type=float, nargs=2, default=None, metavar=("LAT", "LON"))
ap.add_argument("--max-slope", type=float, default=20.0, help="degrees")
ap.add_argument("--climb", type=float, default=8.0, help="metres of effort per metre climbed")
ap.add_argument("--descent", type=float, default=0.0, help="metres of effort per metre descended")
ap.add_argument("--sight", type=float, nargs=3, default=None, metavar=("OBS_LAT", "OBS_LON", "OBS_H"))
ap.add_argument("--target-height", type=float, default=2.0, help="the rover's antenna height for --sight, metres")
ap.add_argument("--footprint", type=float, default=None, metavar="M",
                help="vehicle footprint, metres: slope (and --max-rms) limits at that scale")
ap.add_argument("--max-rms", type=float, default=None, metavar="M", help="roughness limit over --footprint, metres")
ap.add_argument("--downscale", type=int, default=2)
ap.add_argument("--dem-size", type=int, nargs=2, default=None, help="synthetic DEM (h, w); default 46080/downscale x 92160/downscale")
ap.add_argument("--elevation-file", default=None)
ap.add_argument("--out", default="cost.npy")
ap.add_argument("--route", default=None, help="CSV of the route to --to")
a = ap.parse_args()
if not 4 <= len(a.window) <= 6:
    ap.error("--window takes ROW0 COL0 ROWS COLS [STRIDE [WRAP]]")
if a.route and a.to is None:
    ap.error("--route needs --to")
if a.max_rms is not None and a.footprint is None:
    ap.error("--max-rms needs --footprint")

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
rt.apply_scene(named_scene("S1", 16, 16))      # the march parameters the viewshed of --sight uses
rt.set_params(flags=0)
radius_m = 1737400.0 * float(radius_scale)
window = tuple(a.window)
penalty = None
if a.sight is not None:
    _, _, grid = rt.traverse_nodes(window)
    view = rt.viewshed(tuple(a.sight), target_height_m=a.target_height, radius_m=radius_m, **grid)
    penalty = tv.penalty_from_viewshed(view)
    print(f"line of sight to {tuple(a.sight)}: {float(np.isfinite(penalty).mean()):.4f} of the nodes stay open")
if a.footprint is not None:
    relief = rt.relief(window[:5], footprint_m=a.footprint, radius_m=radius_m)
    hazard = tv.penalty_from_slope(relief, a.max_slope)
    if a.max_rms is not None:
        hazard = np.maximum(hazard, tv.penalty_from_roughness(relief, a.max_rms))
    penalty = hazard if penalty is None else np.where(np.isinf(penalty), penalty, hazard)
    print(f"{a.footprint:g} m footprint: {float(np.isfinite(penalty).mean()):.4f} of the nodes stay open")
st = {}
f = rt.traverse(window, np.array(a.start, np.float64), penalty=penalty, max_slope_deg=a.max_slope, climb_cost=a.climb,
                descent_cost=a.descent, radius_m=radius_m, stats=st)
os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
np.save(a.out, f.cost)
print(f"{f.cost.shape[0]}x{f.cost.shape[1]} nodes: {float(np.isfinite(f.cost).mean()):.4f} reachable; {st['kernel_ms']:.2f} ms of "
      f"kernels, {st['launches']} relaxation launches, {st['tile_visits']} tile visits; wrote {a.out}")
if a.to is not None:
    ij = rt.snap_to_nodes(window, [a.to[0]], [a.to[1]])[0]
    try:
        r = tv.route(f, ij)
    except tv.RouteError as e:
        sys.exit(f"no route to node ({ij[0]}, {ij[1]}): {e}")
    print(f"route to node ({ij[0]}, {ij[1]}): {len(r['i'])} nodes, {r['length_m'][-1] / 1000.0:.2f} km, cost "
          f"{r['cost'][-1] / 1000.0:.2f} km of effort, climbs {np.maximum(np.diff(r['height_m']), 0).sum():.0f} m")
    if a.route:
        tv.route_csv(r, a.route)
        print(f"wrote {a.route}")
rt.close()
if dem_buf is not None:
    dem_buf.free()
