#!/usr/bin/env python
"""Distances to the nearest node of a set, buffers, and the reach of its regions.

  python tools/proximity_map.py --map stats.npy --channel 1 --below 0.0 --window 21515 0 127 3840 12 1 \\
      --out prox.npy --buffer 5000 --buffer-out near_shadow.npy --csv shadows.csv
  python tools/proximity_map.py --map ice.npy --below 1.0 --to-map hazard.npy --to-below 0.5 --window 21515 0 127 3840 12 1

--map is a (rows, cols) or (rows, cols, channels) .npy over the window; --below X, --above X or --between A B select the set
(the options of region_catalogue.py).  Distances are straight lines between node positions on a sphere of --radius-m, or on
the terrain with --dem FILE.npy (an (H, W) array of heights in metres above the sphere, which also gives the DEM's size),
exact in whole units of --unit-m.  --out gets (rows, cols, 3) float64: the distance in metres to the nearest node of the set
(inf when the set is empty), that node's index i cols + j and its region's number (-1: none).  --buffer M with --buffer-out
saves the boolean mask of the nodes within M metres of the set.  --csv gets one line per region of the set: the radius in
metres of the largest circle that fits in it and the latitude and longitude of its centre (nodes beyond the window's edge do
not count as outside).  With --to-map OTHER.npy and --to-channel, --to-below / --to-above / --to-between a second set is
selected and the CSV also holds each region's closest approach to it in metres, with the end point in the region and the one
in the second set."""
import argparse, csv, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
from moonrtx_amd import regions as rg
from moonrtx_amd.renderer import MoonRT
from moonrtx_amd.traverse import window_dict
import predicate_args

ap = argparse.ArgumentParser()
ap.add_argument("--map", required=True, help=".npy, (rows, cols) or (rows, cols, channels)")
ap.add_argument("--channel", type=int, default=0)
predicate_args.add_predicate(ap)
predicate_args.add_window(ap)
ap.add_argument("--dem", help=".npy of (H, W) heights in metres above the sphere: distances follow the terrain's nodes")
ap.add_argument("--connectivity", type=int, default=4, choices=(4, 8))
ap.add_argument("--radius-m", type=float, default=1737400.0)
ap.add_argument("--unit-m", type=float, default=0.01, help="the unit positions are rounded to (a coordinate must fit 2^29 of it)")
ap.add_argument("--out", default="prox.npy")
ap.add_argument("--buffer", type=float, metavar="M")
ap.add_argument("--buffer-out", default="buffer.npy")
ap.add_argument("--to-map", help="a second map: the CSV gains each region's closest approach to its set")
ap.add_argument("--to-channel", type=int, default=0)
predicate_args.add_predicate(ap, "to-", required=False)
ap.add_argument("--csv", default="regions.csv")
a = ap.parse_args()
if not 4 <= len(a.window) <= 6:
    ap.error("--window takes ROW0 COL0 ROWS COLS [STRIDE [WRAP]]")
w = window_dict(a.window)
H, W = a.dem_size
heights = None
if a.dem:
    dem = np.load(a.dem)
    if dem.ndim != 2:
        sys.exit(f"{a.dem} is {dem.shape}: a DEM is (H, W)")
    H, W = dem.shape
    rows_at = w["row0"] + np.arange(w["rows"]) * w["stride"]
    if rows_at[0] < 0 or rows_at[-1] >= H:
        sys.exit(f"the window's rows leave the DEM's {H} rows")
    heights = dem[np.ix_(rows_at, (w["col0"] + np.arange(w["cols"]) * w["stride"]) % W)].astype(np.float64)
field = predicate_args.load_map(a.map, w)
if not 0 <= a.channel < field.shape[2]:
    sys.exit(f"{a.map} has {field.shape[2]} channels")
field = field[:, :, a.channel:a.channel + 1]
lo, hi = predicate_args.bounds(a)
other = None
if a.to_map:
    if a.to_below is None and a.to_above is None and a.to_between is None:
        ap.error("--to-map needs one of --to-below, --to-above and --to-between")
    other = predicate_args.load_map(a.to_map, w)
    if not 0 <= a.to_channel < other.shape[2]:
        sys.exit(f"{a.to_map} has {other.shape[2]} channels")
    lo2, hi2 = predicate_args.bounds(a, "to-")
    x = other[:, :, a.to_channel].astype(np.float32)
    second = np.where((x >= np.float32(lo2)) & (x <= np.float32(hi2)), 0, -1).astype(np.int32)
pos = rg.node_positions(w, (H, W), a.radius_m, a.unit_m, heights)
rt = MoonRT(16, 16, device=0)
st = {}
m = rt.regions(field=np.ascontiguousarray(field, np.float32), channel=0, lo=lo, hi=hi, connectivity=a.connectivity,
               wrap=bool(w["wrap"]))
prox = m.proximity(rt, pos, to="set", unit_m=a.unit_m, stats=st)
radius, centre = m.inscribed(rt, pos, a.unit_m)
approach = m.reach(rt, rt.proximity(second, pos, to="set", unit_m=a.unit_m)) if other is not None else None
rt.close()
for path in (a.out, a.csv) + ((a.buffer_out,) if a.buffer is not None else ()):
    d = os.path.dirname(os.path.abspath(path))
    if not os.path.isdir(d):
        sys.exit(f"the directory of {path} does not exist")
np.save(a.out, np.stack([prox.chord_m(), prox.nearest.astype(np.float64), prox.nearest_label(m.labels).astype(np.float64)], -1))
if a.buffer is not None:
    np.save(a.buffer_out, prox.within(a.buffer))


def lat_lon(node):
    """The latitude and longitude in degrees of a node index, as repr strings; empty for -1."""
    if node < 0:
        return ["", ""]
    i, j = divmod(int(node), w["cols"])
    return [repr(90.0 - (w["row0"] + i * w["stride"] + 0.5) * (180.0 / H)),
            repr(-180.0 + ((w["col0"] + j * w["stride"]) % W + 0.5) * (360.0 / W))]


with open(a.csv, "w", newline="") as f:
    out = csv.writer(f)
    out.writerow(["region", "nodes", "inscribed_radius_m", "centre_node", "centre_lat", "centre_lon"] +
                 (["approach_m", "from_node", "from_lat", "from_lon", "to_node", "to_lat", "to_lon"] if approach is not None else []))
    for k in range(m.n):
        line = [k, int(m.table["count"][k]), repr(float(radius[k])), int(centre[k])] + lat_lon(centre[k])
        if approach is not None:
            r = approach[k]
            none = r["d2_min"] == rg.NO_FEATURE
            line += [repr(float("inf") if none else float(np.sqrt(np.float64(r["d2_min"])) * a.unit_m)), int(r["min_at"])] + \
                lat_lon(r["min_at"]) + [int(r["min_nearest"])] + lat_lon(r["min_nearest"])
        out.writerow(line)
print(f"{w['rows']}x{w['cols']} nodes, {m.n} regions over {int(m.table['count'].sum())} nodes: {st['kernel_ms']:.2f} ms and "
      f"{st['pairs']} distance evaluations for the map in {st['launches']} launches")
