#!/usr/bin/env python3
"""The distinct regions of a saved per-node map: which nodes belong together, where each region is
and how large.

  python tools/region_catalogue.py --map stats.npy --channel 1 --below 0.0 --window 21515 0 127 3840 12 1 \\
      --dem-size 23040 46080 --min-area-km2 1 --out labels.npy --csv shadows.csv
  python tools/region_catalogue.py --map temps.npy --channel 0 --below 110 --window 21515 0 127 3840 12 1 --connectivity 8
  python tools/region_catalogue.py --map ice.npy --channel 0 --between 0 1 --window 20000 30000 1024 1024
--map is a (rows, cols) or (rows, cols, channels) array over the nodes of --window ROW0 COL0 ROWS COLS [STRIDE [WRAP]], a
block of DEM texels as tools/traverse_map.py takes it (WRAP 1 joins the last column to the first).  The set is the nodes whose
--channel lies --below X (<=), --above X (>=) or --between A B, compared as float32; a NaN is outside.  A node's area is that
of its lattice cell on a sphere of --radius-m, counted in whole units of --unit-m2, so a region's area is an exact sum.
--out gets the (rows, cols) int32 labels (-1: outside the set; regions below --min-area-km2 are dropped and the rest
renumbered); --csv one line per region, largest first: rank, area in km^2 and in units, nodes, the centroid's latitude and
longitude, the row extent and the column extent.  The total area of the listed regions is printed: the exactly rounded sum
(math.fsum) of the km^2 column, and the sum of the units column, an integer.
--stats FILE[:CH] NAME (repeatable) adds what is inside every listed region of channel CH (default 0)
of another map over the same window: NAME_min, NAME_max, NAME_mean (over the nodes), NAME_area_mean (over the area) and
NAME_min_lat, NAME_min_lon, where the minimum lies; means are exact sums of values rounded to 1 / --stats-scale.  --shape adds
perimeter_km (cell sides on a sphere, counted in whole units of --side-unit-m) and holes (1 - the Euler number in
--connectivity; a region that winds round a wrapped window reads one more)."""
import argparse, csv, math, os, sys
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
ap.add_argument("--connectivity", type=int, default=4, choices=(4, 8))
ap.add_argument("--min-area-km2", type=float, default=0.0)
ap.add_argument("--radius-m", type=float, default=1737400.0)
ap.add_argument("--unit-m2", type=float, default=1.0, help="the unit areas are counted in (a node's area must fit 32 bits of it)")
ap.add_argument("--stats", nargs=2, action="append", default=[], metavar=("FILE[:CH]", "NAME"), help="zonal statistics of another map")
ap.add_argument("--stats-scale", type=float, default=1024.0, help="values are summed in units of 1 / this")
ap.add_argument("--shape", action="store_true", help="perimeter_km and holes")
ap.add_argument("--side-unit-m", type=float, default=1.0, help="the unit cell sides are counted in")
ap.add_argument("--out", default="labels.npy")
ap.add_argument("--csv", default="regions.csv")
a = ap.parse_args()
if not 4 <= len(a.window) <= 6:
    ap.error("--window takes ROW0 COL0 ROWS COLS [STRIDE [WRAP]]")
w = window_dict(a.window)
H, W = a.dem_size
field = predicate_args.load_map(a.map, w)
if field.shape[2] > 16:           # the library compares one channel of at most 16
    field, a.channel = field[:, :, a.channel:a.channel + 1], 0
lo, hi = predicate_args.bounds(a)
weights = rg.row_weights(w, (H, W), a.radius_m, a.unit_m2)
rt = MoonRT(16, 16, device=0)
st = {}
m = rt.regions(field=np.ascontiguousarray(field, np.float32), channel=a.channel, lo=lo, hi=hi, connectivity=a.connectivity,
               wrap=bool(w["wrap"]), row_weights=weights, unit_m2=a.unit_m2, stats=st)
kept = m.filter(min_area=a.min_area_km2 * 1e6)
extra = []                      # (column name, one value per kept region)
for spec, name in a.stats:
    path, _, ch = spec.rpartition(":") if spec.rpartition(":")[2].isdigit() else (spec, "", "0")
    other = np.load(path)
    if other.ndim == 2:
        other = other[:, :, None]
    if other.ndim != 3 or other.shape[:2] != (w["rows"], w["cols"]) or not 0 <= int(ch) < other.shape[2]:
        sys.exit(f"{path} is {other.shape}: the window has {w['rows']} x {w['cols']} nodes and channel {ch} is asked for")
    z = kept.zonal(rt, np.ascontiguousarray(other[:, :, int(ch)], np.float32), row_weights=weights, scale=a.stats_scale)[:, 0]
    at = np.maximum(z["min_at"], 0)
    none = z["count"] == 0
    extra += [(f"{name}_min", z["min"].astype(np.float64)), (f"{name}_max", z["max"].astype(np.float64)),
              (f"{name}_mean", rg.zonal_mean(z, a.stats_scale)), (f"{name}_area_mean", rg.zonal_area_mean(z, a.stats_scale)),
              (f"{name}_min_lat", np.where(none, np.nan, 90.0 - (w["row0"] + (at // w["cols"]) * w["stride"] + 0.5) * (180.0 / H))),
              (f"{name}_min_lon", np.where(none, np.nan, -180.0 + ((w["col0"] + (at % w["cols"]) * w["stride"]) % W + 0.5) * (360.0 / W)))]
if a.shape:
    ew, ns = rg.side_weights(w, (H, W), a.radius_m, a.side_unit_m)
    sh = kept.shapes(rt, a.connectivity, ew, ns)
    extra += [("perimeter_km", sh["perimeter"].astype(np.float64) * (a.side_unit_m / 1e3)), ("holes", kept.holes(sh)[0])]
rt.close()
s = w["stride"]
lat = 90.0 - (w["row0"] + np.arange(w["rows"]) * s + 0.5) * (180.0 / H)
lon = -180.0 + ((w["col0"] + np.arange(w["cols"]) * s) % W + 0.5) * (360.0 / W)
area = kept.area_m2() / 1e6
cen = kept.centroids(lat, lon)
for path in (a.out, a.csv):
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
np.save(a.out, kept.labels)
with open(a.csv, "w", newline="") as f:
    out = csv.writer(f)
    out.writerow(["rank", "region", "area_km2", "area_units", "nodes", "lat", "lon", "row_min", "row_max", "col_west", "col_east"] +
                 [name for name, _ in extra])
    t = kept.table
    for rank, k in enumerate(kept.largest(kept.n), 1):
        west, east = int(t["root_j"][k]) + int(t["dj_min"][k]), int(t["root_j"][k]) + int(t["dj_max"][k])
        if w["wrap"]:
            west, east = west % w["cols"], east % w["cols"]
        out.writerow([rank, int(k), repr(float(area[k])), int(t["weight"][k]), int(t["count"][k]), f"{cen[k, 0]:.6f}", f"{cen[k, 1]:.6f}",
                      int(t["i_min"][k]), int(t["i_max"][k]), west, east] +
                     [int(v[k]) if v.dtype.kind == "i" else repr(float(v[k])) for _, v in extra])
print(f"{w['rows']}x{w['cols']} nodes, {a.connectivity}-connected{', wrapped' if w['wrap'] else ''}: {m.n} regions over "
      f"{int(m.table['count'].sum())} nodes, {kept.n} of at least {a.min_area_km2:g} km^2; {st['label_ms']:.2f} ms to label in "
      f"{st['label_launches']} launches, {st['catalogue_ms']:.2f} ms for the catalogue")
print(f"total area {math.fsum(area.tolist())!r} km^2 = {int(kept.table['weight'].astype(object).sum()) if kept.n else 0} units of "
      f"{a.unit_m2:g} m^2; wrote {a.out} and {a.csv}")
