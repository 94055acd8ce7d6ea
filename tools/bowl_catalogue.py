#!/usr/bin/env python3
"""The nested closed bowls of a window of the DEM, headless: every crater, the craters on its floor and
the basin around it, each with its own spill point; or, with --peaks, every summit with its key col, prominence and parent peak.

  python tools/bowl_catalogue.py --window 20000 30000 1024 1024 --min-depth-m 5 --min-area-km2 1 --csv bowls.csv \\
      --labels bowls_labels.npy
  python tools/bowl_catalogue.py --window 21515 0 127 3840 12 1 --peaks --min-depth-m 100 --csv polar_peaks.csv
--window, --unit-m, --unit-m2 and --outlets as in tools/depression_catalogue.py.  --csv gets one row per bowl at least
--min-depth-m deep and of at least --min-area-km2, in the order of the tree (a child before its parent): bowl, parent (the nearest
kept ancestor, or -1), level (the number of kept ancestors), floor_lat, floor_lon, floor_m, spill_lat, spill_lon, spill_m,
depth_m, area_km2, volume_m3, leaves.  With --peaks the same columns are called peak, parent, level, summit_lat, summit_lon,
summit_m, col_lat, col_lon, col_m, prominence_m, area_km2, volume_m3, summits.  --labels gets the (rows, cols) int32 table of
every node's innermost kept bowl as the row number of the CSV (-1 elsewhere), for tools/region_outlines.py and
tools/proximity_map.py.  Synthetic LOLA-like DEM unless --elevation-file is given."""
import argparse, csv, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np

HEADER = ["bowl", "parent", "level", "floor_lat", "floor_lon", "floor_m", "spill_lat", "spill_lon", "spill_m", "depth_m", "area_km2",
          "volume_m3", "leaves"]
PEAK_HEADER = ["peak", "parent", "level", "summit_lat", "summit_lon", "summit_m", "col_lat", "col_lon", "col_m", "prominence_m",
               "area_km2", "volume_m3", "summits"]


def catalogue_rows(tree, keep, lat, lon, unit_m2):
    """The CSV's rows of the kept bowls of a basins.BowlTree made with unit_m and row weights in units of unit_m2; lat (rows,)
    and lon (cols,) are the node axes in degrees.  A bowl that never spills gets empty spill and depth columns."""
    r = tree.records
    cols = tree.z.shape[1]
    keep = np.asarray(keep, bool)
    nearest = tree.target(keep, innermost=True)
    above = np.where(r["parent"] >= 0, nearest[np.maximum(r["parent"], 0)], -1)      # the nearest kept bowl strictly above
    level = np.zeros(tree.n, np.int64)
    for b in range(tree.n - 1, -1, -1):
        if above[b] >= 0:
            level[b] = level[above[b]] + 1
    at = lambda v: (repr(float(lat[v // cols])), repr(float(lon[v % cols])))
    for b in np.flatnonzero(keep).tolist():
        t = r[b]
        spilled = int(t["spill_at"]) >= 0
        spill = (*at(int(t["spill_at"])), repr(int(t["spill_level"]) * tree.unit_m)) if spilled else ("", "", "")
        depth = repr(abs(int(t["spill_level"]) - int(t["floor_level"])) * tree.unit_m) if spilled else ""
        yield [b, int(above[b]), int(level[b]), *at(int(t["floor_at"])), repr(int(t["floor_level"]) * tree.unit_m), *spill, depth,
               repr(int(t["weight"]) * unit_m2 / 1e6), repr(int(t["volume"]) * unit_m2 * tree.unit_m), int(t["n_leaves"])]


def write_csv(path, header, rows):
    with open(path, "w", newline="") as f:
        out = csv.writer(f)
        out.writerow(header)
        out.writerows(rows)


def main():
    from moonrtx_amd import basins as bs
    from moonrtx_amd import regions as rg
    from moonrtx_amd.renderer import MoonRT, synth_ldem, dem_from_ldem
    from moonrtx_amd.traverse import window_dict
    ap = argparse.ArgumentParser(description="A catalogue of the nested closed bowls, or of the peaks, of a DEM window.")
    ap.add_argument("--window", type=int, nargs="+", required=True, metavar="N", help="ROW0 COL0 ROWS COLS [STRIDE [WRAP]] in DEM texels")
    ap.add_argument("--connectivity", type=int, default=8, choices=(4, 8))
    ap.add_argument("--unit-m", type=float, default=0.01, help="the unit heights are counted in")
    ap.add_argument("--unit-m2", type=float, default=1.0, help="the unit areas are counted in (a node's area must fit 32 bits of it)")
    ap.add_argument("--min-depth-m", type=float, default=0.0, help="the least depth, or with --peaks prominence, of a row")
    ap.add_argument("--min-area-km2", type=float, default=0.0)
    ap.add_argument("--peaks", action="store_true", help="summits, key cols and prominences instead of floors, spills and depths")
    ap.add_argument("--outlets", default=None, metavar="MASK.npy", help="(rows, cols): nonzero nodes are outlets too")
    ap.add_argument("--downscale", type=int, default=2)
    ap.add_argument("--dem-size", type=int, nargs=2, default=None, help="synthetic DEM (h, w); default 46080/downscale x 92160/downscale")
    ap.add_argument("--elevation-file", default=None)
    ap.add_argument("--csv", default=None, help="one row per kept bowl")
    ap.add_argument("--labels", default=None, help=".npy of every node's innermost kept bowl")
    a = ap.parse_args()
    if not 4 <= len(a.window) <= 6:
        ap.error("--window takes ROW0 COL0 ROWS COLS [STRIDE [WRAP]]")
    if not (a.csv or a.labels):
        ap.error("give at least one of --csv and --labels")
    w = window_dict(a.window)
    outlets = None
    if a.outlets:
        outlets = np.load(a.outlets)
        if outlets.shape != (w["rows"], w["cols"]):
            sys.exit(f"{a.outlets} is {outlets.shape}: the window has {w['rows']} x {w['cols']} nodes")
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
    radius_m = 1737400.0 * float(radius_scale)
    heights_m = (rt.traverse_heights(w).astype(np.float64) - 1.0) * radius_m
    weights = rg.row_weights(w, (dh, dw), radius_m, a.unit_m2)
    st = {}
    tree = rt.bowls(bs.quantise_heights(heights_m, a.unit_m), outlets=outlets, connectivity=a.connectivity, wrap=bool(w["wrap"]),
                    invert=a.peaks, row_weights=weights, unit_m=a.unit_m, stats=st)
    lat, lon, _ = rt.traverse_nodes(w)
    rt.close()
    if dem_buf is not None:
        dem_buf.free()
    keep = tree.select(min_depth_m=a.min_depth_m, min_area=a.min_area_km2 * 1e6 / a.unit_m2)
    for path in (a.csv, a.labels):
        if path:
            os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    if a.csv:
        write_csv(a.csv, PEAK_HEADER if a.peaks else HEADER, catalogue_rows(tree, keep, lat, lon, a.unit_m2))
    if a.labels:
        np.save(a.labels, tree.relabel(keep)[0])
    print(f"{w['rows']}x{w['cols']} nodes, {a.connectivity}-connected{', wrapped' if w['wrap'] else ''}: {tree.n} "
          f"{'peaks' if a.peaks else 'bowls'}, {len(tree.roots())} of them outermost, {int(keep.sum())} kept at {a.min_depth_m:g} m and "
          f"{a.min_area_km2:g} km^2; {st['kernel_ms']:.2f} ms in {st['launches']} launches, {st['rounds']} merge rounds; wrote "
          f"{', '.join(p for p in (a.csv, a.labels) if p)}")


if __name__ == "__main__":
    main()
