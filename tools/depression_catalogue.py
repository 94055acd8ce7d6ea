#!/usr/bin/env python3
"""The closed depressions of a window of the DEM, headless: craters, pits and the bowls inside them,
each with the level up to which it is closed, its depth, its pour point and what it holds.

  python tools/depression_catalogue.py --window 20000 30000 1024 1024 --min-depth-m 5 --min-area-km2 1 \\
      --fill fill.npy --depth depth.npy --csv basins.csv --labels basins_labels.npy
  python tools/depression_catalogue.py --window 21515 0 127 3840 12 1 --csv polar_basins.csv
--window ROW0 COL0 ROWS COLS [STRIDE [WRAP]] is a block of DEM texels as in tools/traverse_map.py; the heights are those of
MoonRT.traverse_heights, (D - 1) x radius_m, rounded to whole units of --unit-m.  The window's border rows and, without WRAP, its
border columns are outlets, and so is every nonzero node of --outlets MASK.npy (nodata, a chosen sink, a window's open side).
--fill and --depth get the (rows, cols) int32 fill levels and depths in units of --unit-m.  --csv gets one row per depression
deeper than --min-depth-m and of at least --min-area-km2, the largest volume first: basin, area_km2, nodes, level_m,
depth_max_m, deepest_lat, deepest_lon, pour_lat, pour_lon, volume_m3.  --labels gets the (rows, cols) int32 label table of the
rows' basins (-1 elsewhere) for tools/region_outlines.py and tools/proximity_map.py.  Synthetic LOLA-like DEM unless
--elevation-file is given."""
import argparse, csv, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np

HEADER = ["basin", "area_km2", "nodes", "level_m", "depth_max_m", "deepest_lat", "deepest_lon", "pour_lat", "pour_lon", "volume_m3"]


def catalogue_rows(table, cols, lat, lon, unit_m, unit_m2):
    """The CSV's rows of a (n,) basins.BASIN_DTYPE table made with row weights in units of unit_m2 over heights in units of
    unit_m: the largest volume first (equal volumes: the lower basin number first); lat (rows,) and lon (cols,) are the node
    axes in degrees.  A basin without a pour point (it covers the whole lattice) gets empty pour columns."""
    order = sorted(range(len(table)), key=lambda r: (-int(table[r]["volume"]), r))
    at = lambda v: (repr(float(lat[v // cols])), repr(float(lon[v % cols]))) if v >= 0 else ("", "")
    for r in order:
        t = table[r]
        yield [r, repr(int(t["weight"]) * unit_m2 / 1e6), int(t["count"]), repr(int(t["level_min"]) * unit_m),
               repr(int(t["depth_max"]) * unit_m), *at(int(t["deepest_at"])), *at(int(t["pour_at"])),
               repr(int(t["volume"]) * unit_m2 * unit_m)]


def write_csv(path, rows):
    with open(path, "w", newline="") as f:
        out = csv.writer(f)
        out.writerow(HEADER)
        out.writerows(rows)


def main():
    from moonrtx_amd import basins as bs
    from moonrtx_amd import regions as rg
    from moonrtx_amd.renderer import MoonRT, synth_ldem, dem_from_ldem
    from moonrtx_amd.traverse import window_dict
    ap = argparse.ArgumentParser(description="Fill levels, depths and a catalogue of the closed depressions of a DEM window.")
    ap.add_argument("--window", type=int, nargs="+", required=True, metavar="N", help="ROW0 COL0 ROWS COLS [STRIDE [WRAP]] in DEM texels")
    ap.add_argument("--connectivity", type=int, default=8, choices=(4, 8))
    ap.add_argument("--unit-m", type=float, default=0.01, help="the unit heights are counted in")
    ap.add_argument("--unit-m2", type=float, default=1.0, help="the unit areas are counted in (a node's area must fit 32 bits of it)")
    ap.add_argument("--min-depth-m", type=float, default=0.0)
    ap.add_argument("--min-area-km2", type=float, default=0.0)
    ap.add_argument("--outlets", default=None, metavar="MASK.npy", help="(rows, cols): nonzero nodes are outlets too")
    ap.add_argument("--downscale", type=int, default=2)
    ap.add_argument("--dem-size", type=int, nargs=2, default=None, help="synthetic DEM (h, w); default 46080/downscale x 92160/downscale")
    ap.add_argument("--elevation-file", default=None)
    ap.add_argument("--fill", default=None, help=".npy of the fill levels")
    ap.add_argument("--depth", default=None, help=".npy of the depths")
    ap.add_argument("--csv", default=None, help="one row per depression")
    ap.add_argument("--labels", default=None, help=".npy of the catalogued basins' labels")
    a = ap.parse_args()
    if not 4 <= len(a.window) <= 6:
        ap.error("--window takes ROW0 COL0 ROWS COLS [STRIDE [WRAP]]")
    if not (a.fill or a.depth or a.csv or a.labels):
        ap.error("give at least one of --fill, --depth, --csv and --labels")
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
    st = {}
    fm = rt.fill_depressions(bs.quantise_heights(heights_m, a.unit_m), outlets=outlets, connectivity=a.connectivity,
                             wrap=bool(w["wrap"]), unit_m=a.unit_m, stats=st)
    weights = rg.row_weights(w, (dh, dw), radius_m, a.unit_m2)
    regions, table = fm.catalogue(rt, row_weights=weights, min_depth_m=a.min_depth_m)
    keep = table["weight"].astype(np.float64) * a.unit_m2 >= a.min_area_km2 * 1e6
    lat, lon, _ = rt.traverse_nodes(w)
    rt.close()
    if dem_buf is not None:
        dem_buf.free()
    for path in (a.fill, a.depth, a.csv, a.labels):
        if path:
            os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    if a.fill:
        np.save(a.fill, fm.fill)
    if a.depth:
        np.save(a.depth, fm.depth())
    new = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
    if a.csv:
        write_csv(a.csv, catalogue_rows(table[keep], w["cols"], lat, lon, a.unit_m, a.unit_m2))
    if a.labels:
        np.save(a.labels, np.concatenate([new, np.array([-1], np.int32)])[regions.labels])
    print(f"{w['rows']}x{w['cols']} nodes, {a.connectivity}-connected{', wrapped' if w['wrap'] else ''}: "
          f"{float((fm.depth() > 0).mean()):.4f} of the nodes lie in {regions.n} depressions, {int(keep.sum())} of them deeper than "
          f"{a.min_depth_m:g} m and of at least {a.min_area_km2:g} km^2; fill {st['kernel_ms']:.2f} ms in {st['launches']} launches, "
          f"{st['visits']} tile visits; wrote {', '.join(p for p in (a.fill, a.depth, a.csv, a.labels) if p)}")


if __name__ == "__main__":
    main()
