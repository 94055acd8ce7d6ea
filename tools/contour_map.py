#!/usr/bin/env python3
"""Contour lines of a window of the DEM or of any saved per-node map, headless: elevation contours of
a landing site, the 110 K isotherm of a temperature map, the 1 m line of an ice map.

  python tools/contour_map.py --window 21515 0 127 3840 12 1 --interval-m 500 --geojson polar_contours.geojson
  python tools/contour_map.py --map temps.npy --channel 0 --unit 0.01 --window 20000 30000 512 512 --levels 110 \\
      --min-vertices 8 --geojson isotherm.geojson --csv isotherm.csv
--window ROW0 COL0 ROWS COLS [STRIDE [WRAP]] is a block of DEM texels as in tools/traverse_map.py.  Without --map the heights
are those of MoonRT.traverse_heights, (D - 1) x radius_m, of a synthetic LOLA-like DEM unless --elevation-file is given; with
--map FILE.npy they are channel --channel of a saved (rows, cols[, channels]) map of that window.  Either way they are rounded to
whole units of --unit (basins.quantise_heights; 0.01 by default, a centimetre of height), and a NaN becomes a void node, at
which lines end.  Levels, in the values' own unit (metres for the DEM): every multiple of --interval-m between the least and
the greatest value, or the list after --levels.  A node is above a level c when its rounded value is >= c, so a line is the
isoline of c less half a unit.  --min-vertices N drops shorter lines.
--geojson FILE gets an RFC 7946 FeatureCollection with one LineString per line, nodes at texel centres, and the properties
line, level, level_index, closed and vertices; a closed line repeats its first position.  Lines run with the higher side on
their right while rows run south.  Longitudes are continuous along a line, so a line across the seam leaves +-180.
--csv FILE gets one row per vertex: line, level, closed, vertex, edge, y, x (node coordinates, x unwrapped), lat, lon."""
import argparse, csv, json, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np

HEADER = ["line", "level", "closed", "vertex", "edge", "y", "x", "lat", "lon"]


def quantise(values, unit):
    """Values as int32 counts of unit (basins.quantise_heights), NaN as a void node."""
    from moonrtx_amd import basins as bs
    from moonrtx_amd import contours as ct
    v = np.asarray(values, np.float64)
    nan = np.isnan(v)
    z = bs.quantise_heights(np.where(nan, 0.0, v), unit)
    z[nan] = ct.VOID
    return z


def level_table(z, unit, interval=None, levels=None):
    """The int32 level table: the multiples of interval (in the values' unit) that the valid values span, or the given
    levels, rounded to whole units, sorted, each once."""
    from moonrtx_amd import contours as ct
    if levels is not None:
        return np.unique(np.rint(np.asarray(levels, np.float64) / unit).astype(np.int64)).astype(np.int32)
    valid = z[z != ct.VOID]
    if valid.size == 0:
        return np.zeros(0, np.int32)
    return ct.levels_for(int(valid.min()), int(valid.max()), max(int(round(interval / unit)), 1))


def kept_lines(cs, min_vertices=0):
    return [r for r in range(len(cs)) if int(cs.lines[r]["n_vertices"]) >= min_vertices]


def feature_collection(cs, window, dem_hw, unit, min_vertices=0):
    """The FeatureCollection (a dict) of a contours.Contours: one LineString per line of at least min_vertices vertices, its
    positions (lon, lat) from Contours.latlon, a closed line's first position repeated at its end."""
    features = []
    for r in kept_lines(cs, min_vertices):
        rec = cs.lines[r]
        ll = cs.latlon(r, window, dem_hw)
        pts = [[float(p[1]), float(p[0])] for p in ll]
        if rec["closed"]:
            pts.append(pts[0])
        props = {"line": r, "level": int(rec["level"]) * unit, "level_index": int(rec["level_index"]), "closed": bool(rec["closed"]),
                 "vertices": int(rec["n_vertices"])}
        features.append({"type": "Feature", "properties": props, "geometry": {"type": "LineString", "coordinates": pts}})
    return {"type": "FeatureCollection", "features": features}


def vertex_rows(cs, window, dem_hw, unit, min_vertices=0):
    """The CSV's rows: line, level, closed, vertex, edge, y, x, lat, lon per vertex."""
    for r in kept_lines(cs, min_vertices):
        rec = cs.lines[r]
        xy, ll, edges = cs.xy(r), cs.latlon(r, window, dem_hw), cs.line(r)
        for k in range(len(edges)):
            yield [r, repr(int(rec["level"]) * unit), int(rec["closed"]), k, int(edges[k]), repr(float(xy[k, 0])), repr(float(xy[k, 1])),
                   repr(float(ll[k, 0])), repr(float(ll[k, 1]))]


def main():
    from moonrtx_amd.renderer import MoonRT, synth_ldem, dem_from_ldem
    from moonrtx_amd.traverse import window_dict
    ap = argparse.ArgumentParser(description="Contour lines of a DEM window or of a saved per-node map as GeoJSON and CSV.")
    ap.add_argument("--window", type=int, nargs="+", required=True, metavar="N", help="ROW0 COL0 ROWS COLS [STRIDE [WRAP]] in DEM texels")
    ap.add_argument("--map", default=None, help=".npy, (rows, cols) or (rows, cols, channels), instead of the DEM's heights")
    ap.add_argument("--channel", type=int, default=0)
    ap.add_argument("--unit", type=float, default=0.01, help="the unit the values are rounded to")
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--interval-m", type=float, metavar="D", help="the contour interval, in the values' unit (metres for the DEM)")
    g.add_argument("--levels", type=float, nargs="+", metavar="C")
    ap.add_argument("--min-vertices", type=int, default=0)
    ap.add_argument("--downscale", type=int, default=2)
    ap.add_argument("--dem-size", type=int, nargs=2, default=None, help="the DEM (h, w) the window counts in; default 46080/downscale x 92160/downscale")
    ap.add_argument("--elevation-file", default=None)
    ap.add_argument("--geojson", help="FeatureCollection, one LineString per line")
    ap.add_argument("--csv", help="one row per vertex")
    a = ap.parse_args()
    if not 4 <= len(a.window) <= 6:
        ap.error("--window takes ROW0 COL0 ROWS COLS [STRIDE [WRAP]]")
    if not a.geojson and not a.csv:
        ap.error("give --geojson, --csv or both")
    if a.interval_m is not None and not a.interval_m > 0.0:
        ap.error("--interval-m must be > 0")
    w = window_dict(a.window)
    rt = MoonRT(16, 16, device=0)
    if a.map:
        import predicate_args
        dh, dw = a.dem_size or (46080 // a.downscale, 92160 // a.downscale)
        values = predicate_args.load_map(a.map, w)[:, :, a.channel]
    else:
        dem_buf = None
        if a.elevation_file:
            from moonrtx_amd.ingest import load_elevation_data
            dem, radius_scale = load_elevation_data(a.elevation_file, a.downscale, device=0)
            dh, dw = dem.shape
            rt.upload_dem(dem)
        else:
            dh, dw = a.dem_size or (46080 // a.downscale, 92160 // a.downscale)
            src = synth_ldem(dh, dw, device=0)
            dem_buf, radius_scale = dem_from_ldem(src, dh, dw, 1, device=0)
            src.free()
            rt.bind_dem(dem_buf, dh, dw)
        values = (rt.traverse_heights(w).astype(np.float64) - 1.0) * (1737400.0 * float(radius_scale))
        if dem_buf is not None:
            dem_buf.free()
    z = quantise(values, a.unit)
    levels = level_table(z, a.unit, a.interval_m, a.levels)
    if levels.size == 0:
        rt.close()
        sys.exit("no level lies between the least and the greatest value")
    st = {}
    cs = rt.contours(z, levels, wrap=bool(w["wrap"]), stats=st)
    rt.close()
    for path in (a.geojson, a.csv):
        if path:
            os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    if a.geojson:
        with open(a.geojson, "w") as f:
            json.dump(feature_collection(cs, w, (dh, dw), a.unit, a.min_vertices), f)
    if a.csv:
        with open(a.csv, "w", newline="") as f:
            out = csv.writer(f)
            out.writerow(HEADER)
            out.writerows(vertex_rows(cs, w, (dh, dw), a.unit, a.min_vertices))
    kept = kept_lines(cs, a.min_vertices)
    print(f"{w['rows']}x{w['cols']} nodes{', wrapped' if w['wrap'] else ''}, {levels.size} levels: {len(cs)} lines "
          f"({int(cs.lines['closed'].sum())} closed), {cs.vertices.shape[0]} vertices, {len(kept)} lines of at least {a.min_vertices}; "
          f"{st['kernel_ms']:.2f} ms in {st['launches']} launches; wrote {', '.join(p for p in (a.geojson, a.csv) if p)}")


if __name__ == "__main__":
    main()
