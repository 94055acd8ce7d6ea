#!/usr/bin/env python3
"""Polygons of a GeoJSON file burnt into a label table of a window: zones that come back from a GIS,
put onto the lattice again for zonal statistics, traverse penalties, proximity maps and region reach.

  python tools/rasterise.py --geojson zones.geojson --window 21515 0 127 3840 12 1 --out labels.npy --csv cover.csv
Every Polygon or MultiPolygon Feature (or bare geometry) is one polygon, numbered in the file's order; a MultiPolygon's parts
are rings of the same polygon.  Coordinates are (longitude, latitude) degrees; longitude is read as continuous along a ring, so a
ring across the seam may leave +-180 or jump by 360.  --subcell-bits S (default 4) quantises every vertex to 2^-S of a cell.
--rule evenodd (default: GeoJSON ring orientation is not reliable) or nonzero; --order first (default: the least polygon number
wins where polygons overlap) or last (the painter's order).  A geometry of another type (the MultiLineString that
tools/region_outlines.py writes for a region that winds round the window) keeps its number and covers nothing.
--out FILE gets the (rows, cols) int32 label table, -1 where no polygon covers the node's centre.  --csv FILE gets one row per
polygon: polygon, nodes, area_km2, owned_nodes, owned_area_km2, row_min, row_max, first_node."""
import argparse, csv, json, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np


def polygons_of(doc):
    """([polygon: [ring: [(lat, lon), ...]]], the numbers of the geometries that are no polygons) of a parsed GeoJSON document: a
    FeatureCollection, a Feature or a geometry."""
    kind = doc.get("type")
    items = doc["features"] if kind == "FeatureCollection" else [doc]
    out, skipped = [], []
    for k, item in enumerate(items):
        geom = item.get("geometry") if item.get("type") == "Feature" else item
        gtype = (geom or {}).get("type")
        if gtype == "Polygon":
            parts = [geom["coordinates"]]
        elif gtype == "MultiPolygon":
            parts = geom["coordinates"]
        else:
            parts = []
            skipped.append(k)
        out.append([[(float(pt[1]), float(pt[0])) for pt in ring] for part in parts for ring in part if len(ring)])
    return out, skipped


def cover_rows(cover, unit_m2):
    """The CSV's rows: polygon, nodes, area_km2, owned_nodes, owned_area_km2, row_min, row_max, first_node."""
    for p, c in enumerate(cover):
        yield [p, int(c["count"]), repr(float(c["weight"]) * unit_m2 / 1e6), int(c["owned"]), repr(float(c["owned_weight"]) * unit_m2 / 1e6),
               int(c["i_min"]), int(c["i_max"]), int(c["first_at"])]


def main():
    from moonrtx_amd import regions as rg
    from moonrtx_amd.renderer import MoonRT
    from moonrtx_amd.traverse import window_dict
    import predicate_args
    ap = argparse.ArgumentParser(description="GeoJSON polygons burnt into a label table of a window, with one CSV row per polygon.")
    ap.add_argument("--geojson", required=True, help="Polygon and MultiPolygon features, one polygon per feature")
    predicate_args.add_window(ap)
    ap.add_argument("--out", help=".npy: the (rows, cols) int32 label table")
    ap.add_argument("--csv", help="one row per polygon")
    ap.add_argument("--rule", default="evenodd", choices=("evenodd", "nonzero"))
    ap.add_argument("--order", default="first", choices=("first", "last"))
    ap.add_argument("--subcell-bits", type=int, default=4)
    ap.add_argument("--radius-m", type=float, default=1737400.0)
    ap.add_argument("--unit-m2", type=float, default=1.0, help="the unit areas are counted in (a node's area must fit 32 bits of it)")
    a = ap.parse_args()
    if not 4 <= len(a.window) <= 6:
        ap.error("--window takes ROW0 COL0 ROWS COLS [STRIDE [WRAP]]")
    if not a.out and not a.csv:
        ap.error("give --out, --csv or both")
    w = window_dict(a.window)
    H, W = a.dem_size
    with open(a.geojson) as f:
        polys, skipped = polygons_of(json.load(f))
    for k in skipped:
        print(f"geometry {k} is no Polygon or MultiPolygon: polygon {k} covers nothing", file=sys.stderr)
    pg = rg.Polygons.from_latlon(w, (H, W), polys, a.subcell_bits)
    weights = rg.row_weights(w, (H, W), a.radius_m, a.unit_m2)
    rt = MoonRT(16, 16, device=0)
    st = {}
    labels, cover = rt.rasterise(pg, (w["rows"], w["cols"]), bool(w["wrap"]), a.rule, a.order, weights, stats=st)
    rt.close()
    for path in (a.out, a.csv):
        if path:
            os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    if a.out:
        np.save(a.out, labels)
    if a.csv:
        with open(a.csv, "w", newline="") as f:
            out = csv.writer(f)
            out.writerow(["polygon", "nodes", "area_km2", "owned_nodes", "owned_area_km2", "row_min", "row_max", "first_node"])
            out.writerows(cover_rows(cover, a.unit_m2))
    print(f"{w['rows']}x{w['cols']} nodes{', wrapped' if w['wrap'] else ''}: {pg.n_polygons} polygons, {len(pg)} rings, "
          f"{pg.vertices.shape[0]} vertices, {st['crossings']} crossings, {int((labels >= 0).sum())} nodes covered; "
          f"{st['kernel_ms']:.2f} ms in {st['launches']} launches; wrote {', '.join(p for p in (a.out, a.csv) if p)}")


if __name__ == "__main__":
    main()
