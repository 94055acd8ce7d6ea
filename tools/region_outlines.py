#!/usr/bin/env python3
"""The outlines of the distinct regions of a saved per-node map: every region's boundary as ordered
rings, for a GIS, an overlay or a planner's keep-out polygons.

  python tools/region_outlines.py --map stats.npy --channel 1 --below 0.0 --window 21515 0 127 3840 12 1 \\
      --min-area-km2 1 --geojson shadows.geojson --csv shadows_vertices.csv
--map, --channel, --below / --above / --between, --window, --dem-size, --connectivity, --min-area-km2, --radius-m and --unit-m2
are tools/region_catalogue.py's.  Vertices are the corners at which a ring turns (--all-vertices: one per boundary side); they
sit on the cell edges, half a row or column spacing off the texel-centre nodes.
--geojson FILE gets an RFC 7946 FeatureCollection with one Feature per region: a Polygon of the outer ring and its holes, with
the properties region, area_km2, nodes, holes and perimeter_km (cell sides on a sphere, in whole units of --side-unit-m).  A
region that winds round a wrapped window has no inside in the plane and is written as a MultiLineString of its rings with
"winds": true.  Longitudes are continuous along a ring, so a ring across the seam leaves +-180.  The GeoJSON lists every ring
from its head backwards, the reverse of the order of the CSV and of the vertex table, so that outer rings run counter-clockwise
and holes clockwise in (longitude, latitude) as RFC 7946 asks.
--csv FILE gets one row per vertex: ring, region, role (outer, hole or winding), y, x (corner coordinates, x unwrapped), lat,
lon."""
import argparse, csv, json, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np


def shoelace(ring):
    """Twice the signed area of a closed ring of (lon, lat) pairs as plain floats: > 0 counter-clockwise."""
    return sum(a[0] * b[1] - b[0] * a[1] for a, b in zip(ring[:-1], ring[1:]))


def feature_collection(ol, latlon, properties):
    """The FeatureCollection (a dict) of a regions.Outlines: latlon (m, 2) float64 per vertex (Outlines.corner_latlon),
    properties {name: one value per label}.  A ring runs with its region on the right while rows run south, so in (lon, lat)
    an outer ring is clockwise and a hole counter-clockwise whatever the labels; RFC 7946 asks for the opposite, so every
    ring is written from its head backwards, and the orientation is asserted, not repaired.  ValueError for a label with more
    than one outer ring (a caller's disconnected label): holes cannot be told apart between them."""
    def coords(r):
        rec = ol.rings[r]
        a, n = int(rec["first"]), int(rec["n_vertices"])
        pts = [[float(latlon[a + k, 1]), float(latlon[a + k, 0])] for k in range(n)]
        pts = [pts[0]] + pts[:0:-1]             # the same ring the other way round, still from its head
        return pts + [pts[0]]
    features = []
    for label in np.unique(ol.rings["label"]).tolist():
        ids = ol.of(label).tolist()
        roles = [ol.role(r) for r in ids]
        props = {k: (v[label].item() if hasattr(v[label], "item") else v[label]) for k, v in properties.items()}
        props["region"] = int(label)
        if "winding" in roles:
            props["winds"] = True
            geom = {"type": "MultiLineString", "coordinates": [coords(r) for r in ids]}
        else:
            if roles.count("outer") != 1:
                raise ValueError(f"label {label} has {roles.count('outer')} outer rings: a polygon needs one connected region "
                                 f"per label (label the map with MoonRT.regions, or split the label)")
            rings = [coords(r) for r in ids]
            assert shoelace(rings[0]) > 0 and all(shoelace(h) < 0 for h in rings[1:]), f"label {label}: ring orientation"
            geom = {"type": "Polygon", "coordinates": rings}
        features.append({"type": "Feature", "properties": props, "geometry": geom})
    return {"type": "FeatureCollection", "features": features}


def vertex_rows(ol, latlon):
    """The CSV's rows: ring, region, role, y, x, lat, lon per vertex."""
    for r in range(len(ol)):
        rec = ol.rings[r]
        a = int(rec["first"])
        for k in range(int(rec["n_vertices"])):
            y, x = ol.vertices[a + k].tolist()
            yield [r, int(rec["label"]), ol.role(r), y, x, repr(float(latlon[a + k, 0])), repr(float(latlon[a + k, 1]))]


def main():
    from moonrtx_amd import regions as rg
    from moonrtx_amd.renderer import MoonRT
    from moonrtx_amd.traverse import window_dict
    import predicate_args
    ap = argparse.ArgumentParser(description="Region outlines of a saved per-node map as GeoJSON and CSV.  The GeoJSON lists every "
                                 "ring from its head backwards (outer rings counter-clockwise in longitude / latitude, RFC 7946), "
                                 "the reverse of the order of the CSV and of the vertex table.")
    ap.add_argument("--map", required=True, help=".npy, (rows, cols) or (rows, cols, channels)")
    ap.add_argument("--channel", type=int, default=0)
    predicate_args.add_predicate(ap)
    predicate_args.add_window(ap)
    ap.add_argument("--connectivity", type=int, default=4, choices=(4, 8))
    ap.add_argument("--all-vertices", action="store_true", help="one vertex per boundary side, not only where a ring turns")
    ap.add_argument("--min-area-km2", type=float, default=0.0)
    ap.add_argument("--radius-m", type=float, default=1737400.0)
    ap.add_argument("--unit-m2", type=float, default=1.0, help="the unit areas are counted in (a node's area must fit 32 bits of it)")
    ap.add_argument("--side-unit-m", type=float, default=1.0, help="the unit cell sides are counted in")
    ap.add_argument("--geojson", help="FeatureCollection; ring order reversed against --csv (see above)")
    ap.add_argument("--csv", help="one row per vertex in the vertex table's order: each ring from its head on, region on the right")
    a = ap.parse_args()
    if not 4 <= len(a.window) <= 6:
        ap.error("--window takes ROW0 COL0 ROWS COLS [STRIDE [WRAP]]")
    if not a.geojson and not a.csv:
        ap.error("give --geojson, --csv or both")
    w = window_dict(a.window)
    H, W = a.dem_size
    field = predicate_args.load_map(a.map, w)
    if field.shape[2] > 16:
        field, a.channel = field[:, :, a.channel:a.channel + 1], 0
    lo, hi = predicate_args.bounds(a)
    weights = rg.row_weights(w, (H, W), a.radius_m, a.unit_m2)
    rt = MoonRT(16, 16, device=0)
    st = {}
    m = rt.regions(field=np.ascontiguousarray(field, np.float32), channel=a.channel, lo=lo, hi=hi, connectivity=a.connectivity,
                   wrap=bool(w["wrap"]), row_weights=weights, unit_m2=a.unit_m2)
    kept = m.filter(min_area=a.min_area_km2 * 1e6)
    ol = kept.outlines(rt, a.connectivity, corners=not a.all_vertices, row_weights=weights, stats=st)
    ew, ns = rg.side_weights(w, (H, W), a.radius_m, a.side_unit_m)
    sh = kept.shapes(rt, a.connectivity, ew, ns)
    rt.close()
    latlon = ol.corner_latlon(w, (H, W))
    for path in (a.geojson, a.csv):
        if path:
            os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    if a.geojson:
        fc = feature_collection(ol, latlon, {"area_km2": kept.area_m2() / 1e6, "nodes": kept.table["count"].astype(np.int64),
                                             "holes": ol.holes(kept.n),
                                             "perimeter_km": sh["perimeter"].astype(np.float64) * (a.side_unit_m / 1e3)})
        with open(a.geojson, "w") as f:
            json.dump(fc, f)
    if a.csv:
        with open(a.csv, "w", newline="") as f:
            out = csv.writer(f)
            out.writerow(["ring", "region", "role", "y", "x", "lat", "lon"])
            out.writerows(vertex_rows(ol, latlon))
    print(f"{w['rows']}x{w['cols']} nodes, {a.connectivity}-connected{', wrapped' if w['wrap'] else ''}: {kept.n} regions of at least "
          f"{a.min_area_km2:g} km^2, {len(ol)} rings, {ol.vertices.shape[0]} vertices; {st['kernel_ms']:.2f} ms in {st['launches']} "
          f"launches; wrote {', '.join(p for p in (a.geojson, a.csv) if p)}")


if __name__ == "__main__":
    main()
