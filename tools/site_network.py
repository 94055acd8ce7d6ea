#!/usr/bin/env python3
"""Which two sites together are never dark, and which few: site pairs and greedy site sets over a lat/lon window, from the
terrain horizons and the availability masks, headless.

  python tools/site_network.py --window -88 -90 -180 180 --size 64 64 --time 2025-01-01T00:00:00+00:00 --days 365 \\
      --step-min 60 --height 10 --max-dist-m 5000 --top 20 --csv pairs.csv --k 3 --sites sites.csv --out best.npy
The window's nodes are MoonRT.grid_nodes.  Every node's mask says when the Sun's visible share is >= --min-sun and, with
--min-earth, the Earth's >= --min-earth, seen from --height metres above the ground; the masks stay in one device buffer.
site_pairs gives every node its best partner between --min-dist-m and --max-dist-m (the union of the two masks, or with --both
their intersection) under --rank count (most available epochs) or gap (shortest longest outage); --csv lists the --top distinct
pairs with both sites' lat/lon, their own shares, the joint share, the longest joint outage in hours and its start date; --out
saves every node's record.  greedy_sites grows a set of --k sites, each the one that adds most to the union so far; --sites
lists them with the union's share and longest outage after each.  Synthetic LOLA-like DEM unless --elevation-file is given."""
import argparse, csv, os, sys
from datetime import datetime, timedelta
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
from moonrtx_amd import ephemeris, networks
from moonrtx_amd.renderer import MoonRT, synth_ldem, dem_from_ldem
from moonrtx_amd.scene import named_scene

ap = argparse.ArgumentParser()
ap.add_argument("--window", type=float, nargs=4, required=True, metavar=("LATN", "LATS", "LONW", "LONE"))
ap.add_argument("--size", type=int, nargs=2, default=(64, 64), metavar=("R", "C"))
ap.add_argument("--time", default="2025-01-01T00:00:00+00:00", help="first date, ISO 8601 with UTC offset")
ap.add_argument("--days", type=float, default=365.0)
ap.add_argument("--step-min", type=float, default=60.0)
ap.add_argument("--height", type=float, default=0.0, help="mast height above the ground, metres")
ap.add_argument("--min-sun", type=float, default=0.5)
ap.add_argument("--min-earth", type=float, default=None)
ap.add_argument("--max-dist-m", type=float, default=None)
ap.add_argument("--min-dist-m", type=float, default=0.0)
ap.add_argument("--rank", choices=("count", "gap"), default="count")
ap.add_argument("--both", action="store_true", help="both sites available at once, not either")
ap.add_argument("--top", type=int, default=20)
ap.add_argument("--csv", default=None)
ap.add_argument("--k", type=int, default=0)
ap.add_argument("--sites", default=None)
ap.add_argument("--out", default=None)
ap.add_argument("--unit-m", type=float, default=0.01, help="the unit of the integer positions, metres")
ap.add_argument("--lat", type=float, default=52.2, help="observer (the ephemeris' topocentric frame)")
ap.add_argument("--lon", type=float, default=21.0)
ap.add_argument("--n-az", type=int, default=256)
ap.add_argument("--n-bis", type=int, default=14)
ap.add_argument("--downscale", type=int, default=2)
ap.add_argument("--dem-size", type=int, nargs=2, default=None, help="synthetic DEM (h, w); default 46080/downscale x 92160/downscale")
ap.add_argument("--elevation-file", default=None)
a = ap.parse_args()

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
rt.apply_scene(named_scene("S1", 16, 16))      # the march parameters and Moon radius; the dates' lights come from the ephemeris
rt.set_params(flags=0)
N, S, W, E = a.window
la, lo = MoonRT.grid_nodes(lat=(N, S), lon=(W, E), shape=tuple(a.size))
LA, LO = (x.ravel() for x in np.meshgrid(la, lo, indexing="ij"))
t0 = datetime.fromisoformat(a.time)
m = max(int(a.days * 1440.0 / a.step_min), 1)
times = [t0 + timedelta(minutes=a.step_min * k) for k in range(m)]
n = LA.size
mask = networks.site_mask(rt, LA, LO, times, height_m=a.height, min_sun=a.min_sun, min_earth=a.min_earth, n_az=a.n_az,
                          n_bis=a.n_bis, observer=ephemeris.Observer(a.lat, a.lon, 0.0))
pos = networks.point_positions(LA, LO, 1737400.0, a.unit_m, a.height)
hours = a.step_min / 60.0


def when(first):
    return "" if first < 0 else (t0 + timedelta(minutes=a.step_min * int(first))).isoformat()


st = {}
sp = networks.site_pairs(rt, mask, m, positions=pos, unit_m=a.unit_m, min_dist_m=a.min_dist_m, max_dist_m=a.max_dist_m,
                         op="both" if a.both else "any", rank=a.rank, n_rows=n, stats=st)
top = sp.top(a.top)
print(f"{n} sites x {m} epochs: {st['pairs']} eligible pairs in {st['kernel_ms']:.1f} ms of kernels; own share at best "
      f"{sp.own['count'].max() / m:.4f}" + (f", best pair {top['count'][0] / m:.4f} with a longest outage of "
                                           f"{top['gap'][0] * hours:.1f} h" if len(top) else ", no eligible pair"))
if a.csv:
    with open(a.csv, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["lat_a", "lon_a", "lat_b", "lon_b", "share_a", "share_b", "share_joint", "longest_outage_h", "outage_start"])
        for r in top:
            i, j = int(r["a"]), int(r["b"])
            w.writerow([f"{LA[i]:.6f}", f"{LO[i]:.6f}", f"{LA[j]:.6f}", f"{LO[j]:.6f}", f"{sp.own['count'][i] / m:.6f}",
                        f"{sp.own['count'][j] / m:.6f}", f"{r['count'] / m:.6f}", f"{r['gap'] * hours:.3f}", when(r["gap_first"])])
if a.out:
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    np.save(a.out, sp.best.reshape(tuple(a.size)))
if a.k > 0:
    g = networks.greedy_sites(rt, mask, m, a.k, rank=a.rank, n_rows=n)
    print("greedy sites: " + ", ".join(f"({LA[s]:.3f}, {LO[s]:.3f}) -> {r['count'] / m:.4f}" for s, r in zip(g.sites, g.records)))
    if a.sites:
        with open(a.sites, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["step", "lat", "lon", "share_union", "longest_outage_h", "outage_start"])
            for k, (s, r) in enumerate(zip(g.sites, g.records)):
                w.writerow([k, f"{LA[s]:.6f}", f"{LO[s]:.6f}", f"{r['count'] / m:.6f}", f"{r['gap'] * hours:.3f}", when(r["gap_first"])])
mask.free()
rt.close()
if dem_buf is not None:
    dem_buf.free()
