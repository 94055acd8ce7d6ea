#!/usr/bin/env python3
"""Who sees whom over the terrain, headless: a viewshed over a lat/lon window, or the line of sight
from one point, toward an observer raised H metres above (LAT, LON).

  python tools/viewshed_map.py --observer -89.45 -137.3 10 --window -88 -90 -180 180 --size 512 512 --out view.npy
  python tools/viewshed_map.py --observer -89.45 -137.3 10 --window -88 -90 -180 180 --size 512 512 --mast-max 200 \\
      --n-bis 10 --out mast.npy
  python tools/viewshed_map.py --observer 0 0 1e8 --point -89.5 45.0
The window's nodes are MoonRT.grid_nodes; the .npy holds the (h, w) float32 extra mast height, metres, at which a target raised
--target-height sees the observer: 0 in view, +inf not even with --mast-max (with --n-bis 0, the default, 0 or +inf).
Synthetic LOLA-like DEM unless --elevation-file is given; heights are metres on the DEM's own radius (1737.4 km x its
radius_scale)."""
import argparse, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
from moonrtx_amd.renderer import MoonRT, synth_ldem, dem_from_ldem
from moonrtx_amd.scene import named_scene

ap = argparse.ArgumentParser()
ap.add_argument("--observer", type=float, nargs=3, required=True, metavar=("LAT", "LON", "H"))
ap.add_argument("--window", type=float, nargs=4, default=None, metavar=("N", "S", "W", "E"))
ap.add_argument("--size", type=int, nargs=2, default=(512, 512), metavar=("H", "W"))
ap.add_argument("--point", type=float, nargs=2, default=None, metavar=("LAT", "LON"))
ap.add_argument("--target-height", type=float, default=0.0, help="metres above the terrain of every target")
ap.add_argument("--mast-max", type=float, default=0.0, help="the largest extra mast the bisection tries, metres")
ap.add_argument("--n-bis", type=int, default=0, help="mast probes (0: a plain viewshed)")
ap.add_argument("--downscale", type=int, default=2)
ap.add_argument("--dem-size", type=int, nargs=2, default=None, help="synthetic DEM (h, w); default 46080/downscale x 92160/downscale")
ap.add_argument("--elevation-file", default=None)
ap.add_argument("--out", default="viewshed.npy")
a = ap.parse_args()
if (a.window is None) == (a.point is None):
    ap.error("give exactly one of --window and --point")

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
# the march parameters and Moon radius of scene S1 (step 5e-3, scene_epsilon 1e-4, radius 10); no light or Moon frame is used
rt.apply_scene(named_scene("S1", 16, 16))
rt.set_params(flags=0)
radius_m = 1737400.0 * float(radius_scale)
args = dict(target_height_m=a.target_height, mast_max_m=a.mast_max, n_bis=a.n_bis, radius_m=radius_m)
st = {}
if a.point is not None:
    m = float(rt.line_of_sight([a.point[0]], [a.point[1]], tuple(a.observer), stats=st, **args)[0])
    what = "in view" if m == 0 else ("not in view" if np.isinf(m) else f"in view with a {m:.2f} m mast")
    print(f"({a.point[0]}, {a.point[1]}) -> observer {tuple(a.observer)}: {what} ({st['kernel_ms']:.3f} ms)")
else:
    N, S, W, E = a.window
    v = rt.viewshed(tuple(a.observer), lat=(N, S), lon=(W, E), shape=tuple(a.size), stats=st, **args)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    np.save(a.out, v)
    mast = f", {float(np.isfinite(v).mean()):.4f} with a mast up to {a.mast_max:g} m" if a.n_bis > 0 else ""
    print(f"{a.size[0]}x{a.size[1]} targets: {float((v == 0).mean()):.4f} of the window in view{mast}; "
          f"{st['kernel_ms']:.2f} ms of kernels in {st['launches']} launches; wrote {a.out}")
rt.close()
if dem_buf is not None:
    dem_buf.free()
