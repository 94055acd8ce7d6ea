#!/usr/bin/env python3
"""Landing-hazard maps, headless: slope and roughness under a lander's footprint over a window of the
DEM's texel lattice, and the share of a landing ellipse around every node that is safe.

  python tools/hazard_map.py --window 20000 30000 1024 1024 --footprint 100 --max-slope 10 --max-rms 2 --ellipse 2000 \\
      --out hazard.npy
  python tools/hazard_map.py --point -72.3 58.1 --footprint 100
--window ROW0 COL0 ROWS COLS [STRIDE] is a block of DEM texels (rows from the north, columns from -180), every STRIDE-th one.
--footprint M is the footprint's width in metres (the window is split into row bands of constant width in nodes).  The .npy
holds a (rows, cols, 3) float32 array: slope in degrees, roughness in metres (root mean square about the footprint's
least-squares plane) and the safe share of the --ellipse M box around the node: the fraction of its nodes with slope <=
--max-slope and roughness <= --max-rms.  --point LAT LON prints the values of the nearest node of the DEM instead.  Synthetic
LOLA-like DEM unless --elevation-file is given; heights are metres on the DEM's own radius (1737.4 km x its radius_scale)."""
import argparse, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
from moonrtx_amd.renderer import MoonRT, synth_ldem, dem_from_ldem

ap = argparse.ArgumentParser()
ap.add_argument("--window", type=int, nargs="+", default=None, metavar="N", help="ROW0 COL0 ROWS COLS [STRIDE] in DEM texels")
ap.add_argument("--point", type=float, nargs=2, default=None, metavar=("LAT", "LON"))
ap.add_argument("--footprint", type=float, required=True, metavar="M", help="the footprint's width, metres")
ap.add_argument("--max-slope", type=float, default=10.0, help="degrees")
ap.add_argument("--max-rms", type=float, default=2.0, help="metres")
ap.add_argument("--ellipse", type=float, default=None, metavar="M", help="the landing ellipse's width, metres")
ap.add_argument("--downscale", type=int, default=2)
ap.add_argument("--dem-size", type=int, nargs=2, default=None, help="synthetic DEM (h, w); default 46080/downscale x 92160/downscale")
ap.add_argument("--elevation-file", default=None)
ap.add_argument("--out", default="hazard.npy")
a = ap.parse_args()
if (a.window is None) == (a.point is None):
    ap.error("give exactly one of --window and --point")
if a.window is not None and not 4 <= len(a.window) <= 5:
    ap.error("--window takes ROW0 COL0 ROWS COLS [STRIDE]")

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
rt.set_params(flags=0)
radius_m = 1737400.0 * float(radius_scale)
if a.point is not None:
    ij = rt.snap_to_nodes((0, 0, dh, dw), [a.point[0]], [a.point[1]])[0]
    m = rt.relief((int(ij[0]), int(ij[1]), 1, 1), footprint_m=a.footprint, radius_m=radius_m)
    print(f"texel ({ij[0]}, {ij[1]}) at ({m.lat[0]:.5f}, {m.lon[0]:.5f}), footprint {2 * m.ri + 1} x {2 * m.bands[0][2] + 1} nodes: "
          f"slope {m.slope_deg[0, 0]:.3f} deg, descending towards azimuth {m.aspect_deg[0, 0]:.1f} deg, roughness "
          f"{m.rms_m[0, 0]:.3f} m")
else:
    st = {}
    m = rt.relief(tuple(a.window), footprint_m=a.footprint, radius_m=radius_m, stats=st)
    out = np.full(m.grade.shape + (3,), np.nan, np.float32)
    out[..., 0], out[..., 1] = m.slope_deg, m.rms_m
    safe = (m.slope_deg <= a.max_slope) & (m.rms_m <= a.max_rms)
    msg = (f"{m.grade.shape[0]}x{m.grade.shape[1]} nodes in {len(m.bands)} bands, {st['kernel_ms']:.2f} ms of kernels: "
           f"{float(safe.mean()):.4f} of them safe")
    if a.ellipse is not None:
        out[..., 2] = rt.landing_share(m, a.max_slope, a.max_rms, ellipse_m=a.ellipse)
        msg += f", the best {a.ellipse:g} m ellipse {float(np.nanmax(out[..., 2])):.4f} safe"
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    np.save(a.out, out)
    print(msg + f"; wrote {a.out}")
rt.close()
if dem_buf is not None:
    dem_buf.free()
