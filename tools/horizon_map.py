#!/usr/bin/env python3
"""Long-term Sun statistics over a lat/lon window, or the skyline of one point, from the terrain horizon stage (DESIGN.md
sections 3.8 and 3.9), headless.

  python tools/horizon_map.py --window -85 -90 -180 180 --size 256 256 --time 2025-01-01T00:00:00+00:00 --days 365 \\
      --step-min 60 --out stats.npy
  python tools/horizon_map.py --point -89.5 45.0 --n-az 360 > skyline.csv      (n_az is rounded up to a power of two)
The window's nodes are MoonRT.grid_nodes; stats.npy holds a (4, h, w) float32 array: the mean visible share of the Sun's disc,
the share of dates with any of it up, the share with all of it up, and the longest run of dates with none of it up, in hours.
Synthetic LOLA-like DEM unless --elevation-file is given."""
import argparse, os, sys
from datetime import datetime
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
from moonrtx_amd import ephemeris, sunlight
from moonrtx_amd.renderer import MoonRT, synth_ldem, dem_from_ldem
from moonrtx_amd.scene import named_scene

ap = argparse.ArgumentParser()
ap.add_argument("--window", type=float, nargs=4, default=None, metavar=("N", "S", "W", "E"))
ap.add_argument("--size", type=int, nargs=2, default=(256, 256), metavar=("H", "W"))
ap.add_argument("--point", type=float, nargs=2, default=None, metavar=("LAT", "LON"))
ap.add_argument("--time", default="2025-01-01T00:00:00+00:00", help="first date, ISO 8601 with UTC offset")
ap.add_argument("--days", type=float, default=365.0)
ap.add_argument("--step-min", type=float, default=60.0)
ap.add_argument("--lat", type=float, default=52.2, help="observer (the ephemeris' topocentric frame)")
ap.add_argument("--lon", type=float, default=21.0)
ap.add_argument("--n-az", type=int, default=256)
ap.add_argument("--n-bis", type=int, default=14)
ap.add_argument("--downscale", type=int, default=2)
ap.add_argument("--dem-size", type=int, nargs=2, default=None, help="synthetic DEM (h, w); default 46080/downscale x 92160/downscale")
ap.add_argument("--elevation-file", default=None)
ap.add_argument("--out", default="stats.npy")
a = ap.parse_args()
if (a.window is None) == (a.point is None):
    ap.error("give exactly one of --window and --point")

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
# the march parameters and Moon radius of scene S1 (the reference renderer's: step 5e-3, scene_epsilon 1e-4, radius 10); the
# Sun's positions come from the ephemeris per date, so the scene's own light and Moon frame are not used
rt.apply_scene(named_scene("S1", 16, 16))
rt.set_params(flags=0)
n_az = 1 << max(2, int(np.ceil(np.log2(a.n_az))))
if a.point is not None:
    st = {}
    hz = rt.horizon([a.point[0]], [a.point[1]], n_az=n_az, n_bis=a.n_bis, stats=st)[0]
    print("azimuth_deg,elevation_deg")
    for az, el in zip(MoonRT.horizon_azimuths(n_az), hz):
        print(f"{az:.6f},{el:.6f}")
    print(f"# {n_az} azimuths x {a.n_bis} probes: {st['kernel_ms']:.3f} ms", file=sys.stderr)
else:
    N, S, W, E = a.window
    la, lo = MoonRT.grid_nodes(lat=(N, S), lon=(W, E), shape=tuple(a.size))
    LA, LO = np.meshgrid(la, lo, indexing="ij")
    r = sunlight.illumination_statistics(rt, LA.ravel(), LO.ravel(), datetime.fromisoformat(a.time), a.days, a.step_min,
                                         n_az, a.n_bis, ephemeris.Observer(a.lat, a.lon, 0.0))
    out = np.stack([r.mean_fraction, r.lit_fraction, r.full_fraction, r.longest_dark_h.astype(np.float32)]).reshape(4, *a.size)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    np.save(a.out, out.astype(np.float32))
    print(f"{a.size[0]}x{a.size[1]} points x {len(r.times)} dates: {r.stats['kernel_ms']:.1f} ms of kernels in "
          f"{r.stats['launches']} launches; mean lit share {float(r.lit_fraction.mean()):.4f}, longest night "
          f"{float(r.longest_dark_h.max()):.0f} h; wrote {a.out}")
rt.close()
if dem_buf is not None:
    dem_buf.free()
