#!/usr/bin/env python3
"""For how long can a lander work without a break -- Sun on the panel AND the Earth in view -- over a lat/lon window, or the
epoch-by-epoch record of one point, from a mast top, headless.

  python tools/site_windows.py --window -85 -90 -180 180 --size 256 256 --time 2025-01-01T00:00:00+00:00 --days 365 \\
      --step-min 60 --height 10 --min-sun 0.5 --min-earth 1.0 --out windows.npy
  python tools/site_windows.py --point -89.5 45.0 --height 2 --days 30 > record.csv
The window's nodes are MoonRT.grid_nodes; windows.npy holds an (8, h, w) float32 array: the share of dates with the Sun, the
longest run without it (hours), the same for the Earth, the share of dates with both, the longest unbroken window with both
(hours), the index of its first date (-1: none) and the longest outage (hours).  --point prints time, f_sun, f_earth, both per
date as CSV and the summary line on stderr.  Synthetic LOLA-like DEM unless --elevation-file is given."""
import argparse, os, sys
from datetime import datetime, timedelta
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
ap.add_argument("--height", type=float, default=0.0, help="mast height above the ground, metres")
ap.add_argument("--min-sun", type=float, default=0.5, help="least visible share of the Sun's disc that counts")
ap.add_argument("--min-earth", type=float, default=1.0, help="least visible share of the Earth's disc that counts")
ap.add_argument("--lat", type=float, default=52.2, help="observer (the ephemeris' topocentric frame)")
ap.add_argument("--lon", type=float, default=21.0)
ap.add_argument("--n-az", type=int, default=256)
ap.add_argument("--n-bis", type=int, default=14)
ap.add_argument("--downscale", type=int, default=2)
ap.add_argument("--dem-size", type=int, nargs=2, default=None, help="synthetic DEM (h, w); default 46080/downscale x 92160/downscale")
ap.add_argument("--elevation-file", default=None)
ap.add_argument("--out", default="windows.npy")
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
# the march parameters and Moon radius of scene S1; the Sun's and the Earth's positions come from the ephemeris per date
rt.apply_scene(named_scene("S1", 16, 16))
rt.set_params(flags=0)
n_az = 1 << max(2, int(np.ceil(np.log2(a.n_az))))
obs = ephemeris.Observer(a.lat, a.lon, 0.0)
start = datetime.fromisoformat(a.time)
if a.point is not None:
    la, lo = [a.point[0]], [a.point[1]]
    r = sunlight.site_windows(rt, la, lo, start, a.days, a.step_min, a.height, a.min_sun, a.min_earth, n_az, a.n_bis, obs)
    ep_sun, ep_earth = ephemeris.sun_earth_epochs(r.times, obs)
    hz = rt.horizon(la, lo, n_az=n_az, n_bis=a.n_bis, height_m=a.height)
    f_sun, f_earth = rt.horizon_sun(la, lo, hz, ep_sun)[0], rt.horizon_sun(la, lo, hz, ep_earth)[0]
    print("time,f_sun,f_earth,both")
    for t, fs, fe in zip(r.times, f_sun, f_earth):
        print(f"{t.isoformat()},{fs:.6f},{fe:.6f},{int(fs >= np.float32(a.min_sun) and fe >= np.float32(a.min_earth))}")
    k = int(r.best_start[0])
    best = "none" if k < 0 else f"{r.longest_both_h[0]:.1f} h from {r.times[k].isoformat()}"
    print(f"# {len(r.times)} dates at {a.height} m: Sun {r.sun_share[0]:.4f}, Earth {r.earth_share[0]:.4f}, both "
          f"{r.both_share[0]:.4f}; longest window {best}; longest outage {r.longest_outage_h[0]:.1f} h", file=sys.stderr)
else:
    N, S, W, E = a.window
    la, lo = MoonRT.grid_nodes(lat=(N, S), lon=(W, E), shape=tuple(a.size))
    LA, LO = np.meshgrid(la, lo, indexing="ij")
    r = sunlight.site_windows(rt, LA.ravel(), LO.ravel(), start, a.days, a.step_min, a.height, a.min_sun, a.min_earth, n_az,
                              a.n_bis, obs)
    out = np.stack([r.sun_share, r.longest_no_sun_h, r.earth_share, r.longest_no_earth_h, r.both_share, r.longest_both_h,
                    r.best_start, r.longest_outage_h]).astype(np.float32).reshape(8, *a.size)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    np.save(a.out, out)
    print(f"{a.size[0]}x{a.size[1]} points x {len(r.times)} dates at {a.height} m: {r.stats['kernel_ms']:.1f} ms of kernels in "
          f"{r.stats['launches']} launches; mean share with both {float(r.both_share.mean()):.4f}, longest window "
          f"{float(r.longest_both_h.max()):.0f} h, longest outage {float(r.longest_outage_h.max()):.0f} h; wrote {a.out}")
rt.close()
if dem_buf is not None:
    dem_buf.free()
