#!/usr/bin/env python3
"""Where does buried ice survive, and how deep must it lie?  Ice-stability depths over a lat/lon window, or the depth profile
of one point, from the terrain horizons and the subsurface columns (DESIGN.md sections 3.8, 3.10 and 3.16), headless.

  python tools/ice_map.py --window -85 -90 -180 180 --size 256 256 --time 2025-01-01T00:00:00+00:00 --days 365 --out ice.npy
  python tools/ice_map.py --point -89.5 45.0 --days 365
--scatter K adds the sunlight and infrared the surrounding terrain sends, from K view rays per point (section 3.11).
The window's nodes are MoonRT.grid_nodes; ice.npy holds a (3, h, w) float32 array: the depth below which water ice retreats
by at most 1 mm per 10^9 years (0: stable at the surface; inf: nowhere in the column), the loss rate of ice exposed at the
surface in mm per 10^9 years, and the surface's highest temperature, K.  --point prints per node its depth, its highest
temperature and its mean loss rate.  The regolith is the dry one throughout (ice changes neither k nor c), the rate is the
time mean of the free sublimation rate (no pumping, no recondensation), and the scattering is one bounce.  Synthetic
LOLA-like DEM unless --elevation-file is given."""
import argparse, os, sys
from datetime import datetime
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
from moonrtx_amd import ephemeris, sunlight, thermal, volatiles
from moonrtx_amd.renderer import MoonRT, synth_ldem, dem_from_ldem
from moonrtx_amd.scene import named_scene

ap = argparse.ArgumentParser()
ap.add_argument("--window", type=float, nargs=4, default=None, metavar=("N", "S", "W", "E"))
ap.add_argument("--size", type=int, nargs=2, default=(256, 256), metavar=("H", "W"))
ap.add_argument("--point", type=float, nargs=2, default=None, metavar=("LAT", "LON"))
ap.add_argument("--time", default="2025-01-01T00:00:00+00:00", help="first recorded date, ISO 8601 with UTC offset")
ap.add_argument("--days", type=float, default=365.0)
ap.add_argument("--step-min", type=float, default=60.0)
ap.add_argument("--spinup-lunations", type=int, default=thermal.SPINUP_LUNATIONS)
ap.add_argument("--lat", type=float, default=52.2, help="observer (the ephemeris' topocentric frame)")
ap.add_argument("--lon", type=float, default=21.0)
ap.add_argument("--n-az", type=int, default=256)
ap.add_argument("--n-bis", type=int, default=14)
ap.add_argument("--downscale", type=int, default=2)
ap.add_argument("--dem-size", type=int, nargs=2, default=None, help="synthetic DEM (h, w); default 46080/downscale x 92160/downscale")
ap.add_argument("--elevation-file", default=None)
ap.add_argument("--scatter", type=int, default=0, help="K view rays per point for the terrain-scattered flux (0: none)")
ap.add_argument("--barrier-m", type=float, default=None, help="diffusion length of a dry lag above the ice, m (default: exposed ice)")
ap.add_argument("--out", default="ice.npy")
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
# the march parameters and Moon radius of scene S1; the Sun's positions come from the ephemeris per date
rt.apply_scene(named_scene("S1", 16, 16))
rt.set_params(flags=0)
n_az = 1 << max(2, int(np.ceil(np.log2(a.n_az))))
obs = ephemeris.Observer(a.lat, a.lon, 0.0)
start = datetime.fromisoformat(a.time)
if a.point is not None:
    la, lo, shape = np.array([a.point[0]]), np.array([a.point[1]]), None
else:
    N, S, W, E = a.window
    g_la, g_lo = MoonRT.grid_nodes(lat=(N, S), lon=(W, E), shape=tuple(a.size))
    LA, LO = np.meshgrid(g_la, g_lo, indexing="ij")
    la, lo, shape = LA.ravel(), LO.ravel(), tuple(a.size)
r = sunlight.ice_stability(rt, la, lo, start, a.days, a.step_min, a.spinup_lunations, n_az, a.n_bis, obs, scatter=a.scatter,
                           barrier_m=a.barrier_m)
loss = r.loss_rate_surface * volatiles.MM_PER_GYR
if shape is None:
    print("depth_m,T_max_K,mean_loss_mm_per_Gyr")
    for z, t, e in zip(r.z, r.t_max_nodes[0], r.e_mean[0]):
        print(f"{z:.4f},{t:.3f},{e / volatiles.H2O.rho_solid * volatiles.MM_PER_GYR:.6e}")
    print(f"# ice is stable below {float(r.depth_m[0]):.4f} m; {len(r.times)} dates: {r.stats['kernel_ms']:.3f} ms of kernels",
          file=sys.stderr)
else:
    out = np.stack([r.depth_m, loss, r.t_max_nodes[:, 0]]).reshape(3, *shape)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    np.save(a.out, out.astype(np.float32))
    print(f"{shape[0]}x{shape[1]} points x {len(r.times)} dates: {r.stats['kernel_ms']:.1f} ms of kernels in "
          f"{r.stats['launches']} launches; stable at the surface {float((r.depth_m == 0.0).mean()):.4f} of the points, "
          f"buried {float((np.isfinite(r.depth_m) & (r.depth_m > 0.0)).mean()):.4f}, nowhere "
          f"{float(np.isinf(r.depth_m).mean()):.4f}; wrote {a.out}")
rt.close()
if dem_buf is not None:
    dem_buf.free()
