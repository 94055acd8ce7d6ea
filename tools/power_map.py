#!/usr/bin/env python3
"""Does a solar-powered asset survive there, and on how much battery -- over a lat/lon window, or the date-by-date record of
one point, headless.

  python tools/power_map.py --window -85 -90 -180 180 --size 256 256 --time 2025-01-01T00:00:00+00:00 --days 365 \\
      --height 2 --area 2.0 --eff 0.29 --load 150 --panel azimuth --capacity-wh 5000 --out power.npy
  python tools/power_map.py --point -89.5 45.0 --height 2 --days 30 --area 2 --eff 0.29 --load 150 > record.csv
The window's nodes are MoonRT.grid_nodes; power.npy holds an (8, h, w) float64 array: the energy generated and the net
energy (Wh), the least battery which, starting full, never empties (Wh), the indices of the first and last date of that worst
deficit (-1: none), and for the --capacity-wh battery the lowest state of charge (Wh), the hours during which it could not
carry the load and the energy not delivered (Wh).  --point prints time, f, G, e, s per date as CSV (G, e and s in Wh) and the
summary line on stderr.  --eclipses multiplies the array's output by ephemeris.eclipse_factor, the Earth's cover of the Sun
seen from the Moon's centre (section 3.18): one factor for the whole Moon.  Synthetic LOLA-like DEM unless --elevation-file is given."""
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
ap.add_argument("--height", type=float, default=0.0, help="panel height above the ground, metres")
ap.add_argument("--area", type=float, default=1.0, help="array area, m^2")
ap.add_argument("--eff", type=float, default=0.29, help="conversion efficiency")
ap.add_argument("--load", type=float, default=100.0, help="power drawn, W")
ap.add_argument("--panel", choices=("track", "fixed", "azimuth"), default="track")
ap.add_argument("--normal", type=float, nargs=3, default=None, metavar=("E", "N", "U"), help="the fixed panel's normal")
ap.add_argument("--capacity-wh", type=float, default=0.0, help="the battery whose state of charge is followed, Wh")
ap.add_argument("--lat", type=float, default=52.2, help="observer (the ephemeris' topocentric frame)")
ap.add_argument("--lon", type=float, default=21.0)
ap.add_argument("--n-az", type=int, default=256)
ap.add_argument("--n-bis", type=int, default=14)
ap.add_argument("--downscale", type=int, default=2)
ap.add_argument("--dem-size", type=int, nargs=2, default=None, help="synthetic DEM (h, w); default 46080/downscale x 92160/downscale")
ap.add_argument("--elevation-file", default=None)
ap.add_argument("--eclipses", action="store_true", help="the Earth's cover of the Sun, one factor for the whole Moon")
ap.add_argument("--out", default="power.npy")
a = ap.parse_args()
if (a.window is None) == (a.point is None):
    ap.error("give exactly one of --window and --point")
if (a.panel == "fixed") != (a.normal is not None):
    ap.error("--normal goes with --panel fixed, and only with it")

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
# the march parameters and Moon radius of scene S1; the Sun's position and flux come from the ephemeris per date
rt.apply_scene(named_scene("S1", 16, 16))
rt.set_params(flags=0)
n_az = 1 << max(2, int(np.ceil(np.log2(a.n_az))))
obs = ephemeris.Observer(a.lat, a.lon, 0.0)
start = datetime.fromisoformat(a.time)
kw = dict(area_m2=a.area, efficiency=a.eff, load_w=a.load, panel=a.panel, normal_enu=a.normal, capacity_wh=a.capacity_wh,
          n_az=n_az, n_bis=a.n_bis, observer=obs, eclipses=a.eclipses)
if a.point is not None:
    la, lo = [a.point[0]], [a.point[1]]
    r = sunlight.power_budget(rt, la, lo, start, a.days, a.step_min, a.height, **kw)
    ep = ephemeris.sun_epochs(r.times, obs)
    gen = ephemeris.sun_flux(r.times) * (a.area * a.eff)
    if a.eclipses:
        gen = gen * ephemeris.eclipse_factor(r.times, obs)
    hz = rt.horizon(la, lo, n_az=n_az, n_bis=a.n_bis, height_m=a.height)
    f = rt.horizon_sun(la, lo, hz, ep)[0]
    G = rt.power_budget(la, lo, hz, ep, gen, a.load, panel=a.panel, normal_enu=a.normal, cpw_log2=r.cpw_log2, mode="full")[0]
    L = int(np.rint(np.float32(a.load) * np.float32(2.0 ** r.cpw_log2)))
    cap = sunlight.wh_to_counts(a.capacity_wh, r.cpw_log2, a.step_min)
    wh = lambda c: float(sunlight.counts_to_wh(c, r.cpw_log2, a.step_min))     # noqa: E731
    print("time,f,G_wh,e_wh,s_wh")
    s = cap
    for t, fk, g in zip(r.times, f, G):
        e = int(g) - L
        s = min(cap, max(0, s + e))
        print(f"{t.isoformat()},{fk:.6f},{wh(int(g)):.6f},{wh(e):.6f},{wh(s):.6f}")
    k0, k1 = int(r.deficit_start[0]), int(r.deficit_end[0])
    worst = "none" if k0 < 0 else f"{r.storage_wh[0]:.1f} Wh from {r.times[k0].isoformat()} to {r.times[k1].isoformat()}"
    print(f"# {len(r.times)} dates at {a.height} m, {a.panel} panel: generated {r.generated_wh[0]:.1f} Wh, net {r.net_wh[0]:.1f} Wh; "
          f"worst deficit {worst}; with {a.capacity_wh:.1f} Wh: lowest charge {r.min_charge_wh[0]:.1f} Wh, {r.unmet_h[0]:.1f} h and "
          f"{r.unmet_wh[0]:.1f} Wh unmet", file=sys.stderr)
else:
    N, S, W, E = a.window
    la, lo = MoonRT.grid_nodes(lat=(N, S), lon=(W, E), shape=tuple(a.size))
    LA, LO = np.meshgrid(la, lo, indexing="ij")
    r = sunlight.power_budget(rt, LA.ravel(), LO.ravel(), start, a.days, a.step_min, a.height, **kw)
    out = np.stack([r.generated_wh, r.net_wh, r.storage_wh, r.deficit_start.astype(np.float64), r.deficit_end.astype(np.float64),
                    r.min_charge_wh, r.unmet_h, r.unmet_wh]).reshape(8, *a.size)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    np.save(a.out, out)
    print(f"{a.size[0]}x{a.size[1]} points x {len(r.times)} dates at {a.height} m, {a.panel} panel: {r.stats['kernel_ms']:.1f} ms of "
          f"kernels in {r.stats['launches']} launches; storage need {float(r.storage_wh.min()):.0f} to "
          f"{float(r.storage_wh.max()):.0f} Wh; wrote {a.out}")
rt.close()
if dem_buf is not None:
    dem_buf.free()
