#!/usr/bin/env python3
"""Regolith surface temperatures over a lat/lon window, or the temperature series of one point, from the terrain horizons and
the thermal stage (DESIGN.md sections 3.8 and 3.10), headless.

  python tools/temperature_map.py --window -85 -90 -180 180 --size 256 256 --time 2025-01-01T00:00:00+00:00 --days 365 \\
      --step-min 60 --out temps.npy
  python tools/temperature_map.py --point -89.5 45.0 --days 30 > series.csv
--scatter K adds the sunlight and infrared the surrounding terrain sends, from K view rays per point (section 3.11); with
--point it also prints the point's terrain view factor and its mean scattered flux.  --point ... --depths prints every
node's temperature per date (the COLUMN mode of section 3.16) instead of the surface's alone.
--eclipses lets the Earth cover the Sun (section 3.18); with --point over the hours of a lunar eclipse this prints the
eclipse cooling curve:
  python tools/temperature_map.py --point 0 0 --time 2025-03-14T03:00:00+00:00 --days 0.4 --step-min 5 --eclipses
The window's nodes are MoonRT.grid_nodes; temps.npy holds a (4, h, w) float32 array: the maximum, minimum and mean surface
temperature over the dates and the mean temperature of the column's bottom node, K.  The column is spun up over
--spinup-lunations lunations before the first date.  Synthetic LOLA-like DEM unless --elevation-file is given."""
import argparse, os, sys
from datetime import datetime, timedelta
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
from moonrtx_amd import ephemeris, sunlight, thermal
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
ap.add_argument("--depths", action="store_true", help="with --point: the whole column per date, one CSV column per node")
ap.add_argument("--eclipses", action="store_true", help="the Earth's occultation of the Sun in every column (section 3.18)")
ap.add_argument("--out", default="temps.npy")
a = ap.parse_args()
if a.depths and a.point is None:
    ap.error("--depths goes with --point")
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
    model = rt.thermal_grid(a.step_min * 60.0, a.spinup_lunations, min(thermal.RESETS, a.spinup_lunations))
    m_rec = int(round(a.days * 1440.0 / a.step_min))
    times = [start + timedelta(minutes=(k - model.n_spin) * a.step_min) for k in range(model.n_spin + m_rec)]
    st = {}
    hz = rt.horizon([a.point[0]], [a.point[1]], n_az=n_az, n_bis=a.n_bis, stats=st)
    occ = None
    if a.eclipses:
        if a.scatter:
            ap.error("--point with --scatter keeps the series without eclipses; use --window, or drop --scatter")
        sun, earth = ephemeris.sun_earth_epochs(times, obs)
        occ = (ephemeris.far_sun_epochs(sun, times), earth)
    if a.scatter:
        # the stages of sunlight.surface_temperatures(scatter=K) for one point, with the series kept
        hits, share = rt.view_hits([a.point[0]], [a.point[1]], k=a.scatter, stats=st)
        index, h_lat, h_lon = sunlight.compact_hits(hits)
        n_spin = int(model.n_spin)
        times_h = [start + timedelta(minutes=(k - 2 * n_spin) * a.step_min) for k in range(2 * n_spin + m_rec)]
        q = np.zeros((1, len(times)), np.float32)
        if h_lat.size:
            hz_h = rt.horizon(h_lat, h_lon, n_az=n_az, n_bis=a.n_bis, stats=st)
            ex = rt.surface_temperature_scatter(h_lat, h_lon, hz_h, ephemeris.sun_epochs(times_h, obs),
                                                ephemeris.sun_flux(times_h), model, mode="exitance", stats=st)
            q = rt.scatter_flux(index, ex, thermal.albedo_hemispherical(), thermal.EMISSIVITY, stats=st)
        col = rt.thermal_column if a.depths else rt.surface_temperature_scatter
        ts = col([a.point[0]], [a.point[1]], hz, ephemeris.sun_epochs(times, obs), ephemeris.sun_flux(times), model,
                 mode="column" if a.depths else "full", extra_flux=q, stats=st)[0]
        print(f"# terrain view factor {float(share[0]):.4f} ({h_lat.size} of {a.scatter} rays), mean scattered flux "
              f"{float(q[0, n_spin:].astype(np.float64).mean()):.3f} W m^-2 over the recorded dates", file=sys.stderr)
    elif a.depths or occ is not None:
        ts = rt.thermal_column([a.point[0]], [a.point[1]], hz, ephemeris.sun_epochs(times, obs), ephemeris.sun_flux(times),
                               model, mode="column" if a.depths else "full", stats=st, occultation=occ)[0]
    else:
        ts = rt.surface_temperature([a.point[0]], [a.point[1]], hz, ephemeris.sun_epochs(times, obs),
                                    ephemeris.sun_flux(times), model, mode="full", stats=st)[0]
    if a.depths:
        print("time_utc," + ",".join(f"T_K_at_{z:.4f}_m" for z in rt.thermal_depths(model)))
        for t, v in zip(times[model.n_spin:], ts):
            print(f"{t.isoformat()}," + ",".join(f"{x:.4f}" for x in v))
    else:
        print("time_utc,surface_temperature_K")
        for t, v in zip(times[model.n_spin:], ts):
            print(f"{t.isoformat()},{v:.4f}")
    print(f"# {len(times)} epochs ({model.n_spin} spin-up) x {model.n_sub} steps: {st['kernel_ms']:.3f} ms of kernels",
          file=sys.stderr)
else:
    N, S, W, E = a.window
    la, lo = MoonRT.grid_nodes(lat=(N, S), lon=(W, E), shape=tuple(a.size))
    LA, LO = np.meshgrid(la, lo, indexing="ij")
    r = sunlight.surface_temperatures(rt, LA.ravel(), LO.ravel(), start, a.days, a.step_min, a.spinup_lunations, n_az,
                                      a.n_bis, obs, scatter=a.scatter, eclipses=a.eclipses)
    out = np.stack([r.t_max, r.t_min, r.t_mean, r.t_bottom_mean]).reshape(4, *a.size)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    np.save(a.out, out.astype(np.float32))
    print(f"{a.size[0]}x{a.size[1]} points x {len(r.times)} dates: {r.stats['kernel_ms']:.1f} ms of kernels in "
          f"{r.stats['launches']} launches; surface {float(r.t_min.min()):.1f}-{float(r.t_max.max()):.1f} K, share of points "
          f"below 110 K all the time {float((r.t_max < 110.0).mean()):.4f}; wrote {a.out}")
rt.close()
if dem_buf is not None:
    dem_buf.free()
