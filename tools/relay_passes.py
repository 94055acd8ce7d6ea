#!/usr/bin/env python3
"""When can a lander talk to a relay orbiter?  Coverage of a lat/lon window, or the pass table and the antenna pointing of one
point, against the terrain horizons from a mast top, headless.

  python tools/relay_passes.py --window -85 -90 -180 180 --size 256 256 --orbit 1837.4 0 90 0 0 0 --orbit 1837.4 0 90 90 0 180 \\
      --time 2026-01-01T00:00:00+00:00 --days 14 --step-s 30 --height 2 --min-elev 5 --out coverage.npy
  python tools/relay_passes.py --point -89.5 45.0 --orbit 8237.4 0.6 57 0 90 0 --days 3 > passes.csv
  python tools/relay_passes.py --point -89.5 45.0 --positions table.npy --pointing > pointing.csv
--orbit A_KM E INC RAAN ARGP M0 (degrees; repeatable) is propagated by orbits.kepler_fixed_positions (two-body with the secular
J2 drift: planning accuracy); --positions is the caller's own (S, m, 3) or (m, 3) table of Moon-fixed metres, one row per
--step-s from --time on.  coverage.npy holds an (8, h, w) float32 array: the share of dates with a satellite in view, the share
with two or more, the mean number in view, the longest outage and the longest contact in hours, the index of that contact's
first date (-1: none), the contacts per day and the highest culmination in degrees.  --point prints satellite, AOS, LOS,
duration_s, max_elev_deg, min_range_km per pass as CSV (with --pointing: time, satellite, azimuth_deg, elevation_deg, range_km,
margin_deg per date in view) and the summary line on stderr.  Synthetic LOLA-like DEM unless --elevation-file is given."""
import argparse, os, sys
from datetime import datetime, timedelta
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
from moonrtx_amd import orbits
from moonrtx_amd.renderer import MoonRT, synth_ldem, dem_from_ldem
from moonrtx_amd.scene import named_scene

ap = argparse.ArgumentParser()
ap.add_argument("--window", type=float, nargs=4, default=None, metavar=("LAT0", "LAT1", "LON0", "LON1"))
ap.add_argument("--size", type=int, nargs=2, default=(256, 256), metavar=("H", "W"))
ap.add_argument("--point", type=float, nargs=2, default=None, metavar=("LAT", "LON"))
ap.add_argument("--orbit", type=float, nargs=6, action="append", default=None, metavar=("A_KM", "E", "INC", "RAAN", "ARGP", "M0"))
ap.add_argument("--positions", default=None, help=".npy table of Moon-fixed metres, (S, m, 3) or (m, 3)")
ap.add_argument("--time", default="2026-01-01T00:00:00+00:00", help="first date, ISO 8601 with UTC offset")
ap.add_argument("--days", type=float, default=14.0)
ap.add_argument("--step-s", type=float, default=30.0)
ap.add_argument("--height", type=float, default=0.0, help="mast height above the ground, metres")
ap.add_argument("--min-elev", type=float, default=5.0, help="elevation mask above the local horizontal, degrees")
ap.add_argument("--pointing", action="store_true", help="with --point: the per-date azimuth, elevation and range")
ap.add_argument("--n-az", type=int, default=256)
ap.add_argument("--n-bis", type=int, default=14)
ap.add_argument("--downscale", type=int, default=2)
ap.add_argument("--dem-size", type=int, nargs=2, default=None, help="synthetic DEM (h, w); default 46080/downscale x 92160/downscale")
ap.add_argument("--elevation-file", default=None)
ap.add_argument("--out", default="coverage.npy")
a = ap.parse_args()
if (a.window is None) == (a.point is None):
    ap.error("give exactly one of --window and --point")
if (a.orbit is None) == (a.positions is None):
    ap.error("give --orbit (one or more) or --positions")
if a.pointing and a.point is None:
    ap.error("--pointing goes with --point")

start = datetime.fromisoformat(a.time)
if a.positions:
    pos = np.load(a.positions).astype(np.float64)
    pos = pos[None] if pos.ndim == 2 else pos
else:
    m = int(round(a.days * 86400.0 / a.step_s))
    pos = np.stack([orbits.kepler_fixed_positions(orbits.Elements(o[0] * 1e3, o[1], o[2], o[3], o[4], o[5], start), start, m, a.step_s)
                    for o in a.orbit])
S, m = pos.shape[:2]

if a.elevation_file:
    from moonrtx_amd.ingest import load_elevation_data
    dem, _ = load_elevation_data(a.elevation_file, a.downscale, device=0)
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
rt.apply_scene(named_scene("S1", 16, 16))       # the march parameters and Moon radius of scene S1
rt.set_params(flags=0)
n_az = 1 << max(2, int(np.ceil(np.log2(a.n_az))))
if a.point is not None:
    la, lo = [a.point[0]], [a.point[1]]
    r = orbits.relay_passes(rt, la, lo, pos, start, a.step_s, a.height, a.min_elev, n_az, a.n_bis, list_passes=True)
    if a.pointing:
        hz = rt.horizon(la, lo, n_az=n_az, n_bis=a.n_bis, height_m=a.height)
        full = rt.horizon_passes(la, lo, hz, pos, mode="full", height_m=a.height, min_elev_deg=a.min_elev)[0]
        print("time,satellite,azimuth_deg,elevation_deg,range_km,margin_deg")
        for k in range(m):
            for s in range(S):
                es, az, rng, g = full[s, k]
                if g > 0:
                    print(f"{r.times[k].isoformat()},{s},{az:.4f},{es:.4f},{rng / 1e3:.3f},{g:.4f}")
    else:
        print("satellite,aos,los,duration_s,max_elev_deg,min_range_km")
        p = r.passes
        for rec, t0, t1, d in zip(p.records, p.aos, p.los, p.duration_s):
            print(f"{rec['sat']},{t0.isoformat()},{t1.isoformat()},{d:.1f},{rec['max_elev_deg']:.3f},{rec['min_range_m'] / 1e3:.3f}")
    k = int(r.first_contact[0])
    best = "none" if k < 0 else f"{r.longest_contact_h[0]:.2f} h from {r.times[k].isoformat()}"
    print(f"# {S} satellites x {m} dates at {a.height} m above a {a.min_elev} deg mask: in view {r.share_any[0]:.4f} of the time, "
          f"{len(r.passes.records)} passes, {r.contacts_per_day[0]:.2f} contacts per day; longest contact {best}; longest outage "
          f"{r.longest_outage_h[0]:.2f} h; highest culmination {r.max_elev_deg[0]:.2f} deg", file=sys.stderr)
else:
    la, lo = MoonRT.grid_nodes(lat=tuple(a.window[:2]), lon=tuple(a.window[2:]), shape=tuple(a.size))
    LA, LO = np.meshgrid(la, lo, indexing="ij")
    r = orbits.relay_passes(rt, LA.ravel(), LO.ravel(), pos, start, a.step_s, a.height, a.min_elev, n_az, a.n_bis)
    out = np.stack([r.share_any, r.share_two, r.mean_in_view, r.longest_outage_h, r.longest_contact_h, r.first_contact,
                    r.contacts_per_day, r.max_elev_deg]).astype(np.float32).reshape(8, *a.size)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    np.save(a.out, out)
    print(f"{a.size[0]}x{a.size[1]} points x {S} satellites x {m} dates at {a.height} m: {r.stats['kernel_ms']:.1f} ms of kernels in "
          f"{r.stats['launches']} launches; mean share in view {float(r.share_any.mean()):.4f}, longest outage "
          f"{float(r.longest_outage_h.max()):.1f} h; wrote {a.out}")
rt.close()
if dem_buf is not None:
    dem_buf.free()
