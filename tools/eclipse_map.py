#!/usr/bin/env python3
"""The Earth's occultation of the Sun over a lat/lon window, or per date at one point, headless.

  python tools/eclipse_map.py --time 2025-03-14T06:00:00+00:00 --window 90 -90 -180 180 --size 180 360 --out g.npy
  python tools/eclipse_map.py --time 2025-03-14T03:40:00+00:00 --span-min 400 --step-min 1 --size 180 360 --out summary.npy
  python tools/eclipse_map.py --point 0 0 --time 2025-03-14T03:40:00+00:00 --span-min 400 --step-min 2 > g.csv
g.npy holds an (h, w) float32 array at the window's nodes (MoonRT.grid_nodes): the share of the Sun's disc that the Earth's
disc leaves uncovered at --time, geometric discs only (no atmosphere), whether or not the point's own horizon shows the Sun.
With --span-min and --step-min it holds (8, h, w): the SUMMARY columns MoonRT.OCCULTATION_COLUMNS over the dates.  --point
prints time, g per date as CSV.  Synthetic LOLA-like DEM unless --elevation-file is given."""
import argparse, os, sys
from datetime import datetime, timedelta
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
from moonrtx_amd import ephemeris
from moonrtx_amd.renderer import MoonRT, synth_ldem, dem_from_ldem
from moonrtx_amd.scene import named_scene

ap = argparse.ArgumentParser()
ap.add_argument("--window", type=float, nargs=4, default=(90.0, -90.0, -180.0, 180.0), metavar=("N", "S", "W", "E"))
ap.add_argument("--size", type=int, nargs=2, default=(180, 360), metavar=("H", "W"))
ap.add_argument("--point", type=float, nargs=2, default=None, metavar=("LAT", "LON"))
ap.add_argument("--time", default="2025-03-14T06:00:00+00:00", help="the date, or the first one, ISO 8601 with UTC offset")
ap.add_argument("--span-min", type=float, default=0.0, help="dates over this many minutes (0: the one date)")
ap.add_argument("--step-min", type=float, default=1.0)
ap.add_argument("--lat", type=float, default=52.2, help="observer (the ephemeris' topocentric frame)")
ap.add_argument("--lon", type=float, default=21.0)
ap.add_argument("--downscale", type=int, default=8)
ap.add_argument("--dem-size", type=int, nargs=2, default=None, help="synthetic DEM (h, w); default 46080/downscale x 92160/downscale")
ap.add_argument("--elevation-file", default=None)
ap.add_argument("--out", default="g.npy")
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
rt.apply_scene(named_scene("S1", 16, 16))      # the Moon radius and vertex lift of scene S1; the bodies come from the ephemeris
rt.set_params(flags=0)
obs = ephemeris.Observer(a.lat, a.lon, 0.0)
start = datetime.fromisoformat(a.time)
m = max(1, int(a.span_min // a.step_min) + 1 if a.span_min > 0 else 1)
times = [start + timedelta(minutes=k * a.step_min) for k in range(m)]
sun, earth = ephemeris.sun_earth_epochs(times, obs)
far = ephemeris.far_sun_epochs(sun, times)
st = {}
if a.point is not None:
    g = rt.occultation([a.point[0]], [a.point[1]], far, earth, stats=st)[0]
    print("time_utc,g")
    for t, v in zip(times, g):
        print(f"{t.isoformat()},{v:.6f}")
    print(f"# {m} dates: least g {float(g.min()):.4f}, {int((g == 0).sum())} with the Sun wholly covered", file=sys.stderr)
else:
    N, S, W, E = a.window
    la, lo = MoonRT.grid_nodes(lat=(N, S), lon=(W, E), shape=tuple(a.size))
    LA, LO = np.meshgrid(la, lo, indexing="ij")
    if m == 1:
        out = rt.occultation(LA.ravel(), LO.ravel(), far, earth, stats=st).reshape(*a.size)
        note = f"g {float(out.min()):.4f} to {float(out.max()):.4f}, wholly covered at {float((out == 0).mean()):.4f} of the nodes"
    else:
        r = rt.occultation(LA.ravel(), LO.ravel(), far, earth, summary=True, stats=st)
        out = np.ascontiguousarray(r.T).reshape(8, *a.size)
        note = (f"least g {float(r[:, 1].min()):.4f}, longest cover {float(r[:, 6].max()) * a.step_min:.0f} min, "
                f"{int(r[:, 7].max())} eclipse(s)")
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    np.save(a.out, out.astype(np.float32))
    print(f"{a.size[0]}x{a.size[1]} nodes x {m} date(s): {st['kernel_ms']:.3f} ms of kernels in {st['launches']} launches; {note}; "
          f"wrote {a.out}")
rt.close()
if dem_buf is not None:
    dem_buf.free()
