#!/usr/bin/env python3
"""Sun illumination map of the terrain for a date and an observer, headless: ephemeris -> light + Moon frame -> HIP
illumination stage -> PNG / .npy.

  python tools/illumination_map.py --time 2025-03-07T19:30:00+01:00 --lat 52.2 --lon 21.0 --window 90 -90 -180 180 \\
      --size 2048 4096 --n-sun 16 --out illum.png
  python tools/illumination_map.py ... --window -80 -90 -180 180 --frames 48 --step-min 720 --out polar.npy
(the reference's `--time/--lat/--lon` drive, main.py; synthetic LOLA-like DEM unless --elevation-file is given).
With --frames K the output is the mean `lit` over K dates --step-min minutes apart, the light and Moon frame updated per date:
the fraction of time each node sees the Sun.  Otherwise .npy holds the (h, w, 4) map (lit, irr, mu, D) and .png its `lit`.
Prints the kernel time and the counters (--count adds the deterministic ones: shadow rays, height samples)."""
import argparse, os, sys
from datetime import datetime, timedelta
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
from moonrtx_amd import ephemeris, _lib
from moonrtx_amd.renderer import MoonRT, synth_ldem, dem_from_ldem

ap = argparse.ArgumentParser()
ap.add_argument("--time", required=True, help="ISO 8601 with UTC offset")
ap.add_argument("--lat", type=float, required=True)
ap.add_argument("--lon", type=float, required=True)
ap.add_argument("--elevation-m", type=float, default=0.0)
ap.add_argument("--downscale", type=int, default=8)
ap.add_argument("--dem-size", type=int, nargs=2, default=None, help="synthetic DEM (h, w); default 46080/downscale x 92160/downscale")
ap.add_argument("--elevation-file", default=None)
ap.add_argument("--window", type=float, nargs=4, default=(90.0, -90.0, -180.0, 180.0), metavar=("N", "S", "W", "E"))
ap.add_argument("--terminator", type=float, default=None, metavar="DEG",
                help="instead of --window: a DEG x DEG window centred on the equator's evening terminator of the first date")
ap.add_argument("--size", type=int, nargs=2, default=(512, 1024), metavar=("H", "W"))
ap.add_argument("--n-sun", type=int, default=16)
ap.add_argument("--frames", type=int, default=1)
ap.add_argument("--step-min", type=float, default=60.0)
ap.add_argument("--count", action="store_true", help="maintain the deterministic counters (the counting kernel)")
ap.add_argument("--repeat", type=int, default=1, help="time the first date this many times (kernel ms of each)")
ap.add_argument("--out", default="illum.png")
a = ap.parse_args()

ephemeris.init(ephemeris.Observer(a.lat, a.lon, a.elevation_m))
t0 = datetime.fromisoformat(a.time)
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
rt.set_params(flags=_lib.F_COUNT_STATS if a.count else 0)
N, S, Wl, E = a.window
if a.terminator:
    e0 = ephemeris.calculate_moon_ephemeris(t0, False)
    N, S, Wl, E = a.terminator / 2, -a.terminator / 2, e0.subsolar_lon + 90.0 - a.terminator / 2, e0.subsolar_lon + 90.0 + a.terminator / 2
acc = None
for k in range(max(1, a.frames)):
    eph = ephemeris.calculate_moon_ephemeris(t0 + timedelta(minutes=k * a.step_min), False)
    scene = ephemeris.scene_from_ephemeris(eph, 16, 16)
    rt.set_moon_frame(scene.center, scene.radius, scene.u, scene.v)
    rt.set_light(scene.light_pos, scene.light_radius, scene.light_radiance)
    for rep in range(a.repeat if k == 0 else 1):
        st = {}
        m = rt.illumination_map((N, S), (Wl, E), tuple(a.size), n_sun=a.n_sun, stats=st)
        rays = st.get("shadow_rays", 0)
        rate = f", {rays / st['kernel_ms'] / 1e6:.1f} G shadow rays/s" if rays else ""
        print(f"date {(t0 + timedelta(minutes=k * a.step_min)).isoformat()}: subsolar "
              f"({eph.subsolar_lat:+.3f}, {eph.subsolar_lon:+.3f}); {a.size[0]}x{a.size[1]} nodes x {a.n_sun} Sun samples: "
              f"{st['kernel_ms']:.3f} ms in {st['launches']} launch(es); counters {st}{rate}")
    acc = m[..., 0].astype(np.float64) if acc is None else acc + m[..., 0]
out = (acc / max(1, a.frames)).astype(np.float32) if a.frames > 1 else m
os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
if a.out.endswith(".npy"):
    np.save(a.out, out)
else:
    from PIL import Image
    lit = out if out.ndim == 2 else out[..., 0]
    Image.fromarray(np.clip(np.rint(lit * 255.0), 0, 255).astype(np.uint8)).save(a.out)
lit = out if out.ndim == 2 else out[..., 0]
print(f"wrote {a.out}; mean lit {float(lit.mean()):.4f}, nodes ever lit {float((lit > 0).mean()):.4f}")
rt.close()
if dem_buf is not None:
    dem_buf.free()
