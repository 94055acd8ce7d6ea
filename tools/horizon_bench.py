#!/usr/bin/env python3
"""Measure the horizon stage on one GPU: horizon_kernel over a polar window, horizon_sun_kernel in
both modes over a year of hourly epochs, and the direct alternative (illumination_series at 16 Sun samples) for a slice of
the same points and dates, scaled to the whole.  Kernel times come from the library's HIP events.

  python tools/horizon_bench.py --dem-size 23040 46080 --size 1024 1024 --n-az 256 --n-bis 14 --days 365
"""
import argparse, json, os, sys, time
from datetime import datetime, timedelta, timezone
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
from moonrtx_amd import ephemeris
from moonrtx_amd.renderer import DeviceBuffer, MoonRT, synth_ldem, dem_from_ldem
from moonrtx_amd.scene import named_scene

ap = argparse.ArgumentParser()
ap.add_argument("--dem-size", type=int, nargs=2, default=(23040, 46080))
ap.add_argument("--window", type=float, nargs=4, default=(-80.0, -90.0, -180.0, 180.0), metavar=("N", "S", "W", "E"))
ap.add_argument("--size", type=int, nargs=2, default=(1024, 1024))
ap.add_argument("--n-az", type=int, default=256)
ap.add_argument("--n-bis", type=int, default=14)
ap.add_argument("--days", type=float, default=365.0)
ap.add_argument("--step-min", type=float, default=60.0)
ap.add_argument("--chunk", type=int, default=1 << 17, help="points per horizon call")
ap.add_argument("--full-points", type=int, default=65536, help="points of the FULL-mode measurement")
ap.add_argument("--direct-points", type=int, default=4096, help="points x --direct-dates of the direct series, scaled up")
ap.add_argument("--direct-dates", type=int, default=1024)
ap.add_argument("--repeat", type=int, default=2)
ap.add_argument("--out", default=None, help="write the numbers as JSON here")
a = ap.parse_args()

dh, dw = a.dem_size
src = synth_ldem(dh, dw)
dem, _ = dem_from_ldem(src, dh, dw, 1)
src.free()
rt = MoonRT(16, 16)
rt.bind_dem(dem, dh, dw)
rt.apply_scene(named_scene("S1", 16, 16))      # march parameters and Moon radius of S1 (step 5e-3, scene_epsilon 1e-4, R 10)
rt.set_params(flags=0)
la, lo = MoonRT.grid_nodes(lat=tuple(a.window[:2]), lon=tuple(a.window[2:]), shape=tuple(a.size))
LA, LO = [g.ravel() for g in np.meshgrid(la, lo, indexing="ij")]
P = LA.size
t0 = datetime(2025, 1, 1, tzinfo=timezone.utc)
m = int(round(a.days * 1440.0 / a.step_min))
t = time.perf_counter()
ep = ephemeris.sun_epochs([t0 + timedelta(minutes=k * a.step_min) for k in range(m)], ephemeris.Observer(52.2, 21.0, 0.0))
res = dict(points=P, n_az=a.n_az, n_bis=a.n_bis, epochs=m, ephemeris_s=time.perf_counter() - t)
buf = DeviceBuffer(P * a.n_az * 4)
probes = P * a.n_az * a.n_bis
for rep in range(a.repeat):
    st = {}
    t = time.perf_counter()
    rt.horizon(LA, LO, n_az=a.n_az, n_bis=a.n_bis, stats=st, out=buf)
    res.setdefault("horizon_ms", []).append(st["kernel_ms"])
    res.setdefault("horizon_host_s", []).append(time.perf_counter() - t)
    res.setdefault("horizon_probes_per_s", []).append(probes / (st["kernel_ms"] * 1e-3))
    res["horizon_launches"] = st["launches"]
hz = buf.download(np.float32, (P, a.n_az))
res["horizon_range"] = [float(hz.min()), float(hz.max()), float(hz.mean())]
for rep in range(a.repeat):
    st = {}
    s_ = rt.horizon_sun(LA, LO, buf, ep, summary=True, stats=st, n_az=a.n_az)
    res.setdefault("sun_summary_ms", []).append(st["kernel_ms"])
res["mean_lit_share"] = float(s_[:, 1].mean())
nf = min(a.full_points, P)
for rep in range(a.repeat):
    st = {}
    f_ = rt.horizon_sun(LA[:nf], LO[:nf], buf, ep, stats=st, n_az=a.n_az)
    res.setdefault("sun_full_ms", []).append(st["kernel_ms"])
res["sun_full_points"] = nf
res["sun_full_GBps"] = [nf * m * 4 / (x * 1e-3) / 1e9 for x in res["sun_full_ms"]]
del f_
dp, dd = min(a.direct_points, P), min(a.direct_dates, m)
for rep in range(a.repeat):
    st = {}
    rt.illumination_series(LA[:dp], LO[:dp], ep[:dd], n_sun=16, stats=st)
    res.setdefault("direct_slice_ms", []).append(st["kernel_ms"])
scale = (P / dp) * (m / dd)
res["direct_slice"] = [dp, dd]
res["direct_year_est_s"] = min(res["direct_slice_ms"]) * scale * 1e-3
per_date_direct = min(res["direct_slice_ms"]) * (P / dp) / dd          # ms per date for all P points
per_date_sun = min(res["sun_summary_ms"]) / m
res["break_even_dates"] = min(res["horizon_ms"]) / max(per_date_direct - per_date_sun, 1e-9)
buf.free()
rt.close()
dem.free()
print(json.dumps(res))
if a.out:
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
