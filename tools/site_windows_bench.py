#!/usr/bin/env python3
"""Measure the mast-height horizon and the joint windows on one GPU, over a polar window of the
full-size DEM and a year of hourly epochs: horizon_raised_kernel at height 0 and at --height against horizon_kernel
(alternating, so that the spread between runs of one kernel is seen beside the difference), and horizon_windows_kernel
against what it replaces -- two FULL horizon_sun calls, their read-back and the numpy reduction on the host (the runs of the
reduction are a Python loop per point: its time is reported for --reduce-points points and scaled).  Kernel times come from the
library's HIP events; the FULL path's wall time is a host clock around calls that end in a synchronise and a read-back.

  python tools/site_windows_bench.py --dem-size 23040 46080 --size 256 256 --n-az 256 --n-bis 14 --days 365 --height 10
"""
import argparse, json, os, sys, time
from datetime import datetime, timedelta, timezone
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np
from moonrtx_amd import ephemeris
from moonrtx_amd.renderer import DeviceBuffer, MoonRT, synth_ldem, dem_from_ldem
from moonrtx_amd.scene import named_scene

ap = argparse.ArgumentParser()
ap.add_argument("--dem-size", type=int, nargs=2, default=(23040, 46080))
ap.add_argument("--window", type=float, nargs=4, default=(-84.0, -90.0, -180.0, 180.0), metavar=("N", "S", "W", "E"))
ap.add_argument("--size", type=int, nargs=2, default=(256, 256))
ap.add_argument("--n-az", type=int, default=256)
ap.add_argument("--n-bis", type=int, default=14)
ap.add_argument("--days", type=float, default=365.0)
ap.add_argument("--step-min", type=float, default=60.0)
ap.add_argument("--height", type=float, default=10.0)
ap.add_argument("--repeat", type=int, default=3)
ap.add_argument("--reduce-points", type=int, default=256, help="points of the host reduction that is timed and scaled")
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
ep_sun, ep_earth = ephemeris.sun_earth_epochs([t0 + timedelta(minutes=k * a.step_min) for k in range(m)],
                                              ephemeris.Observer(52.2, 21.0, 0.0))
res = dict(points=P, n_az=a.n_az, n_bis=a.n_bis, epochs=m, height_m=a.height, ephemeris_s=time.perf_counter() - t)
buf = DeviceBuffer(P * a.n_az * 4)
rt.horizon(LA[:4096], LO[:4096], n_az=a.n_az, n_bis=a.n_bis, out=buf)                    # warm-up: code objects
rt.horizon(LA[:4096], LO[:4096], n_az=a.n_az, n_bis=a.n_bis, out=buf, height_m=a.height)
ground = None
for rep in range(a.repeat):                     # alternating: ground, raised at 0, raised at --height
    for key, kw in (("horizon_points_ms", {}), ("horizon_raised_h0_ms", dict(height_m=0.0)),
                    ("horizon_raised_ms", dict(height_m=a.height))):
        st = {}
        rt.horizon(LA, LO, n_az=a.n_az, n_bis=a.n_bis, stats=st, out=buf, **kw)
        res.setdefault(key, []).append(st["kernel_ms"])
        if key != "horizon_raised_ms":
            hz = buf.download(np.float32, (P, a.n_az))
            if ground is None:
                ground = hz
            res["h0_bit_equal"] = bool(res.get("h0_bit_equal", True) and np.array_equal(hz.view(np.uint32), ground.view(np.uint32)))
hz = buf.download(np.float32, (P, a.n_az))      # the raised horizons: what the windows are measured on
res["horizon_range_raised"] = [float(hz.min()), float(hz.max()), float(hz.mean())]
res["horizon_range_ground"] = [float(ground.min()), float(ground.max()), float(ground.mean())]
rt.horizon_windows(LA[:1024], LO[:1024], buf, ep_sun, ep_earth, n_az=a.n_az)            # warm-up
rt.horizon_sun(LA[:1024], LO[:1024], buf, ep_sun, n_az=a.n_az)
for rep in range(a.repeat):                     # alternating: the windows call, the two FULL calls it replaces
    st = {}
    t = time.perf_counter()
    w = rt.horizon_windows(LA, LO, buf, ep_sun, ep_earth, min_a=0.5, min_b=1.0, stats=st, n_az=a.n_az)
    res.setdefault("windows_wall_s", []).append(time.perf_counter() - t)
    res.setdefault("windows_ms", []).append(st["kernel_ms"])
    st = {}
    t = time.perf_counter()
    fa = rt.horizon_sun(LA, LO, buf, ep_sun, stats=st, n_az=a.n_az, chunk_bytes=1 << 30)
    fb = rt.horizon_sun(LA, LO, buf, ep_earth, stats=st, n_az=a.n_az, chunk_bytes=1 << 30)
    res.setdefault("two_full_wall_s", []).append(time.perf_counter() - t)
    res.setdefault("two_full_ms", []).append(st["kernel_ms"])
    res["two_full_launches"] = st["launches"]
res["windows_device_bytes"] = P * (a.n_az + 8) * 4 + 2 * m * 32
res["two_full_output_bytes"] = 2 * P * m * 4
import mast_model                                # the numpy reduction of tests/mast_model.py: what a user would write
nr = min(a.reduce_points, P)
t = time.perf_counter()
want, cnt = mast_model.windows(fa[:nr], fb[:nr], 0.5, 1.0)
dt = time.perf_counter() - t
res["reduce_points"] = nr
res["reduce_s"] = dt
res["reduce_est_s"] = dt * P / nr
res["windows_equal_reduction"] = bool(np.array_equal(w[:nr, [1, 3, 5, 6, 7]], want[:, [1, 3, 5, 6, 7]].astype(np.float32)))
res["mean_shares"] = [float(w[:, j].mean()) for j in (0, 2, 4)]
res["longest_window_epochs"] = float(w[:, 5].max())
buf.free()
rt.close()
dem.free()
print(json.dumps(res))
if a.out:
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
