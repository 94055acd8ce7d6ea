#!/usr/bin/env python3
"""the Sun illumination series on the headline DEM (cfg3's synthetic 23040 x 46080), 1024 seeded
random points over the whole Moon, 30 days at 10-minute steps (4321 epochs), n_sun = 16.  Prints one JSON line:
  series_ms         the production kernel (HIP events), best of --repeat;
  count_ms          the counting build's kernel, with its shadow_rays / height_samples;
  grays_per_s       shadow_rays / series_ms;
  loop_wall_s       host clock of the per-date loop (set_moon_frame + set_light + illumination_at per epoch) for the same work,
                    loop_kernel_ms the sum of its kernels' HIP-event times;
  series_wall_s     host clock of one illumination_series call (upload, launch, read-back);
  epochs_s          host clock of ephemeris.sun_epochs for the 4321 dates;
  events_wall_s     host clock of sunlight.terrain_sun_events end to end, ephemeris included (with its event count).
  python tools/illum_series_bench.py [--points 1024] [--days 30] [--step-min 10] [--n-sun 16] [--series-only]"""
import argparse, json, os, sys, time
from datetime import datetime, timedelta, timezone
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
from moonrtx_amd import ephemeris, _lib
from moonrtx_amd.renderer import MoonRT, synth_ldem, dem_from_ldem
from moonrtx_amd.scene import named_scene
from moonrtx_amd.sunlight import terrain_sun_events

ap = argparse.ArgumentParser()
ap.add_argument("--points", type=int, default=1024)
ap.add_argument("--days", type=float, default=30.0)
ap.add_argument("--step-min", type=float, default=10.0)
ap.add_argument("--n-sun", type=int, default=16)
ap.add_argument("--repeat", type=int, default=5)
ap.add_argument("--dem-size", type=int, nargs=2, default=(23040, 46080))
ap.add_argument("--series-only", action="store_true", help="the series kernels alone (for a profiler run)")
a = ap.parse_args()

obs = ephemeris.Observer(52.2, 21.0, 0.0)
start = datetime(2025, 3, 1, tzinfo=timezone.utc)
m = int(round(a.days * 1440.0 / a.step_min)) + 1
times = [start + timedelta(minutes=a.step_min * k) for k in range(m)]
w = time.perf_counter()
ep = ephemeris.sun_epochs(times, obs)
epochs_s = time.perf_counter() - w
rng = np.random.default_rng(2025)
lat = np.degrees(np.arcsin(rng.uniform(-1.0, 1.0, a.points)))
lon = rng.uniform(-180.0, 180.0, a.points)

dh, dw = a.dem_size
src = synth_ldem(dh, dw)
dem, _ = dem_from_ldem(src, dh, dw, 1)
src.free()
s = named_scene("S1", 16, 16)
rt = MoonRT(16, 16)
rt.bind_dem(dem, dh, dw)
rt.apply_scene(s)
res = dict(points=a.points, epochs=m, n_sun=a.n_sun, dem=[dh, dw], epochs_s=round(epochs_s, 3))

rt.set_params(flags=_lib.F_COUNT_STATS)
st = {}
rt.illumination_series(lat, lon, ep, n_sun=a.n_sun, stats=st)
res.update(count_ms=round(st["kernel_ms"], 3), shadow_rays=int(st["shadow_rays"]), height_samples=int(st["height_samples"]))
rt.set_params(flags=0)
best, walls = None, []
for _ in range(max(1, a.repeat)):
    st = {}
    w = time.perf_counter()
    out = rt.illumination_series(lat, lon, ep, n_sun=a.n_sun, stats=st)
    walls.append(time.perf_counter() - w)
    best = st["kernel_ms"] if best is None else min(best, st["kernel_ms"])
res.update(series_ms=round(best, 3), series_wall_s=round(min(walls), 3),
           grays_per_s=round(res["shadow_rays"] / best / 1e6, 2), lit_share=round(float((out[..., 0] > 0).mean()), 4))
if not a.series_only:
    st = {}
    w = time.perf_counter()
    for k in range(m):
        rt.set_moon_frame(ep[k, 5:8], s.radius, ep[k, 8:11], ep[k, 11:14])
        rt.set_light(ep[k, 0:3], ep[k, 3], ep[k, 4])
        rt.illumination_at(lat, lon, n_sun=a.n_sun, stats=st)
    res["loop_wall_s"] = round(time.perf_counter() - w, 3)
    res["loop_kernel_ms"] = round(st["kernel_ms"], 3)
    res["loop_over_series_wall"] = round(res["loop_wall_s"] / res["series_wall_s"], 1)
    w = time.perf_counter()
    ev = terrain_sun_events(rt, lat, lon, start, a.days, step_min=a.step_min, n_sun=a.n_sun, refine=15, observer=obs)
    res.update(events_wall_s=round(time.perf_counter() - w, 3), events=len(ev.events),
               events_flicker=sum(e.flicker for e in ev.events), refine_ms=round(ev.refine.get("kernel_ms", 0.0), 3),
               refine_windows=len(ev.events))
rt.close()
dem.free()
print(json.dumps(res))
