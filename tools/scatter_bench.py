#!/usr/bin/env python3
"""Measure the terrain-scattered flux (DESIGN.md sections 3.11 and 4.12) on one GPU: view_hits_kernel's rays per second on
a polar window, the hit count and terrain share, and surface_temperatures(scatter=K) end to end with the time of each stage,
against scatter=0 on the same points.  Kernel times of the view hits come from the library's HIP events; stage times are host
clocks around calls that end in a device synchronise.

  python tools/scatter_bench.py --dem-size 23040 46080 --size 256 256 --k 64 --days 365 --out profiles/scatter_bench.json
"""
import argparse, json, os, sys, time
from datetime import datetime, timezone
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
from moonrtx_amd import ephemeris, sunlight, thermal
from moonrtx_amd.renderer import MoonRT, synth_ldem, dem_from_ldem
from moonrtx_amd.scene import named_scene

ap = argparse.ArgumentParser()
ap.add_argument("--dem-size", type=int, nargs=2, default=(23040, 46080))
ap.add_argument("--window", type=float, nargs=4, default=(-80.0, -90.0, -180.0, 180.0), metavar=("N", "S", "W", "E"))
ap.add_argument("--size", type=int, nargs=2, default=(256, 256))
ap.add_argument("--k", type=int, default=64)
ap.add_argument("--n-az", type=int, default=256)
ap.add_argument("--n-bis", type=int, default=14)
ap.add_argument("--days", type=float, default=365.0)
ap.add_argument("--spinup-lunations", type=int, default=thermal.SPINUP_LUNATIONS)
ap.add_argument("--budget-gb", type=float, default=8.0)
ap.add_argument("--repeat", type=int, default=2, help="repeats of the view-hit measurement")
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
res = dict(points=P, k=a.k, n_az=a.n_az, n_bis=a.n_bis, days=a.days, spinup_lunations=a.spinup_lunations,
           dem=[dh, dw], window=list(a.window), budget_gb=a.budget_gb, mapping="one lane per (point, j)")
rt.view_hits(LA[:256], LO[:256], k=a.k)        # warm-up
for rep in range(a.repeat):
    st = {}
    _, share = rt.view_hits(LA, LO, k=a.k, stats=st)
    res.setdefault("view_hits_ms", []).append(st["kernel_ms"])
res["view_rays_per_s"] = P * a.k / (min(res["view_hits_ms"]) * 1e-3)
res["terrain_share_mean"] = float(share.mean())
res["points_seeing_terrain"] = float((share > 0).mean())
t0 = datetime(2025, 1, 1, tzinfo=timezone.utc)
obs = ephemeris.Observer(52.2, 21.0, 0.0)
kw = dict(spinup_lunations=a.spinup_lunations, n_az=a.n_az, n_bis=a.n_bis, observer=obs)
t = time.perf_counter()
base = sunlight.surface_temperatures(rt, LA, LO, t0, a.days, **kw)
res["scatter0_s"] = time.perf_counter() - t
t = time.perf_counter()
scat = sunlight.surface_temperatures(rt, LA, LO, t0, a.days, scatter=a.k, budget_bytes=int(a.budget_gb * (1 << 30)), **kw)
res["scatter_s"] = time.perf_counter() - t
res["scatter_hits"] = int(scat.stats["scatter_hits"])
res["stage_s"] = scat.stats["stage_s"]
res["kernel_ms_total"] = scat.stats["kernel_ms"]
d = scat.t_mean - base.t_mean
res["t_mean_rise_K"] = dict(min=float(d.min()), max=float(d.max()), mean=float(d.mean()))
res["t_min_rise_K"] = dict(min=float((scat.t_min - base.t_min).min()), max=float((scat.t_min - base.t_min).max()))
cold = base.t_max < 40.0
res["never_warm_points"] = int(cold.sum())
if cold.any():
    res["never_warm_t_mean_K"] = dict(before=float(base.t_mean[cold].mean()), after=float(scat.t_mean[cold].mean()),
                                      after_min=float(scat.t_mean[cold].min()), after_max=float(scat.t_mean[cold].max()))
rt.close()
dem.free()
print(json.dumps(res))
if a.out:
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
