#!/usr/bin/env python3
"""Measure the line-of-sight stage on one GPU: 1024 x 1024 viewsheds on the full-size synthetic DEM
for a local observer (a 50 km window about a 10 m mast), a whole-window observer (a 300 km window seen from a point inside
it) and an orbital one (1e8 m above a far point), each plain (n_bis = 0) and with mast bisections (n_bis = 12).  Kernel times
come from the library's HIP events.

  python tools/viewshed_bench.py --out profiles/viewshed_bench.json
"""
import argparse, json, math, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
from moonrtx_amd.renderer import MoonRT, synth_ldem, dem_from_ldem
from moonrtx_amd.scene import named_scene

ap = argparse.ArgumentParser()
ap.add_argument("--dem-size", type=int, nargs=2, default=(23040, 46080))
ap.add_argument("--size", type=int, nargs=2, default=(1024, 1024))
ap.add_argument("--mast-max", type=float, default=2000.0)
ap.add_argument("--repeat", type=int, default=3)
ap.add_argument("--out", default=None, help="write the numbers as JSON here")
a = ap.parse_args()

dh, dw = a.dem_size
src = synth_ldem(dh, dw)
dem, scale = dem_from_ldem(src, dh, dw, 1)
src.free()
rt = MoonRT(16, 16)
rt.bind_dem(dem, dh, dw)
rt.apply_scene(named_scene("S1", 16, 16))      # march parameters and Moon radius of S1 (step 5e-3, scene_epsilon 1e-4, R 10)
rt.set_params(flags=0)
radius_m = 1737400.0 * scale


def box(lat0, lon0, km):
    dl = math.degrees(km * 1e3 / radius_m) / 2
    return dict(lat=(lat0 + dl, lat0 - dl), lon=(lon0 - dl / math.cos(math.radians(lat0)), lon0 + dl / math.cos(math.radians(lat0))))


cases = {
    "local_50km": ((-45.0, 30.0, 10.0), box(-45.0, 30.0, 50.0)),
    "window_300km": ((-45.2, 30.3, 10.0), box(-45.0, 30.0, 300.0)),
    "orbital": ((-30.0, 50.0, 1e8), box(-45.0, 30.0, 300.0)),
}
res = dict(dem=[dh, dw], size=list(a.size), mast_max_m=a.mast_max, radius_m=radius_m)
targets = a.size[0] * a.size[1]
for name, (obs, g) in cases.items():
    for n_bis in (0, 12):
        key = f"{name}_nbis{n_bis}"
        ms = []
        for rep in range(a.repeat):
            st = {}
            v = rt.viewshed(obs, shape=tuple(a.size), mast_max_m=a.mast_max if n_bis else 0.0, n_bis=n_bis, radius_m=radius_m,
                            stats=st, **g)
            ms.append(st["kernel_ms"])
        rt.set_params(flags=1)
        st = {}
        rt.viewshed(obs, shape=tuple(a.size), mast_max_m=a.mast_max if n_bis else 0.0, n_bis=n_bis, radius_m=radius_m, stats=st,
                    **g)
        rt.set_params(flags=0)
        res[key] = dict(observer=list(obs), window=g, kernel_ms=ms, in_view=float((v == 0).mean()),
                        finite=float(np.isfinite(v).mean()), probes=int(st["shadow_rays"]),
                        probes_per_target=st["shadow_rays"] / targets,
                        steps_per_probe=(st["height_samples"] - 10 * targets) / max(st["shadow_rays"], 1),
                        probes_per_s=st["shadow_rays"] / (min(ms) * 1e-3))
        print(key, json.dumps(res[key]))
rt.close()
dem.free()
print(json.dumps(res))
if a.out:
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
