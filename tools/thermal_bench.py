#!/usr/bin/env python3
"""Measure the surface-temperature stage on one GPU: thermal_kernel in SUMMARY over a polar window
for a year of hourly epochs with the default spin-up, the same year without spin-up (the difference is the spin-up's share),
and FULL / SUMMARY / FLUX on the first --small-points points.  Horizons come from horizon_kernel into a device buffer first.
--volatile times VOLATILE (mrtx_thermal_column, section 4.17) beside SUMMARY through mrtx_thermal on those points, --repeat
runs each, alternating.  Kernel times come from the library's HIP events.

  python tools/thermal_bench.py --dem-size 23040 46080 --size 1024 1024 --days 365
"""
import argparse, json, os, sys, time
from datetime import datetime, timedelta, timezone
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
from moonrtx_amd import ephemeris, thermal
from moonrtx_amd.renderer import DeviceBuffer, MoonRT, synth_ldem, dem_from_ldem
from moonrtx_amd.scene import named_scene

ap = argparse.ArgumentParser()
ap.add_argument("--dem-size", type=int, nargs=2, default=(23040, 46080))
ap.add_argument("--window", type=float, nargs=4, default=(-80.0, -90.0, -180.0, 180.0), metavar=("N", "S", "W", "E"))
ap.add_argument("--size", type=int, nargs=2, default=(1024, 1024))
ap.add_argument("--n-az", type=int, default=256)
ap.add_argument("--n-bis", type=int, default=14)
ap.add_argument("--days", type=float, default=365.0)
ap.add_argument("--spinup-lunations", type=int, default=thermal.SPINUP_LUNATIONS)
ap.add_argument("--small-points", type=int, default=65536, help="points of the FULL / FLUX / small SUMMARY measurements")
ap.add_argument("--skip-large", action="store_true", help="only the small-point measurements")
ap.add_argument("--repeat", type=int, default=2)
ap.add_argument("--volatile", action="store_true", help="also VOLATILE beside SUMMARY on the small points, alternating")
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
P = LA.size if not a.skip_large else min(LA.size, a.small_points)
LA, LO = LA[:P], LO[:P]
md = MoonRT.thermal_grid(3600.0, a.spinup_lunations)
md0 = MoonRT.thermal_grid(3600.0, 0, 0)
m_rec = int(round(a.days * 24))
t0 = datetime(2025, 1, 1, tzinfo=timezone.utc)
times = [t0 + timedelta(hours=k - md.n_spin) for k in range(md.n_spin + m_rec)]
t = time.perf_counter()
ep = ephemeris.sun_epochs(times, ephemeris.Observer(52.2, 21.0, 0.0))
fl = ephemeris.sun_flux(times)
res = dict(points=P, n_az=a.n_az, n_bis=a.n_bis, epochs=len(times), spin_epochs=md.n_spin, n_sub=md.n_sub,
           n_nodes=md.n_nodes, ephemeris_s=time.perf_counter() - t)
buf = DeviceBuffer(P * a.n_az * 4)
st = {}
rt.horizon(LA, LO, n_az=a.n_az, n_bis=a.n_bis, stats=st, out=buf)
res["horizon_ms"] = st["kernel_ms"]
steps_per_point = lambda mm: mm * md.n_sub * (md.n_nodes - 2)        # interior node updates
for name, npts, model, e, f in (("summary_spin", P, md, ep, fl), ("summary_nospin", P, md0, ep[md.n_spin:], fl[md.n_spin:]),
                                ("small_summary_spin", min(P, a.small_points), md, ep, fl)):
    if a.skip_large and not name.startswith("small"):
        continue
    for rep in range(a.repeat):
        st = {}
        s_ = rt.surface_temperature(LA[:npts], LO[:npts], buf, e, f, model, mode="summary", stats=st, n_az=a.n_az)
        res.setdefault(name + "_ms", []).append(st["kernel_ms"])
        res[name + "_caps"] = st["newton_cap_hits"]
    res[name + "_node_updates_per_s"] = npts * steps_per_point(e.shape[0]) / (min(res[name + "_ms"]) * 1e-3)
    res[name + "_range"] = [float(s_[:, 1].min()), float(s_[:, 0].max()), float(s_[:, 2].mean()), float(s_[:, 3].mean())]
ns = min(P, a.small_points)
m_full = min(m_rec, 720)
for name, mode, e, f, model in (("small_full_month", "full", ep[:md.n_spin + m_full], fl[:md.n_spin + m_full], md),
                                ("small_flux_month", "flux", ep[md.n_spin:md.n_spin + m_full], fl[md.n_spin:md.n_spin + m_full],
                                 md)):
    for rep in range(a.repeat):
        st = {}
        rt.surface_temperature(LA[:ns], LO[:ns], buf, e, f, model, mode=mode, stats=st, n_az=a.n_az)
        res.setdefault(name + "_ms", []).append(st["kernel_ms"])
if a.volatile:
    from moonrtx_amd import volatiles
    for rep in range(a.repeat):
        st = {}
        rt.surface_temperature(LA[:ns], LO[:ns], buf, ep, fl, md, mode="summary", stats=st, n_az=a.n_az)
        res.setdefault("alt_summary_ms", []).append(st["kernel_ms"])
        st = {}
        v_ = rt.thermal_column(LA[:ns], LO[:ns], buf, ep, fl, md, mode="volatile", species=volatiles.H2O, stats=st, n_az=a.n_az)
        res.setdefault("alt_volatile_ms", []).append(st["kernel_ms"])
    res["volatile_over_summary"] = min(res["alt_volatile_ms"]) / min(res["alt_summary_ms"])
    depth = volatiles.stability_depth(v_[:, :, 0], MoonRT.thermal_depths(md))
    res["volatile_depth_share"] = dict(surface=float((depth == 0.0).mean()), buried=float(np.isfinite(depth).mean()),
                                       never=float(np.isinf(depth).mean()))
if "summary_spin_ms" in res:
    res["spinup_share"] = 1.0 - min(res["summary_nospin_ms"]) / min(res["summary_spin_ms"])
buf.free()
rt.close()
dem.free()
print(json.dumps(res))
if a.out:
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
