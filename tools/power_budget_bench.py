#!/usr/bin/env python3
"""Measure the site power budget on one GPU, over a polar window of the full-size DEM and a year of
hourly epochs: power_budget_kernel's SUMMARY against what it replaces -- mrtx_horizon_sun FULL, its read-back and the numpy
reduction of the energy balance on the host (a loop over the dates, vectorised over the points; its time is reported for
--reduce-points points and scaled) -- alternating, so that the spread between runs of one path is seen beside the
difference, with the eight columns of the two paths compared bit for bit on the reduced points in every run and SUMMARY's
output compared between runs; a difference ends the tool with an error before any time is reported.  Kernel times come from the
library's HIP events; wall times are a host clock around calls that end in a synchronise and a read-back.

  python tools/power_budget_bench.py --dem-size 23040 46080 --size 256 256 --n-az 256 --n-bis 14 --days 365
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
ap.add_argument("--window", type=float, nargs=4, default=(-84.0, -90.0, -180.0, 180.0), metavar=("N", "S", "W", "E"))
ap.add_argument("--size", type=int, nargs=2, default=(256, 256))
ap.add_argument("--n-az", type=int, default=256)
ap.add_argument("--n-bis", type=int, default=14)
ap.add_argument("--days", type=float, default=365.0)
ap.add_argument("--step-min", type=float, default=60.0)
ap.add_argument("--height", type=float, default=2.0)
ap.add_argument("--area", type=float, default=2.0)
ap.add_argument("--eff", type=float, default=0.29)
ap.add_argument("--load", type=float, default=150.0)
ap.add_argument("--capacity-wh", type=float, default=5000.0)
ap.add_argument("--repeat", type=int, default=3)
ap.add_argument("--reduce-points", type=int, default=4096, help="points of the host reduction that is timed and scaled")
ap.add_argument("--out", default=None, help="write the numbers as JSON here")
a = ap.parse_args()


def reduce_on_host(f, gen, load, cpw, cap, ini):
    """The eight columns of section 3.17 from FULL fractions (P, m) for a tracking panel: the counts as the kernel rounds them,
    then the balance date by date, vectorised over the points."""
    scale = np.float32(2.0 ** cpw)
    G = np.rint((gen.astype(np.float32)[None, :] * f) * scale).astype(np.int64)
    L = np.rint(load.astype(np.float32) * scale).astype(np.int64)
    P, m = G.shape
    S = np.zeros(P, np.int64); peak = np.zeros(P, np.int64); peak_at = np.full(P, -1, np.int64)
    D = np.zeros(P, np.int64); first = np.full(P, -1, np.int64); last = np.full(P, -1, np.int64)
    s = np.full(P, ini, np.int64); min_s = np.full(P, np.iinfo(np.int64).max); n_un = np.zeros(P, np.int64); un = np.zeros(P, np.int64)
    for k in range(m):
        e = G[:, k] - L[k]
        S += e
        d = peak - S
        up = d > D
        D = np.where(up, d, D); first = np.where(up, peak_at + 1, first); last = np.where(up, k, last)
        top = S >= peak
        peak = np.where(top, S, peak); peak_at = np.where(top, k, peak_at)
        t = s + e
        s = np.minimum(cap, np.maximum(0, t))
        min_s = np.minimum(min_s, s)
        n_un += t < 0
        un += np.maximum(0, -t)
    return np.stack([G.sum(1), S, D, first, last, min_s, n_un, un], -1)


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
times = [t0 + timedelta(minutes=k * a.step_min) for k in range(m)]
t = time.perf_counter()
ep = ephemeris.sun_epochs(times, ephemeris.Observer(52.2, 21.0, 0.0))
gen = ephemeris.sun_flux(times) * (a.area * a.eff)
load = np.full(m, a.load)
res = dict(points=P, n_az=a.n_az, n_bis=a.n_bis, epochs=m, height_m=a.height, ephemeris_s=time.perf_counter() - t)
cpw = MoonRT.power_scale(gen, load)
cap = int(round(a.capacity_wh * 2.0 ** cpw / (a.step_min / 60.0)))
res["cpw_log2"], res["capacity_counts"] = cpw, cap
buf = DeviceBuffer(P * a.n_az * 4)
st = {}
rt.horizon(LA, LO, n_az=a.n_az, n_bis=a.n_bis, out=buf, height_m=a.height, stats=st)
res["horizon_ms"] = st["kernel_ms"]
kw = dict(panel="track", cpw_log2=cpw, capacity=cap, n_az=a.n_az)
rt.power_budget(LA[:1024], LO[:1024], buf, ep, gen, load, **kw)                          # warm-up: code objects
rt.horizon_sun(LA[:1024], LO[:1024], buf, ep, n_az=a.n_az)
nr, first = min(a.reduce_points, P), None
sel = np.arange(nr) * (P // nr)                 # the reduced points, spread over the window
for rep in range(a.repeat):                     # alternating: SUMMARY, the FULL call it replaces
    st = {}
    t = time.perf_counter()
    w = rt.power_budget(LA, LO, buf, ep, gen, load, stats=st, **kw)
    res.setdefault("summary_wall_s", []).append(time.perf_counter() - t)
    res.setdefault("summary_ms", []).append(st["kernel_ms"])
    st = {}
    t = time.perf_counter()
    f = rt.horizon_sun(LA, LO, buf, ep, stats=st, n_az=a.n_az, chunk_bytes=1 << 30)
    res.setdefault("full_wall_s", []).append(time.perf_counter() - t)
    res.setdefault("full_ms", []).append(st["kernel_ms"])
    res["full_launches"] = st["launches"]
    t = time.perf_counter()
    want = reduce_on_host(f[sel], gen, load, cpw, cap, cap)
    res.setdefault("reduce_s", []).append(time.perf_counter() - t)
    if not np.array_equal(w[sel], want):        # no time is reported for wrong bits
        bad = np.argwhere(w[sel] != want)
        i, j = bad[0]
        sys.exit(f"run {rep}: SUMMARY differs from the reduction of FULL in {len(bad)} entries, first at point {sel[i]} "
                 f"column {j}: {w[sel[i], j]} for {want[i, j]}")
    if first is None:
        first = w
    elif not np.array_equal(w, first):
        sys.exit(f"run {rep}: SUMMARY differs from run 0")
res["summary_device_bytes"] = P * (a.n_az * 4 + 64) + m * (32 + 4 + 4)
res["full_output_bytes"] = P * m * 4
res["reduce_points"], res["reduce_est_s"] = nr, [dt * P / nr for dt in res["reduce_s"]]
res["summary_equals_reduction"] = True          # checked in every run above: all eight columns of the reduced points
wh = 2.0 ** -cpw * (a.step_min / 60.0)
res["storage_need_wh"] = [float(w[:, 2].min() * wh), float(w[:, 2].max() * wh), float(w[:, 2].mean() * wh)]
res["points_with_unmet_load"] = int((w[:, 6] > 0).sum())
buf.free()
rt.close()
dem.free()
print(json.dumps(res))
if a.out:
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
