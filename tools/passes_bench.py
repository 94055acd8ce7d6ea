#!/usr/bin/env python3
"""Measure the orbiter passes on one GPU: a polar window, four relay satellites on 12-hour elliptical
orbits, 14 days at 30 s steps -- passes_summary_kernel and both launches of passes_list_kernel -- and, in the same run on the same
points, horizons and epoch count, horizon_windows_kernel, which the parent commit has: the yardstick.  The calls alternate, so
that the spread between runs of one kernel is seen beside the difference; the first call of each is a warm-up (code objects,
buffers).  Kernel times come from the library's HIP events.  The yardstick's two epoch tables are synthetic discs (0.27 and 0.95
deg) circling low over the polar horizon, where the Sun and the Earth stand.

  python tools/passes_bench.py --size 256 256 --days 14 --step-s 30 --out profiles/passes_bench.json --md profiles/passes.md
"""
import argparse, json, os, statistics, sys
from datetime import datetime, timezone
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
from moonrtx_amd import ephemeris, orbits
from moonrtx_amd.renderer import DeviceBuffer, MoonRT, synth_ldem, dem_from_ldem
from moonrtx_amd.scene import named_scene

ap = argparse.ArgumentParser()
ap.add_argument("--dem-size", type=int, nargs=2, default=(5760, 11520))
ap.add_argument("--window", type=float, nargs=4, default=(-84.0, -90.0, -180.0, 180.0), metavar=("N", "S", "W", "E"))
ap.add_argument("--size", type=int, nargs=2, default=(256, 256))
ap.add_argument("--n-az", type=int, default=256)
ap.add_argument("--n-bis", type=int, default=12)
ap.add_argument("--days", type=float, default=14.0)
ap.add_argument("--step-s", type=float, default=30.0)
ap.add_argument("--sats", type=int, default=4)
ap.add_argument("--min-elev", type=float, default=5.0)
ap.add_argument("--repeat", type=int, default=5)
ap.add_argument("--out", default=None, help="write the numbers as JSON here")
ap.add_argument("--md", default=None, help="write the table as markdown here")
a = ap.parse_args()

dh, dw = a.dem_size
src = synth_ldem(dh, dw)
dem, _ = dem_from_ldem(src, dh, dw, 1)
src.free()
rt = MoonRT(16, 16)
rt.bind_dem(dem, dh, dw)
s = named_scene("S1", 16, 16)
rt.apply_scene(s)
rt.set_params(flags=0)
la, lo = MoonRT.grid_nodes(lat=tuple(a.window[:2]), lon=tuple(a.window[2:]), shape=tuple(a.size))
LA, LO = [g.ravel() for g in np.meshgrid(la, lo, indexing="ij")]
P = LA.size
t0 = datetime(2026, 1, 1, tzinfo=timezone.utc)
m = int(round(a.days * 86400.0 / a.step_s))
S = a.sats
pos = np.stack([orbits.kepler_fixed_positions(orbits.Elements(6142.4e3, 0.6, 57.0, 360.0 * j / S, 90.0, 360.0 * j / S, t0), t0, m,
                                              a.step_s) for j in range(S)])
# the yardstick's tables: one ephemeris row's Moon frame, the light 2e4 R away on a slow circle 88 deg from the south pole:
# low over a polar horizon, as the Sun and the Earth stand there
row = ephemeris.sun_epochs([t0], ephemeris.Observer(52.2, 21.0, 0.0))[0]
ez = row[8:11] / np.linalg.norm(row[8:11])
v0 = row[11:14] - (row[11:14] @ ez) * ez
v0 /= np.linalg.norm(v0)
Mf = np.stack([np.cross(ez, v0), v0, ez])
ang = 2.0 * np.pi * np.arange(m) / 2000.0
dist = 2.0e4 * float(s.radius)


def discs(phase, radius_deg):
    c88, s88 = np.cos(np.radians(88.0)), np.sin(np.radians(88.0))
    d = np.stack([s88 * np.sin(ang + phase), s88 * np.cos(ang + phase), np.full(m, -c88)], -1)
    ep = np.tile(row, (m, 1))
    ep[:, 0:3] = row[5:8] + (dist * d) @ Mf
    ep[:, 3] = dist * np.sin(np.radians(radius_deg))
    return ep


ep_a, ep_b = discs(0.0, 0.27), discs(2.0, 0.95)
res = dict(points=P, n_az=a.n_az, n_bis=a.n_bis, epochs=m, satellites=S, min_elev_deg=a.min_elev, dem=[dh, dw])
buf = DeviceBuffer(P * a.n_az * 4)
st = {}
rt.horizon(LA, LO, n_az=a.n_az, n_bis=a.n_bis, out=buf, stats=st)
res["horizon_ms"] = st["kernel_ms"]
kw = dict(n_az=a.n_az, min_elev_deg=a.min_elev)
summ = recs = win = None
for rep in range(a.repeat + 1):                 # alternating: SUMMARY, LIST, the windows; round 0 is the warm-up
    st = {}
    summ = rt.horizon_passes(LA, LO, buf, pos, mode="summary", stats=st, **kw)
    st2 = {}
    recs = rt.horizon_passes(LA, LO, buf, pos, mode="list", stats=st2, **kw)
    st3 = {}
    win = rt.horizon_windows(LA, LO, buf, ep_a, ep_b, min_a=0.5, min_b=1.0, n_az=a.n_az, stats=st3)
    if rep:
        res.setdefault("summary_ms", []).append(st["kernel_ms"])
        res.setdefault("list_count_ms", []).append(st2["count_ms"])
        res.setdefault("list_fill_ms", []).append(st2["fill_ms"])
        res.setdefault("windows_ms", []).append(st3["kernel_ms"])
res["passes"] = int(len(recs))
res["share_in_view"] = float(summ[:, 0].mean())
res["windows_share_a"] = float(win[:, 0].mean())
evals = float(P) * S * m
med = lambda k: statistics.median(res[k])       # noqa: E731
res["ns_per_eval"] = dict(summary=med("summary_ms") * 1e6 / evals, list_count=med("list_count_ms") * 1e6 / evals,
                          list_fill=med("list_fill_ms") * 1e6 / evals, windows=med("windows_ms") * 1e6 / (float(P) * 2 * m))
res["summary_over_windows_per_eval"] = res["ns_per_eval"]["summary"] / res["ns_per_eval"]["windows"]
buf.free()
rt.close()
dem.free()
print(json.dumps(res))
if a.out:
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
if a.md:
    rows = [("passes_summary_kernel", "summary_ms", "summary", S), ("passes_list_kernel (count)", "list_count_ms", "list_count", S),
            ("passes_list_kernel (fill: count + fill launches)", "list_fill_ms", "list_fill", S),
            ("horizon_windows_kernel (two bodies)", "windows_ms", "windows", 2)]
    with open(a.md, "w") as fh:
        fh.write("# Orbiter passes (DESIGN.md 4.33)\n\n")
        fh.write(f"`tools/passes_bench.py`: {a.size[0]} x {a.size[1]} points of {a.window[0]} .. {a.window[1]} deg latitude on a {dh} x {dw} "
                 f"DEM, n_az = {a.n_az}, {S} satellites, {m} epochs ({a.days:g} days at {a.step_s:g} s), mask {a.min_elev:g} deg; "
                 f"{a.repeat} alternating rounds after a warm-up, kernel times from HIP events.  {res['passes']} passes; "
                 f"a satellite in view {res['share_in_view']:.3f} of the time.\n\n")
        fh.write("| kernel | median ms | min .. max ms | evaluations per (point, epoch) | ns per evaluation |\n|---|---|---|---|---|\n")
        for name, key, short, per in rows:
            fh.write(f"| `{name}` | {med(key):.2f} | {min(res[key]):.2f} .. {max(res[key]):.2f} | {per} | {res['ns_per_eval'][short]:.5f} |\n")
        fh.write(f"\nOne satellite evaluation costs {res['summary_over_windows_per_eval']:.2f} of one body of `horizon_windows_kernel` "
                 "(SUMMARY against the windows, per evaluation).\n")
