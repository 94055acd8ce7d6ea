"""Timed traverse and drive mask timings on the full-size DEM -> profiles/timed_traverse_bench.json.

A 2048 x 2048 mid-latitude window: mrtx_traverse, mrtx_traverse_timed without a table, with an all-ones table and with a
moving-night table of 720 hourly epochs; a wrapped south-polar cap with all ones and the moving night; then mrtx_horizon_mask
against mrtx_horizon_windows on 65 536 points x 8 760 epochs.  Per row the best of --repeats runs after a warm-up run: kernel ms
(HIP events around the stage's launches), relaxation launches, tile visits."""
import argparse
import json
import os
import sys
from datetime import datetime, timedelta, timezone

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from moonrtx_amd import ephemeris as E                                      # noqa: E402
from moonrtx_amd import traverse as tv                                      # noqa: E402
from moonrtx_amd.renderer import DeviceBuffer, MoonRT, synth_ldem, dem_from_ldem    # noqa: E402
from moonrtx_amd.scene import named_scene                                   # noqa: E402

DEM_H, DEM_W = 23040, 46080
SLOPE_DEG = 15.0
N_EPOCHS, TPE, TPC = 720, 3600, 1.0         # hourly epochs of 1 s ticks; 1 m of effort per second


def night_table(rows, cols, width, speed):
    """A device table rows x cols x W64: a dark band of `width` columns that moves `speed` columns per epoch (every row alike)."""
    e = np.arange(N_EPOCHS)
    j0 = np.floor(speed * e).astype(np.int64) % (cols + width) - width
    j = np.arange(cols)
    dark = (j[:, None] >= j0[None, :]) & (j[:, None] < j0[None, :] + width)
    row = tv.pack_mask(~dark)                                               # (cols, W64)
    buf = DeviceBuffer(rows * row.nbytes)
    block = np.ascontiguousarray(np.broadcast_to(row, (64,) + row.shape))
    for a in range(0, rows, 64):
        buf.upload(block[:min(64, rows - a)], a * row.nbytes)
    return buf


def ones_table(rows, cols):
    W64 = tv.mask_words(N_EPOCHS)
    buf = DeviceBuffer(rows * cols * W64 * 8)
    block = np.full((64, cols, W64), ~np.uint64(0), np.uint64)
    for a in range(0, rows, 64):
        buf.upload(block[:min(64, rows - a)], a * cols * W64 * 8)
    return buf


def best_of(fn, repeats):
    fn()                                                                    # warm-up
    best = None
    for _ in range(repeats):
        st, extra = fn()
        if best is None or st["kernel_ms"] < best["kernel_ms"]:
            best = dict(st, **extra)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-mask", action="store_true", help="skip the horizon_mask rows")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "timed_traverse_bench.json"))
    a = ap.parse_args()
    src = synth_ldem(DEM_H, DEM_W)
    dem, scale = dem_from_ldem(src, DEM_H, DEM_W, 1)
    src.free()
    rt = MoonRT(16, 16)
    rt.bind_dem(dem, DEM_H, DEM_W)
    rt.apply_scene(named_scene("S1", 16, 16))
    rt.set_params(flags=0)
    rm = 1737400.0 * scale
    res = {"dem": [DEM_H, DEM_W], "max_slope_deg": SLOPE_DEG, "n_epochs": N_EPOCHS, "ticks_per_epoch": TPE, "ticks_per_cost": TPC,
           "repeats": a.repeats, "cases": {}}
    windows = {"mid-latitude 2048 x 2048": ((10000, 21000, 2048, 2048), [(1024, 1024)], (256, 8.0)),
               "south-polar cap 512 x 3840, stride 12, wrapped": ((DEM_H - 1 - 511 * 12, 0, 512, 3840, 12, 1), [(500, 100)], (480, 16.0))}
    for name, (w, s, (width, speed)) in windows.items():
        nodes = np.array(s, np.int32)
        rows, cols = w[2], w[3]

        def plain():
            st = {}
            f = rt.traverse(w, nodes=nodes, max_slope_deg=SLOPE_DEG, radius_m=rm, stats=st, heights=False)
            return st, dict(reached=float(np.isfinite(f.cost).mean()))

        def timed(avail):
            def go():
                st = {}
                f = rt.traverse_timed(w, nodes=nodes, avail=avail, n_epochs=None if avail is None else N_EPOCHS,
                                      ticks_per_epoch=TPE, ticks_per_cost=TPC, max_slope_deg=SLOPE_DEG, radius_m=rm, stats=st)
                reach = f.arrival != tv.NEVER
                return st, dict(reached=float(reach.mean()), last_arrival_h=float(f.arrival[reach].max()) / 3600.0,
                                no_pred=int((f.pred == 254).sum()))
            return go
        out = res["cases"][name] = {}
        out["mrtx_traverse"] = best_of(plain, a.repeats)
        out["timed, no table"] = best_of(timed(None), a.repeats)
        for label, make in (("timed, all ones", lambda: ones_table(rows, cols)),
                            ("timed, moving night", lambda: night_table(rows, cols, width, speed))):
            buf = make()
            out[label] = best_of(timed(buf), a.repeats)
            buf.free()
        for k, v in out.items():
            print(name, k, json.dumps(v), flush=True)
    if not a.no_mask:
        la, lo = MoonRT.grid_nodes(lat=(-84.0, -90.0), lon=(-180.0, 180.0), shape=(256, 256))
        LA, LO = (x.ravel() for x in np.meshgrid(la, lo, indexing="ij"))
        t0 = datetime(2025, 1, 1, tzinfo=timezone.utc)
        ea, eb = E.sun_earth_epochs([t0 + timedelta(hours=k) for k in range(8760)], E.Observer(52.2, 21.0, 0.0))
        hz = DeviceBuffer(LA.size * 64 * 4)
        rt.horizon(LA, LO, n_az=64, n_bis=10, out=hz)
        out = DeviceBuffer(LA.size * tv.mask_words(8760) * 8)

        def mask():
            st = {}
            rt.horizon_mask(LA, LO, hz, ea, eb, min_a=0.5, min_b=0.5, n_az=64, out=out, stats=st, chunk_bytes=1 << 40)
            return st, {}

        def windows_():
            st = {}
            rt.horizon_windows(LA, LO, hz, ea, eb, min_a=0.5, min_b=0.5, n_az=64, stats=st, chunk_bytes=1 << 40)
            return st, {}
        res["horizon_mask 65536 x 8760"] = {"mrtx_horizon_mask": best_of(mask, a.repeats),
                                            "mrtx_horizon_windows": best_of(windows_, a.repeats)}
        print(json.dumps(res["horizon_mask 65536 x 8760"]), flush=True)
        hz.free()
        out.free()
    rt.close()
    dem.free()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"timed_traverse_bench": a.out}))


if __name__ == "__main__":
    main()
