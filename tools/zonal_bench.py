"""Zonal statistics and outline timings -> profiles/zonal_bench.json.

Per window (4096 x 4096 and 16384 x 16384, wrapped, 4-connected) and region set of tools/regions_bench.py -- the full set, a
random mask at the 4-connected percolation threshold 0.59, and the slope of a synthetic DEM under a footprint thresholded at
--max-slope degrees -- the kernel ms of mrtx_regions_zonal with 1 and with 4 channels, with 4 channels and a 64-bin histogram,
and of mrtx_regions_shape, every table on the device, each with the in-wave run reduction and with one set of atomics per node
(MOONRT_REGIONS_ZONAL=plain); the records of the two are compared.  The field is the relief table of the window (slope,
roughness and their companions, float4); the 1-channel field is the first quarter of the same memory read as one channel.
For context only: the numpy restatement of the 1-channel statistics on the host (np.add.at, np.minimum.at, np.maximum.at) over
the first window's random set."""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from moonrtx_amd import _lib                                                       # noqa: E402
from moonrtx_amd import regions as rg                                              # noqa: E402
from moonrtx_amd.renderer import DeviceBuffer, MoonRT, synth_ldem, dem_from_ldem   # noqa: E402
from regions_bench import DEM_H, DEM_W, label, random_mask                         # noqa: E402

SCALE = 1024.0


def zonal(rt, n, labels, k, field, n_ch, bins, mode, repeats):
    """Best kernel ms of `repeats` zonal calls in `mode` (runs or plain); (ms, launches, records, histogram or None)."""
    os.environ["MOONRT_REGIONS_ZONAL"] = mode
    z = _lib.MrtxZonalSpec(n, n, 1, n_ch, SCALE, 0, bins, 0.0, bins / 0.5 if bins else 1.0, 0)
    out = DeviceBuffer(max(56 * k * n_ch, 56))
    hist = DeviceBuffer(8 * k * (bins + 2)) if bins and k else None
    best, st = None, _lib.MrtxStats()
    try:
        for _ in range(repeats):
            rt._check(rt._lib.mrtx_regions_zonal(rt._ctx, C.byref(z), labels.ptr, None, k, field.ptr, None, None, out.ptr, None,
                                                 hist.ptr if hist else None, None, C.byref(st)), "mrtx_regions_zonal")
            best = st.kernel_ms if best is None else min(best, st.kernel_ms)
        return best, st.launches, out.download(rg.ZONAL_DTYPE, (k, n_ch)), hist.download(np.uint64, (k, bins + 2)) if hist else None
    finally:
        out.free()
        if hist:
            hist.free()
        del os.environ["MOONRT_REGIONS_ZONAL"]


def shape(rt, n, labels, k, mode, repeats):
    os.environ["MOONRT_REGIONS_ZONAL"] = mode
    out = DeviceBuffer(max(32 * k, 32))
    best, st = None, _lib.MrtxStats()
    try:
        for _ in range(repeats):
            rt._check(rt._lib.mrtx_regions_shape(rt._ctx, n, n, 1, 4, labels.ptr, None, k, None, None, out.ptr, None, C.byref(st)),
                      "mrtx_regions_shape")
            best = st.kernel_ms if best is None else min(best, st.kernel_ms)
        return best, st.launches, out.download(rg.SHAPE_DTYPE, (k,))
    finally:
        out.free()
        del os.environ["MOONRT_REGIONS_ZONAL"]


def host_zonal(labels, x, k):
    """The 1-channel statistics with numpy on the host: seconds, and (count, sum, min, max) to compare."""
    t0 = time.perf_counter()
    lab, x = labels.reshape(-1), x.reshape(-1)
    ok = (lab >= 0) & ~np.isnan(x)
    lab, x = lab[ok], x[ok]
    p = x.astype(np.float64) * SCALE
    q = np.where(np.abs(p) >= 2.0 ** 31, np.sign(p) * 2.0 ** 31, np.rint(p)).astype(np.int64)
    count = np.bincount(lab, minlength=k)
    total = np.zeros(k, np.int64)
    np.add.at(total, lab, q)
    lo, hi = np.full(k, np.inf, np.float32), np.full(k, -np.inf, np.float32)
    np.minimum.at(lo, lab, x)
    np.maximum.at(hi, lab, x)
    return time.perf_counter() - t0, (count, total, lo, hi)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--plain-repeats", type=int, default=1, help="the yardstick takes up to minutes per call")
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 16384])
    ap.add_argument("--max-slope", type=float, default=8.0, help="degrees: the relief set is slope <= this")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zonal_bench.json"))
    a = ap.parse_args()
    src = synth_ldem(DEM_H, DEM_W)
    dem, scale = dem_from_ldem(src, DEM_H, DEM_W, 1)
    src.free()
    rt = MoonRT(16, 16)
    rt.bind_dem(dem, DEM_H, DEM_W)
    rt.set_params(flags=0)
    res = {"dem": [DEM_H, DEM_W], "connectivity": 4, "wrap": 1, "max_slope_deg": a.max_slope, "scale": SCALE, "cases": []}
    for n in a.sizes:
        N = n * n
        labels = DeviceBuffer(4 * N)
        relief = DeviceBuffer(16 * N)
        t = _lib.MrtxRelief(3000, 10000, n, n, 1, 2, 2, 0, 1737400.0 * scale)
        st = _lib.MrtxStats()
        rt._check(rt._lib.mrtx_relief(rt._ctx, C.byref(t), relief.ptr, None, C.byref(st)), "mrtx_relief")
        rnd = random_mask(n, 0.59)
        buf = DeviceBuffer(N)
        sets = {"full": np.ones((n, n), np.uint8), "random 0.59": rnd, f"relief, slope <= {a.max_slope:g} deg": None}
        for name, m in sets.items():
            if m is not None:
                buf.upload(m)
                r = _lib.MrtxRegions(n, n, 1, 4, 1, 0, -math.inf, math.inf, 0)
                _, _, k = label(rt, r, None, buf.ptr, labels, 1)
            else:
                r = _lib.MrtxRegions(n, n, 1, 4, 4, 0, -math.inf, math.tan(math.radians(a.max_slope)), 0)
                _, _, k = label(rt, r, relief.ptr, None, labels, 1)
            row = dict(window=[n, n], set=name, regions=k)
            for key, n_ch, bins in (("zonal_1ch", 1, 0), ("zonal_4ch", 4, 0), ("zonal_4ch_hist64", 4, 64)):
                if k * (bins + 2) > 1 << 28:        # more columns than a histogram may hold
                    row.update({f"{key}_runs_ms": None, f"{key}_plain_ms": None})
                    continue
                ms, launches, zr, hr = zonal(rt, n, labels, k, relief, n_ch, bins, "runs", a.repeats)
                pms, _, zp, hp = zonal(rt, n, labels, k, relief, n_ch, bins, "plain", a.plain_repeats)
                row.update({f"{key}_runs_ms": ms, f"{key}_plain_ms": pms, f"{key}_launches": launches,
                            f"{key}_same": bool(zr.tobytes() == zp.tobytes() and (hr is None or np.array_equal(hr, hp)))})
                if key == "zonal_1ch":
                    row["counted"] = int(zr["count"].sum())
                print(json.dumps({key: [ms, pms]}), flush=True)
            ms, launches, sr = shape(rt, n, labels, k, "runs", a.repeats)
            pms, _, sp = shape(rt, n, labels, k, "plain", a.plain_repeats)
            row.update(shape_runs_ms=ms, shape_plain_ms=pms, shape_launches=launches, shape_same=bool(sr.tobytes() == sp.tobytes()))
            res["cases"].append(row)
            print(json.dumps(row), flush=True)
        if not a.no_host and n == a.sizes[0]:
            buf.upload(rnd)
            r = _lib.MrtxRegions(n, n, 1, 4, 1, 0, -math.inf, math.inf, 0)
            _, _, k = label(rt, r, None, buf.ptr, labels, 1)
            ms, _, zr, _ = zonal(rt, n, labels, k, relief, 1, 0, "runs", a.repeats)
            t0 = time.perf_counter()
            lab_h, x_h = labels.download(np.int32, (n, n)), relief.download(np.float32, (n, n))
            down_s = time.perf_counter() - t0
            host_s, (count, total, lo, hi) = host_zonal(lab_h, x_h, k)
            zr = zr[:, 0]
            full = zr["count"] > 0
            same = bool(np.array_equal(count, zr["count"]) and np.array_equal(total, zr["sum"]) and
                        np.array_equal(lo[full], zr["min"][full]) and np.array_equal(hi[full], zr["max"][full]))
            res["host"] = dict(window=[n, n], set="random 0.59", regions=k, zonal_1ch_runs_ms=ms, download_s=down_s,
                               numpy_s=host_s, same_records=same)
            print("host", json.dumps(res["host"]), flush=True)
        for b in (labels, relief, buf):
            b.free()
    rt.close()
    dem.free()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"zonal_bench": a.out}))


if __name__ == "__main__":
    main()
