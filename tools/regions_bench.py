"""Region labelling and catalogue timings -> profiles/regions_bench.json.

Per window (4096 x 4096 and 16384 x 16384, wrapped, 4-connected) and set -- the full set, a random mask at the 4-connected
percolation threshold 0.59, and the slope of a synthetic DEM under a footprint thresholded at --max-slope degrees -- the
kernel ms of the label call and of the catalogue call, apart, every table on the device.  The catalogue is timed twice on
every set: with the in-wave run reduction and with one set of atomics per node (MOONRT_REGIONS_CATALOGUE=plain); the
records are compared.  For context only: scipy.ndimage.label on the host over the 4096 x 4096 random mask, unwrapped, its
labels compared with the device's node for node."""
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

DEM_H, DEM_W = 23040, 46080


def random_mask(n, density, seed=59):
    rng = np.random.default_rng(seed)
    out = np.empty((n, n), np.uint8)
    for a in range(0, n, 1024):
        out[a:a + 1024] = rng.random((min(1024, n - a), n), np.float32) < density
    return out


def label(rt, r, field, mask, labels, repeats):
    """Best kernel ms of `repeats` label calls on device tables; (ms, launches, K)."""
    best, k, st = None, C.c_uint32(0), _lib.MrtxStats()
    for _ in range(repeats):
        rt._check(rt._lib.mrtx_regions_label(rt._ctx, C.byref(r), field, None, mask, None, labels.ptr, None, C.byref(k),
                                             C.byref(st)), "mrtx_regions_label")
        best = st.kernel_ms if best is None else min(best, st.kernel_ms)
    return best, st.launches, k.value


def catalogue(rt, r, labels, k, mode, repeats):
    """Best kernel ms of `repeats` catalogue calls in `mode` (runs or plain), and the records."""
    os.environ["MOONRT_REGIONS_CATALOGUE"] = mode
    out = DeviceBuffer(max(56 * k, 56))
    best, st = None, _lib.MrtxStats()
    try:
        for _ in range(repeats):
            rt._check(rt._lib.mrtx_regions_stats(rt._ctx, r.rows, r.cols, r.wrap, labels.ptr, None, k, None, out.ptr, None,
                                                 C.byref(st)), "mrtx_regions_stats")
            best = st.kernel_ms if best is None else min(best, st.kernel_ms)
        return best, out.download(rg.REGION_DTYPE, (k,))
    finally:
        out.free()
        del os.environ["MOONRT_REGIONS_CATALOGUE"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 16384])
    ap.add_argument("--max-slope", type=float, default=8.0, help="degrees: the relief set is slope <= this")
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regions_bench.json"))
    a = ap.parse_args()
    src = synth_ldem(DEM_H, DEM_W)
    dem, scale = dem_from_ldem(src, DEM_H, DEM_W, 1)
    src.free()
    rt = MoonRT(16, 16)
    rt.bind_dem(dem, DEM_H, DEM_W)
    rt.set_params(flags=0)
    res = {"dem": [DEM_H, DEM_W], "connectivity": 4, "wrap": 1, "max_slope_deg": a.max_slope, "cases": []}
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
                field, mask = None, buf.ptr
            else:
                r = _lib.MrtxRegions(n, n, 1, 4, 4, 0, -math.inf, math.tan(math.radians(a.max_slope)), 0)
                field, mask = relief.ptr, None
            ms, launches, k = label(rt, r, field, mask, labels, a.repeats)
            runs_ms, t_runs = catalogue(rt, r, labels, k, "runs", a.repeats)
            plain_ms, t_plain = catalogue(rt, r, labels, k, "plain", a.repeats)
            row = dict(window=[n, n], set=name, regions=k, in_set=int(t_runs["count"].sum()), label_ms=ms,
                       label_launches=launches, catalogue_runs_ms=runs_ms, catalogue_plain_ms=plain_ms,
                       largest=int(t_runs["count"].max()) if k else 0, same_records=bool(np.array_equal(t_runs, t_plain)))
            res["cases"].append(row)
            print(json.dumps(row), flush=True)
        if not a.no_scipy and n == a.sizes[0]:
            from scipy import ndimage
            buf.upload(rnd)
            r = _lib.MrtxRegions(n, n, 0, 4, 1, 0, -math.inf, math.inf, 0)
            ms, _, k = label(rt, r, None, buf.ptr, labels, a.repeats)
            t0 = time.perf_counter()
            ref, kk = ndimage.label(rnd)
            host_s = time.perf_counter() - t0
            same = bool(kk == k and np.array_equal(ref.astype(np.int32) - 1, labels.download(np.int32, (n, n))))
            res["scipy"] = dict(window=[n, n], set="random 0.59, unwrapped", regions=k, label_ms=ms, scipy_label_s=host_s,
                                same_labels=same)
            print("scipy", json.dumps(res["scipy"]), flush=True)
        for b in (labels, relief, buf):
            b.free()
    rt.close()
    dem.free()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"regions_bench": a.out}))


if __name__ == "__main__":
    main()
