#!/usr/bin/env python
"""Times the polygon rasterisation: kernel_ms of mrtx_rasterise under MOONRT_RASTER = bins and brute
on the polar window 21515 0 127 3840 12 1, from tables on the device, and the wall time of the plain model of
tests/raster_model.py on the host.  The polygons are the outlines of a thresholded map: a low-pass of noise, which is what real
shadow maps look like, labelled by MoonRT.regions and traced by MoonRT.region_outlines.  After --warmup calls the median of
--runs calls (brute: --brute-runs, it is the slow yardstick); the two variants and the model must give back the label table.
One JSON line.

  python tools/raster_bench.py --runs 7 --out profiles/raster_bench.json"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np
from moonrtx_amd.renderer import DeviceBuffer, MoonRT

ap = argparse.ArgumentParser()
ap.add_argument("--window", type=int, nargs=6, default=[21515, 0, 127, 3840, 12, 1], metavar="N")
ap.add_argument("--sigma", type=float, default=6.0, help="the low-pass of the map, in nodes")
ap.add_argument("--all-vertices", action="store_true")
ap.add_argument("--runs", type=int, default=7)
ap.add_argument("--brute-runs", type=int, default=1)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--no-model", action="store_true")
ap.add_argument("--out")
a = ap.parse_args()
rows, cols, wrap = a.window[2], a.window[3], bool(a.window[5])


def blob_mask(rows, cols, sigma, seed=2):
    """Gaussian low-pass (sigma nodes, periodic) of white noise, thresholded at its median."""
    x = np.random.default_rng(seed).standard_normal((rows, cols)).astype(np.float32)
    gy = np.exp(-2.0 * (np.pi * sigma) ** 2 * np.fft.fftfreq(rows) ** 2).astype(np.float32)
    gx = np.exp(-2.0 * (np.pi * sigma) ** 2 * np.fft.rfftfreq(cols) ** 2).astype(np.float32)
    y = np.fft.irfft2(np.fft.rfft2(x) * gy[:, None] * gx[None, :], s=(rows, cols))
    return (y > np.median(y)).astype(np.uint8)


rt = MoonRT(16, 16, device=0)
region_map = rt.regions(mask=blob_mask(rows, cols, a.sigma), wrap=wrap)
pg = rt.region_outlines(region_map.labels, region_map.n, wrap=wrap, corners=not a.all_vertices).polygons(region_map.n)
rb, vb = DeviceBuffer(max(pg.rings.nbytes, 24)), DeviceBuffer(max(pg.vertices.nbytes, 8))
rb.upload(pg.rings)
vb.upload(pg.vertices)
tables = (rb, len(pg), vb, pg.vertices.shape[0], pg.n_polygons, 0)
rec = {"window": a.window, "regions": region_map.n, "rings": len(pg), "vertices": int(pg.vertices.shape[0])}
for variant, runs, warmup in (("bins", a.runs, a.warmup), ("brute", a.brute_runs, 0)):
    os.environ["MOONRT_RASTER"] = variant
    ms = []
    for r in range(warmup + runs):
        st = {}
        labels, cover = rt.rasterise(tables, (rows, cols), wrap, stats=st)
        if r >= warmup:
            ms.append(st["kernel_ms"])
    assert (labels == region_map.labels).all() and cover["count"].tolist() == region_map.table["count"].tolist(), variant
    rec["crossings"] = st["crossings"]
    rec[variant] = {"launches": st["launches"], "runs": len(ms), "kernel_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}
os.environ.pop("MOONRT_RASTER", None)
rb.free()
vb.free()
rt.close()
if not a.no_model:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import raster_model
    t0 = time.perf_counter()
    labels, cover, n = raster_model.raster(pg.rings, pg.vertices, pg.n_polygons, rows, cols, wrap, 0)
    rec["model_host_ms"] = (time.perf_counter() - t0) * 1e3
    assert (labels == region_map.labels).all() and n == rec["crossings"]
print(json.dumps(rec), flush=True)
if a.out:
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
