#!/usr/bin/env python
"""Times the region outlines (profiles/outlines.md): kernel_ms of the count call and of the fill call
of mrtx_regions_outline under MOONRT_REGIONS_OUTLINE = contract and jump on n x n lattices, from a label table on the device,
for three inputs: a random mask at 0.59 (the 4-connected percolation threshold), a smooth-blob mask (a thresholded low-pass of noise, which is what real shadow maps look
like) and one spiral whose single ring is about half the lattice long.  The masks are labelled by MoonRT.regions first; after
--warmup calls the median of --runs calls, per variant; the two variants must give the same bytes.  One JSON line per size and
input.

  python tools/outline_bench.py --sizes 1024 4096 --runs 7 --out profiles/outlines_bench.json"""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
from moonrtx_amd.renderer import DeviceBuffer, MoonRT

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096])
ap.add_argument("--runs", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--all-vertices", action="store_true")
ap.add_argument("--out")
a = ap.parse_args()


def random_mask(n, seed=1):
    return (np.random.default_rng(seed).random((n, n)) < 0.59).astype(np.uint8)


def blob_mask(n, seed=2, sigma=12.0):
    """Gaussian low-pass (sigma nodes, periodic) of white noise, thresholded at its median."""
    x = np.random.default_rng(seed).standard_normal((n, n)).astype(np.float32)
    k = np.fft.fftfreq(n).astype(np.float32)
    g = np.exp(-2.0 * (np.pi * sigma) ** 2 * k * k).astype(np.float32)
    y = np.fft.irfft2(np.fft.rfft2(x) * g[:, None] * g[None, :n // 2 + 1], s=(n, n))
    return (y > np.median(y)).astype(np.uint8)


def spiral_mask(n):
    """A one-node-wide rectangular spiral from (0, 0) inwards, its arms two nodes apart: one region, one ring."""
    m = np.zeros((n, n), np.uint8)
    top, left, bottom, right = 0, 0, n - 1, n - 1
    m[0, 0:n] = 1
    while True:
        if bottom - top < 2: break
        m[top:bottom + 1, right] = 1            # down the right side
        left_end = left
        if right - left_end < 2: break
        m[bottom, left_end:right + 1] = 1       # left along the bottom
        top += 2
        if bottom - top < 2: break
        m[top:bottom + 1, left] = 1             # up the left side
        right -= 2
        if right - left < 2: break
        m[top, left:right + 1] = 1              # right along the next arm
        left += 2
        bottom -= 2
    return m


rt = MoonRT(16, 16, device=0)
lines = []
for n in a.sizes:
    for name, make in (("random_0.59", random_mask), ("blobs", blob_mask), ("spiral", spiral_mask)):
        region_map = rt.regions(mask=make(n))
        buf = DeviceBuffer(4 * n * n)
        buf.upload(region_map.labels)
        rec, got = {}, {}
        for variant in ("contract", "jump"):
            os.environ["MOONRT_REGIONS_OUTLINE"] = variant
            count_ms, fill_ms = [], []
            for r in range(a.warmup + a.runs):
                st = {}
                ol = rt.region_outlines(buf, region_map.n, corners=not a.all_vertices, shape=(n, n), stats=st)
                if r >= a.warmup:
                    count_ms.append(st["count_ms"])
                    fill_ms.append(st["fill_ms"])
            got[variant] = ol
            rec[variant] = {"launches": st["launches"], "runs": len(fill_ms), "count_ms": statistics.median(count_ms),
                            "fill_ms": statistics.median(fill_ms), "fill_min_ms": min(fill_ms), "fill_max_ms": max(fill_ms)}
        buf.free()
        assert got["contract"].rings.tobytes() == got["jump"].rings.tobytes()
        assert got["contract"].vertices.tobytes() == got["jump"].vertices.tobytes()
        rec = dict({"n": n, "input": name, "regions": region_map.n, "rings": len(ol), "vertices": int(ol.vertices.shape[0]),
                    "sides": int(ol.rings["n_sides"].astype(np.int64).sum()), "longest_ring": int(ol.rings["n_sides"].max())}, **rec)
        lines.append(rec)
        print(json.dumps(rec), flush=True)
rt.close()
if a.out:
    with open(a.out, "w") as f:
        json.dump(lines, f, indent=1)
        f.write("\n")
