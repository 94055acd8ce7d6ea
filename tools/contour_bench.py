#!/usr/bin/env python
"""Times the contour lines (profiles/contours.md): kernel_ms of the count call and of the fill call of
mrtx_contours on n x n lattices, heights and tables on the device, for three inputs (smooth blobs: a Gaussian low-pass of
noise, which is what terrain and temperature maps look like; white noise; one spiral whose single line is about half the
lattice long) at 1 and at 16 levels.  Beside each, for scale only, the fill call of mrtx_regions_outline (every side a vertex)
on the mask z >= c of the same lattice at the one level, and the ratio of the two fill calls.  After --warmup calls the median
of --runs calls.  One JSON line per size and input.

  python tools/contour_bench.py --sizes 1024 4096 --runs 7 --out profiles/contours_bench.json"""
import argparse, ctypes as C, json, os, statistics, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
from moonrtx_amd import _lib
from moonrtx_amd import contours as ct
from moonrtx_amd.renderer import DeviceBuffer, MoonRT

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096])
ap.add_argument("--runs", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out")
a = ap.parse_args()


def blob_heights(n, seed=2, sigma=12.0):
    """Gaussian low-pass (sigma nodes, periodic) of white noise, scaled so that its extremes are near +-1000."""
    x = np.random.default_rng(seed).standard_normal((n, n)).astype(np.float32)
    k = np.fft.fftfreq(n).astype(np.float32)
    g = np.exp(-2.0 * (np.pi * sigma) ** 2 * k * k).astype(np.float32)
    y = np.fft.irfft2(np.fft.rfft2(x) * g[:, None] * g[None, :n // 2 + 1], s=(n, n))
    return np.rint(y * (1000.0 / np.abs(y).max())).astype(np.int32)


def noise_heights(n, seed=1):
    return np.random.default_rng(seed).integers(-1000, 1001, (n, n)).astype(np.int32)


def spiral_heights(n):
    """A one-node-wide rectangular spiral from (0, 0) inwards at +500 over -500, its arms two nodes apart."""
    m = np.zeros((n, n), np.uint8)
    top, left, bottom, right = 0, 0, n - 1, n - 1
    m[0, 0:n] = 1
    while True:
        if bottom - top < 2: break
        m[top:bottom + 1, right] = 1            # down the right side
        if right - left < 2: break
        m[bottom, left:right + 1] = 1           # left along the bottom
        top += 2
        if bottom - top < 2: break
        m[top:bottom + 1, left] = 1             # up the left side
        right -= 2
        if right - left < 2: break
        m[top, left:right + 1] = 1              # right along the next arm
        left += 2
        bottom -= 2
    return np.where(m != 0, 500, -500).astype(np.int32)


def check(rt, rc, what):
    if rc != 0:
        raise RuntimeError(f"{what}: {rt._lib.mrtx_last_error(rt._ctx).decode()}")


def time_contours(rt, zb, n, levels):
    """(count_ms, fill_ms, launches of the fill call, lines, vertices): the medians over the runs."""
    lv = np.ascontiguousarray(levels, np.int32)
    k = _lib.MrtxContours(n, n, 0, int(lv.size), 0)
    nl, nv, st = C.c_uint64(0), C.c_uint64(0), _lib.MrtxStats()
    check(rt, rt._lib.mrtx_contours(rt._ctx, C.byref(k), zb.ptr, None, lv.ctypes.data, None, None, 0, None, None, 0, C.byref(nl), C.byref(nv),
                                    C.byref(st)), "mrtx_contours")
    L, V = int(nl.value), int(nv.value)
    lb, vb = DeviceBuffer(max(32 * L, 32)), DeviceBuffer(max(4 * V, 4))
    count_ms, fill_ms = [], []
    try:
        for r in range(a.warmup + a.runs):
            check(rt, rt._lib.mrtx_contours(rt._ctx, C.byref(k), zb.ptr, None, lv.ctypes.data, None, None, 0, None, None, 0, C.byref(nl),
                                            C.byref(nv), C.byref(st)), "mrtx_contours")
            t_count = st.kernel_ms
            check(rt, rt._lib.mrtx_contours(rt._ctx, C.byref(k), zb.ptr, None, lv.ctypes.data, lb.ptr, None, L, vb.ptr, None, V, C.byref(nl),
                                            C.byref(nv), C.byref(st)), "mrtx_contours")
            if r >= a.warmup:
                count_ms.append(t_count)
                fill_ms.append(st.kernel_ms)
        longest = int(lb.download(_lib.CONTOUR_LINE_DTYPE, (L,))["n_vertices"].max()) if L else 0
    finally:
        lb.free()
        vb.free()
    return {"levels": int(lv.size), "lines": L, "vertices": V, "longest_line": longest, "launches": int(st.launches), "runs": len(fill_ms),
            "count_ms": statistics.median(count_ms), "fill_ms": statistics.median(fill_ms), "fill_min_ms": min(fill_ms),
            "fill_max_ms": max(fill_ms)}


def time_outline(rt, z, n, c):
    """The fill call of mrtx_regions_outline on the mask z >= c as one label, every side a vertex."""
    labels = np.where(z >= c, 0, -1).astype(np.int32)
    buf = DeviceBuffer(4 * n * n)
    buf.upload(labels)
    o = _lib.MrtxOutline(n, n, 0, 4, _lib.OUTLINE_ALL, 0)
    nr, nv, st = C.c_uint64(0), C.c_uint64(0), _lib.MrtxStats()
    check(rt, rt._lib.mrtx_regions_outline(rt._ctx, C.byref(o), buf.ptr, None, 1, None, None, None, 0, None, None, 0, C.byref(nr), C.byref(nv),
                                           C.byref(st)), "mrtx_regions_outline")
    R, V = int(nr.value), int(nv.value)
    rb, vb = DeviceBuffer(max(48 * R, 48)), DeviceBuffer(max(8 * V, 8))
    fill_ms = []
    try:
        for r in range(a.warmup + a.runs):
            check(rt, rt._lib.mrtx_regions_outline(rt._ctx, C.byref(o), buf.ptr, None, 1, None, rb.ptr, None, R, vb.ptr, None, V, C.byref(nr),
                                                   C.byref(nv), C.byref(st)), "mrtx_regions_outline")
            if r >= a.warmup:
                fill_ms.append(st.kernel_ms)
    finally:
        rb.free()
        vb.free()
        buf.free()
    return {"rings": R, "sides": V, "launches": int(st.launches), "fill_ms": statistics.median(fill_ms)}


rt = MoonRT(16, 16, device=0)
records = []
for n in a.sizes:
    for name, make in (("blobs", blob_heights), ("noise", noise_heights), ("spiral", spiral_heights)):
        z = make(n)
        zb = DeviceBuffer(4 * n * n)
        zb.upload(z)
        try:
            one = time_contours(rt, zb, n, [0])
            many = time_contours(rt, zb, n, ct.levels_for(-800, 800, 100))
        finally:
            zb.free()
        outline = time_outline(rt, z, n, 0)
        rec = {"n": n, "input": name, "contours_1": one, "contours_16": many, "outline": outline,
               "fill_ratio_1_level": one["fill_ms"] / outline["fill_ms"]}
        records.append(rec)
        print(json.dumps(rec), flush=True)
rt.close()
if a.out:
    with open(a.out, "w") as f:
        json.dump(records, f, indent=1)
        f.write("\n")
