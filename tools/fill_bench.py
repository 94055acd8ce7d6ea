#!/usr/bin/env python
"""Times the depression fill (profiles/fill.md): kernel_ms, launches and visits of mrtx_fill under
MOONRT_FILL = tiles and sweep on n x n lattices, from a height table on the device, for two inputs: a window of the synthetic
LOLA-like DEM (mrtx_synth_ldem) in centimetres, and one flat-floored basin inside a rim with a single notch, the worst case for
propagation.  --runs runs per variant after --warmup, all reported; the two variants must give the same bytes.  Node visits
are what a variant touches: tile visits x 32 x 32 for tiles, launches x n x n for the sweep.  --scipy adds the wall time of a
CPU reference (reconstruction by erosion with scipy.ndimage, sizes up to 1024 only) when scipy is importable.  After the fills
the depressions are labelled by MoonRT.regions and mrtx_fill_basins is timed on those labels.  One JSON line per size and input.

  python tools/fill_bench.py --sizes 1024 4096 --runs 3 --out profiles/fill_bench.json"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
from moonrtx_amd import basins as bs
from moonrtx_amd.renderer import DeviceBuffer, MoonRT, dem_from_ldem, synth_ldem

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096])
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--dem-size", type=int, nargs=2, default=(8192, 16384))
ap.add_argument("--connectivity", type=int, default=8, choices=(4, 8))
ap.add_argument("--variants", nargs="+", default=["tiles", "sweep"], choices=("tiles", "sweep"))
ap.add_argument("--scipy", action="store_true")
ap.add_argument("--out")
a = ap.parse_args()


def flat_basin(n):
    z = np.zeros((n, n), np.int32)
    z[0, :] = z[-1, :] = z[:, 0] = z[:, -1] = 100
    z[n // 2 + 3, n - 1] = 7
    return z


def scipy_fill(z, conn):
    """Reconstruction by erosion: from +inf inside and z on the border, W = max(z, min over the neighbourhood of W) until
    nothing changes."""
    from scipy import ndimage
    fp = np.ones((3, 3), bool) if conn == 8 else ndimage.generate_binary_structure(2, 1)
    w = np.full(z.shape, np.iinfo(np.int32).max, np.int32)
    w[0, :], w[-1, :], w[:, 0], w[:, -1] = z[0, :], z[-1, :], z[:, 0], z[:, -1]
    while True:
        new = np.maximum(z, ndimage.minimum_filter(w, footprint=fp, mode="nearest"))
        np.minimum(new, w, out=new)
        if (new == w).all():
            return w
        w = new


dh, dw = a.dem_size
src = synth_ldem(dh, dw, device=0)
dem, scale = dem_from_ldem(src, dh, dw, 1, device=0)
src.free()
rt = MoonRT(16, 16, device=0)
rt.bind_dem(dem, dh, dw)
lines = []
for n in a.sizes:
    terrain = bs.quantise_heights((rt.traverse_heights((dh // 4, dw // 4, n, n)).astype(np.float64) - 1.0) * 1737400.0 * float(scale), 0.01)
    for name, z in (("synth_ldem", terrain), ("flat_basin", flat_basin(n))):
        buf = DeviceBuffer(4 * n * n)
        buf.upload(z)
        rec, got = {"n": n, "input": name}, {}
        for variant in a.variants:
            os.environ["MOONRT_FILL"] = variant
            runs = []
            for r in range(a.warmup + a.runs):
                st = {}
                m = rt.fill_depressions(buf, connectivity=a.connectivity, shape=(n, n), stats=st)
                if r >= a.warmup:
                    runs.append({"kernel_ms": st["kernel_ms"], "launches": st["launches"], "visits": st["visits"],
                                 "node_visits": st["visits"] * 32 * 32 if variant == "tiles" else (st["launches"] - 1) * n * n})
            got[variant] = m.fill
            rec[variant] = runs
        buf.free()
        if len(got) == 2:
            assert got["tiles"].tobytes() == got["sweep"].tobytes()
            rec["visits_saved"] = 1.0 - min(r["node_visits"] for r in rec["tiles"]) / max(1, min(r["node_visits"] for r in rec["sweep"]))
        rec["in_depression"] = float((m.depth() > 0).mean())
        # the catalogue of the depressions: the labels of MoonRT.regions, then mrtx_fill_basins from host tables
        regions = rt.regions(mask=m.mask(), connectivity=a.connectivity)
        basins_ms = []
        for r in range(a.warmup + a.runs):
            st = {}
            table = rt.basins(regions.labels, regions.n, m, stats=st)
            if r >= a.warmup:
                basins_ms.append(st["kernel_ms"])
        rec["basins"] = {"regions": regions.n, "largest": int(table["count"].max()) if regions.n else 0, "kernel_ms": basins_ms}
        if a.scipy and n <= 1024:
            try:
                t0 = time.time()
                ref = scipy_fill(z, a.connectivity)
                rec["scipy_s"] = time.time() - t0
                assert (ref == m.fill).all()
            except ImportError:
                rec["scipy_s"] = None
        lines.append(rec)
        print(json.dumps(rec), flush=True)
rt.close()
dem.free()
os.environ.pop("MOONRT_FILL", None)
if a.out:
    with open(a.out, "w") as f:
        json.dump(lines, f, indent=1)
        f.write("\n")
