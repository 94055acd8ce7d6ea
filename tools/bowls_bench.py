#!/usr/bin/env python
"""Times the depression hierarchy and writes profiles/bowls.md: mrtx_bowls on the four inputs of
tools/fill_bench.py (n x n windows of the synthetic LOLA-like DEM in centimetres, and one flat-floored basin with a single notch,
n = 1024 and 4096), heights on the device, records and labels made on the device and downloaded.  --runs sized calls after
--warmup; per input the median and the spread (min .. max) of kernel_ms (the device phases), of the call's wall time and of
the share of the wall time that is not kernel_ms (the host's sort and union-find over the minima, staging and waits), the
launches, the merge rounds, the bowls, and the wall time of reading the records and labels back.  Beside them, for scale,
mrtx_fill (tiles) and the catalogue of its depressions (MoonRT.regions + mrtx_fill_basins), which this stage leaves as they were.
The model of the tests is too slow here, so each input asserts identity 1 against mrtx_fill and the root bowls' volumes against
the sum of mrtx_fill_basins' volumes.

  python tools/bowls_bench.py --sizes 1024 4096 --runs 3 --out profiles/bowls.md"""
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
ap.add_argument("--out")
a = ap.parse_args()


def flat_basin(n):
    z = np.zeros((n, n), np.int32)
    z[0, :] = z[-1, :] = z[:, 0] = z[:, -1] = 100
    z[n // 2 + 3, n - 1] = 7
    return z


def spread(v):
    return f"{float(np.median(v)):.2f} ({min(v):.2f} .. {max(v):.2f})"


dh, dw = a.dem_size
src = synth_ldem(dh, dw, device=0)
dem, scale = dem_from_ldem(src, dh, dw, 1, device=0)
src.free()
rt = MoonRT(16, 16, device=0)
rt.bind_dem(dem, dh, dw)
os.environ.pop("MOONRT_FILL", None)
lines = []
for n in a.sizes:
    terrain = bs.quantise_heights((rt.traverse_heights((dh // 4, dw // 4, n, n)).astype(np.float64) - 1.0) * 1737400.0 * float(scale), 0.01)
    for name, z in (("synth_ldem", terrain), ("flat_basin", flat_basin(n))):
        buf = DeviceBuffer(4 * n * n)
        buf.upload(z)
        rec = {"n": n, "input": name, "kernel_ms": [], "count_ms": [], "wall_ms": [], "host_share": [], "launches": [], "rounds": []}
        for r in range(a.warmup + a.runs):
            st = {}
            t0 = time.perf_counter()
            tree = rt.bowls(buf, connectivity=a.connectivity, shape=(n, n), stats=st)
            wall = (time.perf_counter() - t0) * 1e3
            if r >= a.warmup:
                rec["kernel_ms"].append(st["kernel_ms"] - st["count_ms"])      # the sized call alone
                rec["count_ms"].append(st["count_ms"])
                rec["wall_ms"].append(wall)
                rec["host_share"].append(1.0 - st["kernel_ms"] / wall)
                rec["launches"].append(st["launches"])
                rec["rounds"].append(st["rounds"])
        rec["bowls"], rec["roots"] = tree.n, len(tree.roots())
        lb = DeviceBuffer(4 * n * n)
        rb = DeviceBuffer(max(64 * tree.n, 64))
        t0 = time.perf_counter()
        lb.download(np.int32, (n, n))
        rb.download(bs.BOWL_DTYPE, (tree.n,))
        rec["readback_ms"] = (time.perf_counter() - t0) * 1e3
        lb.free()
        rb.free()
        # for scale: the fill and the catalogue of its depressions
        fill_ms, cat_ms = [], []
        for r in range(a.warmup + a.runs):
            st, st2 = {}, {}
            m = rt.fill_depressions(buf, connectivity=a.connectivity, shape=(n, n), stats=st)
            regions, table = m.catalogue(rt, stats=st2)
            if r >= a.warmup:
                fill_ms.append(st["kernel_ms"])
                cat_ms.append(st2["kernel_ms"])
        buf.free()
        rec["fill_ms"], rec["catalogue_ms"], rec["depressions"] = fill_ms, cat_ms, regions.n
        assert (tree.fill() == m.fill).all(), "identity 1"
        assert sum(int(v) for v in tree.records["volume"][tree.roots()]) % 2 ** 64 == sum(int(v) for v in table["volume"]) % 2 ** 64
        lines.append(rec)
        print(json.dumps(rec), flush=True)
rt.close()
dem.free()
if a.out:
    with open(a.out, "w") as f:
        f.write("# The depression hierarchy on one MI355X (tools/bowls_bench.py)\n\n")
        f.write(f"Median (min .. max) of {a.runs} runs after {a.warmup} warm-up, connectivity {a.connectivity}, heights on the device.  "
                "kernel_ms: the device phases of the sized call; count: those of the counting call before it; wall: both calls and the "
                "downloads, as MoonRT.bowls makes them; not kernel: the share of the wall time outside the device phases (the host's sort "
                "and union-find over the minima, staging, downloads).  fill and catalogue: mrtx_fill (tiles) and MoonRT.regions + "
                "mrtx_fill_basins on the same input, unchanged by this stage.  Every input passed identity 1 against mrtx_fill and the "
                "volume sum against mrtx_fill_basins.\n\n")
        f.write("| n | input | bowls | roots | rounds | launches | kernel_ms | count ms | wall ms | not kernel | readback ms | fill ms | catalogue ms |\n")
        f.write("|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in lines:
            f.write(f"| {r['n']} | {r['input']} | {r['bowls']} | {r['roots']} | {max(r['rounds'])} | {min(r['launches'])} .. {max(r['launches'])} | "
                    f"{spread(r['kernel_ms'])} | {spread(r['count_ms'])} | {spread(r['wall_ms'])} | {spread(r['host_share'])} | "
                    f"{r['readback_ms']:.2f} | {spread(r['fill_ms'])} | {spread(r['catalogue_ms'])} |\n")
        f.write("\nrounds: of the sized call; launches: both calls together (the jumps stop at the first batch that moves nothing, so their number can "
                "differ from run to run).\n")
