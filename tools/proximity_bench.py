#!/usr/bin/env python
"""Times the proximity maps (profiles/proximity.md): kernel_ms and pairs of MOONRT_PROXIMITY = prune and
brute on an n x n wrapped polar window (stride s = 12, less beyond 1920 rows, of a DEM of 23040 rows and s n columns, the last
row beside the pole) with a
feature set of about 5 % of the nodes in compact discs; the median of --runs runs after one warm-up, and the reach of the
discs.  One JSON line per size.

  python tools/proximity_bench.py --sizes 256 1024 --brute-up-to 256 --runs 5 --out profiles/proximity_bench.json"""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
from moonrtx_amd import regions as rg
from moonrtx_amd.renderer import MoonRT

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", type=int, nargs="+", default=[256, 1024])
ap.add_argument("--brute-up-to", type=int, default=256, help="brute is timed up to this size (once above 512)")
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--out")
a = ap.parse_args()


def discs(n, seed=1):
    """About 5 % of an n x n wrapped lattice in discs of radius n / 20: labels, the disc's number or -1."""
    rng = np.random.default_rng(seed)
    rad = max(n // 20, 1)
    k = max(int(round(0.05 * n * n / (np.pi * rad * rad))), 1)
    i, j = np.mgrid[0:n, 0:n]
    lab = np.full((n, n), -1, np.int32)
    for d in range(k):
        ci, cj = rng.integers(0, n, 2)
        dj = (j - cj + n // 2) % n - n // 2
        lab[(i - ci) ** 2 + dj ** 2 <= rad * rad] = d
    return lab, k


rt = MoonRT(16, 16, device=0)
lines = []
for n in a.sizes:
    s = min(12, 23040 // n)                                 # beyond 1920 rows a smaller stride, so that the window fits
    pos = rg.node_positions((23040 - s * n, 0, n, n, s, 1), (23040, s * n))
    lab, k = discs(n)
    rec = {"n": n, "features": int((lab >= 0).sum()), "share": float((lab >= 0).mean()), "discs": k}
    maps = {}
    for variant in ("prune", "brute"):
        if variant == "brute" and n > a.brute_up_to:
            continue
        os.environ["MOONRT_PROXIMITY"] = variant
        runs = 1 if variant == "brute" and n > 512 else a.runs
        ms, pairs = [], set()
        for r in range(runs + (runs > 1)):
            st = {}
            maps[variant] = rt.proximity(lab, pos, stats=st)
            if r or runs == 1:
                ms.append(st["kernel_ms"])
            pairs.add(st["pairs"])
            launches = st["launches"]
        assert len(pairs) == 1
        rec[variant] = {"kernel_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "runs": len(ms),
                        "pairs": pairs.pop(), "launches": launches}
    if "brute" in maps:
        assert maps["prune"].nearest.tobytes() == maps["brute"].nearest.tobytes()
        assert maps["prune"].dist2.tobytes() == maps["brute"].dist2.tobytes()
    os.environ["MOONRT_PROXIMITY"] = "prune"
    ms = []
    for r in range(a.runs + 1):
        st = {}
        rt.region_reach(lab, k, maps["prune"], stats=st)
        if r:
            ms.append(st["kernel_ms"])
    rec["reach"] = {"kernel_ms": statistics.median(ms), "launches": st["launches"]}
    lines.append(rec)
    print(json.dumps(rec), flush=True)
rt.close()
if a.out:
    with open(a.out, "w") as f:
        json.dump(lines, f, indent=1)
        f.write("\n")
