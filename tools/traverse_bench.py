"""Least-cost traverse timings on the full-size DEM -> profiles/traverse_bench.json.

Per case: kernel ms (init + every relaxation launch + predecessors), relaxation launches, tile visits and visits per tile,
for a 4096 x 4096 mid-latitude window and a wrapped south-polar cap, at tile edges 8, 16 and 32; then a 2048 x 2048 window
against SciPy's Dijkstra on the host over the same float32 weights (the costs compared bit for bit)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from moonrtx_amd.renderer import MoonRT, synth_ldem, dem_from_ldem        # noqa: E402
from moonrtx_amd.traverse import max_slope_grade                         # noqa: E402

DEM_H, DEM_W = 23040, 46080
SLOPE_DEG = 15.0


def run(rt, t, src, tile, repeats):
    """Best of `repeats` traverses of the window of MrtxTraverse t (its grade from SLOPE_DEG) from nodes `src` at tile edge
    `tile`."""
    os.environ["MOONRT_TRAVERSE_TILE"] = str(tile)
    w = (t.row0, t.col0, t.rows, t.cols, t.stride, t.wrap)
    best = f = None
    for _ in range(repeats):
        st = {}
        f = rt.traverse(w, nodes=np.array(src, np.int32), max_slope_deg=SLOPE_DEG, climb_cost=t.climb_cost,
                        descent_cost=t.descent_cost, radius_m=t.radius_m, stats=st, heights=False)
        if best is None or st["kernel_ms"] < best["kernel_ms"]:
            best = dict(st)
    tiles = -(-t.rows // tile) * -(-t.cols // tile)
    best.update(tile=tile, tiles=tiles, visits_per_tile=best["tile_visits"] / tiles,
                reachable=float(np.isfinite(f.cost).mean()), no_pred=int((f.pred == 254).sum()))
    return best, f.cost


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "traverse_bench.json"))
    a = ap.parse_args()
    import traverse_model as tm
    src = synth_ldem(DEM_H, DEM_W)
    dem, scale = dem_from_ldem(src, DEM_H, DEM_W, 1)
    src.free()
    rt = MoonRT(16, 16)
    rt.bind_dem(dem, DEM_H, DEM_W)
    rm = 1737400.0 * scale
    grade = max_slope_grade(SLOPE_DEG)          # what MoonRT.traverse makes of it
    cases = {
        "mid-latitude 4096 x 4096": (tm.make_window(9000, 20000, 4096, 4096, radius_m=rm, max_grade=grade), [(2048, 2048)]),
        "south-polar cap 512 x 3840, stride 12, wrapped": (
            tm.make_window(DEM_H - 1 - 511 * 12, 0, 512, 3840, stride=12, wrap=1, radius_m=rm, max_grade=grade), [(500, 100)]),
    }
    res = {"dem": [DEM_H, DEM_W], "max_slope_deg": SLOPE_DEG, "climb_cost": 8.0, "descent_cost": 0.0, "cases": {}}
    for name, (t, s) in cases.items():
        res["cases"][name] = []
        for tile in (32, 16, 8):
            r, _ = run(rt, t, s, tile, a.repeats)
            res["cases"][name].append(r)
            print(name, json.dumps(r), flush=True)
    if not a.no_scipy:
        from scipy.sparse import csr_matrix
        from scipy.sparse.csgraph import dijkstra
        t = tm.make_window(10000, 21000, 2048, 2048, radius_m=rm, max_grade=grade)
        r, d = run(rt, t, [(1024, 1024)], 32, a.repeats)
        D = rt.traverse_heights((t.row0, t.col0, t.rows, t.cols))
        wt = tm.weights(D, None, tm.lengths(t, (DEM_H, DEM_W)), t)
        rows, cols = t.rows, t.cols
        ii, jj = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
        us, vs, ws = [], [], []
        for k in range(8):
            ui, uj = ii + tm.DI[k], jj + tm.DJ[k]
            ok = (ui >= 0) & (ui < rows) & (uj >= 0) & (uj < cols) & np.isfinite(wt[k])
            us.append((ui * cols + uj)[ok]); vs.append((ii * cols + jj)[ok]); ws.append(wt[k][ok].astype(np.float64))
        g = csr_matrix((np.concatenate(ws), (np.concatenate(us), np.concatenate(vs))), shape=(rows * cols,) * 2)
        t0 = time.perf_counter()
        ref = dijkstra(g, directed=True, indices=[1024 * cols + 1024], min_only=True).reshape(rows, cols)
        host_s = time.perf_counter() - t0
        same = bool(np.array_equal(ref.view(np.uint64), d.view(np.uint64)))
        res["scipy_2048"] = dict(gpu=r, scipy_dijkstra_s=host_s, edges=int(g.nnz), bit_equal=same)
        print("scipy 2048^2", json.dumps(res["scipy_2048"]), flush=True)
    rt.close()
    dem.free()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"traverse_bench": a.out}))


if __name__ == "__main__":
    main()
