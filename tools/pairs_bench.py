#!/usr/bin/env python
"""Times the joint availability of mask rows: kernel_ms, pairs and word-pairs per second of
  best    an n x n polar map's nodes (240 m apart) over --epochs epochs, every node's best partner within --max-dist-m, in the
          variants MOONRT_PAIRS = prune and brute (the same bytes and the same pairs, asserted)
  all     --all-rows rows against each other without positions
  rows    ROWS over the map's n x n rows
and, for a yardstick, the seconds the numpy model takes for the best partners of --model-rows rows without positions, with
its word-pairs per second.  The masks are synthetic: each node a day of its own period, phase and length, and a few outages,
so nights last hundreds of epochs as real ones do.  The median of --runs runs after one warm-up.  One JSON line per case.

  python tools/pairs_bench.py --size 256 --epochs 8760 --runs 3 --out profiles/pairs_bench.json"""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
from moonrtx_amd import networks as nw
from moonrtx_amd import traverse as tv
from moonrtx_amd._lib import PAIR_DTYPE
from moonrtx_amd.renderer import DeviceBuffer, MoonRT

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--epochs", type=int, default=8760)
ap.add_argument("--max-dist-m", type=float, default=5000.0)
ap.add_argument("--all-rows", type=int, default=4096)
ap.add_argument("--model-rows", type=int, default=256)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--out")
a = ap.parse_args()


def masks(n_rows, m, seed=1, block=4096):
    """(n_rows, W64) uint64: per row a lit share of 60 to 90 % in days of 500 to 800 epochs, and three outages of up to 200."""
    rng = np.random.default_rng(seed)
    out = np.empty((n_rows, tv.mask_words(m)), np.uint64)
    k = np.arange(m)
    for r0 in range(0, n_rows, block):
        n = min(block, n_rows - r0)
        period = rng.uniform(500, 800, (n, 1))
        bits = ((k[None, :] + rng.uniform(0, 800, (n, 1))) % period) < period * rng.uniform(0.6, 0.9, (n, 1))
        for _ in range(3):
            s = rng.integers(0, m, (n, 1))
            bits &= ~((k[None, :] >= s) & (k[None, :] < s + rng.integers(1, 200, (n, 1))))
        out[r0:r0 + n] = tv.pack_mask(bits)
    return out


def row_stats(J):
    """count, gap and gap_first of every row of booleans: the numpy model."""
    idx = np.arange(J.shape[-1])
    run = idx - np.maximum.accumulate(np.where(J, idx, -1), axis=-1)
    gap = run.max(axis=-1)
    return J.sum(axis=-1), gap, np.where(gap > 0, run.argmax(axis=-1) - gap + 1, -1)


def timed(rt, call, runs):
    ms, pairs, launches, res = [], set(), 0, None
    for r in range(runs + (runs > 1)):
        st = {}
        res = call(st)
        if r or runs == 1:
            ms.append(st["kernel_ms"])
        pairs.add(st["pairs"])
        launches = st["launches"]
    assert len(pairs) == 1
    return res, {"kernel_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "runs": len(ms),
                 "pairs": pairs.pop(), "launches": launches}


rt = MoonRT(16, 16, device=0)
n, m = a.size * a.size, a.epochs
w64 = tv.mask_words(m)
words = masks(n, m)
i, j = np.divmod(np.arange(n), a.size)
pos = np.stack([240 * j, 240 * i, np.zeros(n, np.int64)], -1).astype(np.int32)
mask_buf, pos_buf, out_buf = DeviceBuffer(words.nbytes), DeviceBuffer(pos.nbytes), DeviceBuffer(16 * n)
mask_buf.upload(words)
pos_buf.upload(pos)
lines = []

rec = {"case": "best", "rows": n, "epochs": m, "words": w64, "max_dist_m": a.max_dist_m}
d2_max = nw.distance_d2(a.max_dist_m, 1.0, False)
got = {}
for variant in ("prune", "brute"):
    os.environ["MOONRT_PAIRS"] = variant
    _, rec[variant] = timed(rt, lambda st: rt.mask_pairs(mask_buf, m, n_rows=n, positions_a=pos_buf, d2_max=d2_max, out=out_buf,
                                                         stats=st), a.runs)
    rec[variant]["word_pairs_per_s"] = rec[variant]["pairs"] * w64 / (rec[variant]["kernel_ms"] * 1e-3)
    got[variant] = out_buf.download(np.uint8, (16 * n,)).tobytes()
assert got["prune"] == got["brute"] and rec["prune"]["pairs"] == rec["brute"]["pairs"]
os.environ["MOONRT_PAIRS"] = "prune"
lines.append(rec)
print(json.dumps(rec), flush=True)

k = min(a.all_rows, n)
rec = {"case": "all", "rows": k, "epochs": m, "words": w64}
_, t = timed(rt, lambda st: rt.mask_pairs(mask_buf, m, n_rows=k, out=out_buf, stats=st), a.runs)
t["word_pairs_per_s"] = t["pairs"] * w64 / (t["kernel_ms"] * 1e-3)
rec.update(t)
lines.append(rec)
print(json.dumps(rec), flush=True)

rec = {"case": "rows", "rows": n, "epochs": m, "words": w64}
_, t = timed(rt, lambda st: rt.mask_pairs(mask_buf, m, n_rows=n, mode="rows", out=out_buf, stats=st), a.runs)
t["words_per_s"] = n * w64 / (t["kernel_ms"] * 1e-3)
rec.update(t)
lines.append(rec)
print(json.dumps(rec), flush=True)

# the numpy model on a subset: every row's best partner by count, then gap, then index
q = min(a.model_rows, k)
bits = tv.unpack_mask(words[:q], m)
t0 = time.perf_counter()
model = np.zeros(q, PAIR_DTYPE)
for r in range(q):
    c, g, f = row_stats(bits[r] | bits)
    c[r] = -1                                               # never itself
    b = np.lexsort((np.arange(q), g, -c))[0]
    model[r] = (b, c[b], g[b], f[b])
sec = time.perf_counter() - t0
dev = rt.mask_pairs(words[:q], m)
assert np.array_equal(dev, model)
rec = {"case": "numpy_model", "rows": q, "epochs": m, "seconds": sec, "pairs": q * (q - 1),
       "word_pairs_per_s": q * (q - 1) * w64 / sec}
lines.append(rec)
print(json.dumps(rec), flush=True)

for b in (mask_buf, pos_buf, out_buf):
    b.free()
rt.close()
if a.out:
    with open(a.out, "w") as f:
        json.dump(lines, f, indent=1)
        f.write("\n")
