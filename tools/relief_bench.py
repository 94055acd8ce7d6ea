"""Relief map timings on the full-size DEM -> profiles/relief_bench.md.

An 8192 x 8192 window of the 23040 x 46080 DEM at footprints (1, 1), (4, 4), (16, 16) and (32, 32): kernel ms of the LDS-staged
kernel at every tile shape and of the kernel that reads each footprint straight from global memory (MOONRT_RELIEF_TILE = 0),
the bytes the window must move at least (its texels and their halo once, 8 B each in the DEM's row-pair storage, plus the
float4 per node written), and the time mrtx_probe_stream takes to read that many bytes on the same machine."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from moonrtx_amd import _lib                                              # noqa: E402
from moonrtx_amd.renderer import DeviceBuffer, MoonRT, synth_ldem, dem_from_ldem        # noqa: E402

DEM_H, DEM_W = 23040, 46080
N = 8192
FOOTPRINTS = ((1, 1), (4, 4), (16, 16), (32, 32))
TILES = (16, 32, 64, 0)


def kernel_ms(rt, t, out, tile, repeats):
    os.environ["MOONRT_RELIEF_TILE"] = str(tile)
    best = None
    for _ in range(repeats + 1):            # the first call warms up
        st = _lib.MrtxStats()
        rt._check(rt._lib.mrtx_relief(rt._ctx, C.byref(t), out.ptr, None, C.byref(st)), "mrtx_relief")
        best = st.kernel_ms if best is None else min(best, st.kernel_ms)
    return best


def stream_ms(lib, nbytes, repeats=5):
    lib.mrtx_probe_stream(0, nbytes, 1)
    t0 = time.perf_counter()
    if lib.mrtx_probe_stream(0, nbytes, repeats) != 0:
        raise RuntimeError("mrtx_probe_stream failed")
    one = time.perf_counter() - t0
    t0 = time.perf_counter()
    lib.mrtx_probe_stream(0, nbytes, 3 * repeats)
    three = time.perf_counter() - t0
    return (three - one) / (2 * repeats) * 1e3      # the allocation and the fill cancel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--direct-max", type=int, default=16, help="largest footprint the direct kernel is timed at")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relief_bench.md"))
    a = ap.parse_args()
    src = synth_ldem(DEM_H, DEM_W)
    dem, scale = dem_from_ldem(src, DEM_H, DEM_W, 1)
    src.free()
    rt = MoonRT(16, 16)
    rt.set_params(flags=0)
    rt.bind_dem(dem, DEM_H, DEM_W)
    out = DeviceBuffer(16 * N * N)
    lines = ["# Relief maps on the full-size DEM", "",
             f"{N} x {N} window of the {DEM_H} x {DEM_W} DEM at (7000, 19000), stride 1, production flags; best of "
             f"{a.repeats} after a warm-up call.  Tile = MOONRT_RELIEF_TILE: nodes per workgroup (16 = 16 x 16, 32 = 32 x 32, "
             "64 = 64 rows x 16 columns), 0 = every footprint read straight from global memory.  Bytes = the window's texels "
             "and halo once at 8 B each + 16 B written per node; stream = mrtx_probe_stream reading that many bytes.", "",
             "| footprint | tile | kernel ms | MB read | MB written | stream ms | kernel / stream |", "|---|---|---|---|---|---|---|"]
    for ri, rj in FOOTPRINTS:
        t = _lib.MrtxRelief(7000, 19000, N, N, 1, ri, rj, 0, 1737400.0 * scale)
        rd, wr = (N + 2 * ri) * (N + 2 * rj) * 8, N * N * 16
        sm = stream_ms(rt._lib, rd + wr)
        for tile in TILES:
            if tile == 0 and ri > a.direct_max:
                lines.append(f"| ({ri}, {rj}) | 0 | not measured (footprints above --direct-max) | | | | |")
                continue
            ms = kernel_ms(rt, t, out, tile, 1 if tile == 0 and ri > 4 else a.repeats)
            lines.append(f"| ({ri}, {rj}) | {tile} | {ms:.3f} | {rd / 1e6:.1f} | {wr / 1e6:.1f} | {sm:.3f} | {ms / sm:.2f} |")
            print(lines[-1], flush=True)
    out.free()
    rt.close()
    dem.free()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
