"""Every library call the terrain and lattice methods of MoonRT make, as text: the methods run against the fake library of
tests/fake_moonrt.py, and every call is written with its scalars, its structs, where each pointer points and the CRC32 of
each host input, between the allocations, downloads and frees, followed by what the method returned (or raised) and the
stats it left.  Run it on two trees and compare the files: a refactor of the Python binding must leave them identical byte
for byte.  Needs no GPU and no libmoonrt.so.

    python tools/facade_trace.py before.txt --tree /path/to/a/checkout/of/the/parent
    python tools/facade_trace.py after.txt
    cmp before.txt after.txt
"""
import argparse
import json
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, M, N_AZ = 7, 5, 8                    # points, epochs, horizon azimuths
SCENARIOS = []


def add(name, run, script=None, refuse=(), raises=None):
    """A scenario: run(s) calls one method on s.rt; script = the counts the fake library reports; refuse = the (entry point,
    k) calls it refuses; raises = the exception the method must end with."""
    SCENARIOS.append((name, run, script or {}, set(refuse), raises))


class Scene:
    """What a scenario works with: a fresh MoonRT on the fake library, a stats dict, and seeded inputs."""

    def __init__(self, rmod, fake):
        self.rmod, self.fake, self.stats, self.bufs = rmod, fake, {}, []
        self.rt = rmod.MoonRT(8, 8)
        self.rng = np.random.default_rng(20260101)
        self.la, self.lo = np.arange(N) * 1.5 - 4.0, np.arange(N) * 2.0 - 3.0
        self.ep, self.ep2 = self.rng.normal(size=(M, 14)), self.rng.normal(size=(M, 14))
        self.hz = self.rng.normal(size=(N, N_AZ)).astype(np.float32)
        self.flux = np.linspace(1300.0, 1400.0, M)

    def dev(self, array, device=0):
        """A DeviceBuffer holding `array`."""
        a = np.ascontiguousarray(array)
        b = self.rmod.DeviceBuffer(a.nbytes, device)
        b.upload(a)
        self.bufs.append(b)
        return b

    def empty(self, nbytes):
        b = self.rmod.DeviceBuffer(nbytes)
        self.bufs.append(b)
        return b

    def ints(self, shape, lo=-1, hi=3, dtype=np.int32):
        return self.rng.integers(lo, hi, shape).astype(dtype)

    def field(self, shape):
        return self.rng.normal(size=shape).astype(np.float32)

    def model(self, n_spin=2):
        m = self.rmod.MoonRT.thermal_grid()
        m.n_spin = n_spin
        return m

    def dem(self):
        self.rt.upload_dem(np.ones((16, 32), np.float32))
        return self.rt


# ---- the terrain methods ----------------------------------------------------------------------------------------------
def terrain():
    T = "terrain."
    add(T + "sun_samples", lambda s: s.rt.sun_samples(4))
    add(T + "sun_samples bad n", lambda s: s.rt.sun_samples(3), raises=ValueError)
    add(T + "grid_nodes", lambda s: s.rmod.MoonRT.grid_nodes((10, -10), (0, 40), (4, 5)))
    add(T + "horizon_azimuths", lambda s: s.rmod.MoonRT.horizon_azimuths(8))
    add(T + "horizon_azimuths bad", lambda s: s.rt.horizon_azimuths(6), raises=ValueError)
    add(T + "power_scale", lambda s: (s.rt.power_scale([100.0, 250.0], 40.0), s.rt.power_scale([0.0], 0.0), s.rt.power_scale(0.5, 0.25)))
    add(T + "power_scale inf", lambda s: s.rt.power_scale([np.inf], 1.0), raises=ValueError)
    add(T + "power_scale too large", lambda s: s.rt.power_scale([1e30], 1.0), raises=ValueError)
    add(T + "view_samples", lambda s: s.rt.view_samples(16))
    add(T + "view_samples bad", lambda s: s.rt.view_samples(5), raises=ValueError)
    add(T + "thermal_depths", lambda s: (s.rt.thermal_depths(), s.rmod.MoonRT.thermal_depths(s.model())))

    grid = dict(lat=(10.0, -10.0), lon=(0.0, 40.0), shape=(6, 5))
    add(T + "illumination_map unbanded", lambda s: s.rt.illumination_map(**grid, n_sun=4, stats=s.stats))
    add(T + "illumination_map banded", lambda s: s.rt.illumination_map(**grid, band_bytes=16 * 5 * 2, stats=s.stats))
    add(T + "illumination_map rows uneven", lambda s: s.rt.illumination_map(**grid, rows=(1, 6), band_bytes=16 * 5 * 2, stats=s.stats))
    add(T + "illumination_at", lambda s: s.rt.illumination_at(s.la, s.lo, n_sun=8, stats=s.stats))
    add(T + "illumination_at mismatch", lambda s: s.rt.illumination_at(s.la, s.lo[:3]), raises=ValueError)

    add(T + "illumination_series", lambda s: s.rt.illumination_series(s.la, s.lo, s.ep, stats=s.stats))
    add(T + "illumination_series count", lambda s: s.rt.illumination_series(s.la, s.lo, s.ep, count=3))
    add(T + "illumination_series first", lambda s: s.rt.illumination_series(s.la, s.lo, s.ep, first=np.arange(N) % 3, count=2, stats=s.stats))
    add(T + "illumination_series uneven chunks", lambda s: s.rt.illumination_series(s.la, s.lo, s.ep, first=np.arange(N) % 2, count=3,
                                                                                     chunk_bytes=3 * 48, stats=s.stats))
    add(T + "illumination_series no points", lambda s: s.rt.illumination_series([], [], s.ep, stats=s.stats))
    add(T + "illumination_series first without count", lambda s: s.rt.illumination_series(s.la, s.lo, s.ep, first=np.zeros(N)), raises=ValueError)
    add(T + "illumination_series first shape", lambda s: s.rt.illumination_series(s.la, s.lo, s.ep, first=[0, 1], count=2), raises=ValueError)
    add(T + "illumination_series points mismatch", lambda s: s.rt.illumination_series(s.la, s.lo[:2], s.ep), raises=ValueError)
    add(T + "illumination_series bad epochs", lambda s: s.rt.illumination_series(s.la, s.lo, np.zeros((M, 13))), raises=ValueError)

    add(T + "horizon", lambda s: s.rt.horizon(s.la, s.lo, n_az=N_AZ, n_bis=5, stats=s.stats))
    add(T + "horizon uneven chunks", lambda s: s.rt.horizon(s.la, s.lo, n_az=N_AZ, chunk_bytes=3 * 4 * N_AZ, stats=s.stats))
    add(T + "horizon height scalar", lambda s: s.rt.horizon(s.la, s.lo, n_az=N_AZ, height_m=2.0, radius_m=1000.0, stats=s.stats))
    add(T + "horizon height per point", lambda s: s.rt.horizon(s.la, s.lo, n_az=N_AZ, height_m=np.arange(N), chunk_bytes=3 * 4 * N_AZ))
    add(T + "horizon height size", lambda s: s.rt.horizon(s.la, s.lo, n_az=N_AZ, height_m=[1.0, 2.0]), raises=ValueError)
    add(T + "horizon out", lambda s: s.rt.horizon(s.la, s.lo, n_az=N_AZ, out=s.empty(4 * N * N_AZ), chunk_bytes=3 * 4 * N_AZ, stats=s.stats))
    add(T + "horizon out small", lambda s: s.rt.horizon(s.la, s.lo, n_az=N_AZ, out=s.empty(4 * N * N_AZ - 4)), raises=ValueError)
    add(T + "horizon no points", lambda s: s.rt.horizon([], [], n_az=N_AZ, stats=s.stats), raises=s_error())

    def both(name, run, **kw):          # a query that reads horizons: from the host and from a DeviceBuffer
        add(T + name, lambda s: run(s, s.hz, {}), **kw)
        add(T + name + " device horizon", lambda s: run(s, s.dev(s.hz), {"n_az": N_AZ}), **kw)
    both("horizon_windows", lambda s, hz, kw: s.rt.horizon_windows(s.la, s.lo, hz, s.ep, s.ep2, min_a=0.25, min_b=0.75, stats=s.stats, **kw))
    both("horizon_windows uneven chunks", lambda s, hz, kw: s.rt.horizon_windows(s.la, s.lo, hz, s.ep, s.ep2, chunk_bytes=3 * 4 * (N_AZ + 8),
                                                                                 stats=s.stats, **kw))
    add(T + "horizon_windows epochs differ", lambda s: s.rt.horizon_windows(s.la, s.lo, s.hz, s.ep, s.ep2[:3]), raises=ValueError)
    add(T + "horizon_windows no n_az", lambda s: s.rt.horizon_windows(s.la, s.lo, s.dev(s.hz), s.ep, s.ep2), raises=ValueError)
    add(T + "horizon_windows buffer small", lambda s: s.rt.horizon_windows(s.la, s.lo, s.dev(s.hz[1:]), s.ep, s.ep2, n_az=N_AZ), raises=ValueError)
    add(T + "horizon_windows horizon shape", lambda s: s.rt.horizon_windows(s.la, s.lo, s.hz[1:], s.ep, s.ep2), raises=ValueError)

    both("horizon_mask", lambda s, hz, kw: s.rt.horizon_mask(s.la, s.lo, hz, s.ep, s.ep2, stats=s.stats, **kw))
    both("horizon_mask one body", lambda s, hz, kw: s.rt.horizon_mask(s.la, s.lo, hz, s.ep, None, min_a=0.1, stats=s.stats, **kw))
    both("horizon_mask uneven chunks", lambda s, hz, kw: s.rt.horizon_mask(s.la, s.lo, hz, s.ep, chunk_bytes=3 * 4 * (N_AZ + 2), stats=s.stats, **kw))
    add(T + "horizon_mask out offset", lambda s: s.rt.horizon_mask(s.la, s.lo, s.hz, s.ep, s.ep2, out=s.empty(16 + 8 * N), out_offset=16,
                                                                   chunk_bytes=3 * 4 * (N_AZ + 2), stats=s.stats))
    add(T + "horizon_mask out offset odd", lambda s: s.rt.horizon_mask(s.la, s.lo, s.hz, s.ep, out=s.empty(64 + 8 * N), out_offset=4), raises=ValueError)
    add(T + "horizon_mask out small", lambda s: s.rt.horizon_mask(s.la, s.lo, s.hz, s.ep, out=s.empty(8 * N), out_offset=8), raises=ValueError)
    add(T + "horizon_mask epochs differ", lambda s: s.rt.horizon_mask(s.la, s.lo, s.hz, s.ep, s.ep2[:2]), raises=ValueError)

    gen = np.linspace(100.0, 300.0, M)
    both("power_budget summary", lambda s, hz, kw: s.rt.power_budget(s.la, s.lo, hz, s.ep, gen, 40.0, stats=s.stats, **kw))
    both("power_budget full uneven chunks", lambda s, hz, kw: s.rt.power_budget(s.la, s.lo, hz, s.ep, gen, gen[::-1], mode="full",
                                                                                chunk_bytes=3 * 4 * M, stats=s.stats, **kw))
    add(T + "power_budget fixed", lambda s: s.rt.power_budget(s.la, s.lo, s.hz, s.ep, gen, 40.0, panel="fixed", normal_enu=(0.0, 0.6, 0.8),
                                                              cpw_log2=3, capacity=1000, initial=10, chunk_bytes=3 * 4 * (N_AZ + 16)))
    add(T + "power_budget azimuth", lambda s: s.rt.power_budget(s.la, s.lo, s.hz, s.ep, gen, 40.0, panel="azimuth", capacity=77))
    add(T + "power_budget bad mode", lambda s: s.rt.power_budget(s.la, s.lo, s.hz, s.ep, gen, 40.0, mode="all"), raises=ValueError)
    add(T + "power_budget bad panel", lambda s: s.rt.power_budget(s.la, s.lo, s.hz, s.ep, gen, 40.0, panel="flat"), raises=ValueError)
    add(T + "power_budget normal without fixed", lambda s: s.rt.power_budget(s.la, s.lo, s.hz, s.ep, gen, 40.0, normal_enu=(0, 0, 1)), raises=ValueError)
    add(T + "power_budget fixed without normal", lambda s: s.rt.power_budget(s.la, s.lo, s.hz, s.ep, gen, 40.0, panel="fixed"), raises=ValueError)

    both("horizon_sun", lambda s, hz, kw: s.rt.horizon_sun(s.la, s.lo, hz, s.ep, stats=s.stats, **kw))
    both("horizon_sun summary", lambda s, hz, kw: s.rt.horizon_sun(s.la, s.lo, hz, s.ep, summary=True, chunk_bytes=8, stats=s.stats, **kw))
    both("horizon_sun uneven chunks", lambda s, hz, kw: s.rt.horizon_sun(s.la, s.lo, hz, s.ep, chunk_bytes=3 * 4 * M, stats=s.stats, **kw))
    add(T + "horizon_sun no points", lambda s: s.rt.horizon_sun([], [], np.zeros((0, N_AZ), np.float32), s.ep, stats=s.stats), raises=s_error())

    add(T + "occultation", lambda s: s.rt.occultation(s.la, s.lo, s.ep, s.ep2, stats=s.stats))
    add(T + "occultation summary", lambda s: s.rt.occultation(s.la, s.lo, s.ep, s.ep2, summary=True, chunk_bytes=8, stats=s.stats))
    add(T + "occultation uneven chunks", lambda s: s.rt.occultation(s.la, s.lo, s.ep, s.ep2, chunk_bytes=3 * 4 * M, stats=s.stats))
    add(T + "occultation epochs differ", lambda s: s.rt.occultation(s.la, s.lo, s.ep, s.ep2[:1]), raises=ValueError)

    pos = np.random.default_rng(5).normal(size=(2, M, 3)) * 2e6
    for mode in ("full", "summary", "list"):
        both(f"horizon_passes {mode}", lambda s, hz, kw, mode=mode: s.rt.horizon_passes(s.la, s.lo, hz, pos, mode=mode, stats=s.stats, **kw),
             script={"passes": 3})
        add(T + f"horizon_passes {mode} uneven chunks",
            lambda s, mode=mode: s.rt.horizon_passes(s.la, s.lo, s.hz, pos, mode=mode, height_m=np.arange(N), min_elev_deg=5.0,
                                                     chunk_bytes=3 * {"full": 16 * 2 * M, "summary": 4 * (N_AZ + 8), "list": 4 * N_AZ + 24}[mode],
                                                     stats=s.stats), script={"passes": 2})
    add(T + "horizon_passes list none", lambda s: s.rt.horizon_passes(s.la, s.lo, s.hz, pos[0], mode="list", height_m=3.0, radius_m=1e6, stats=s.stats))
    add(T + "horizon_passes fill refused", lambda s: s.rt.horizon_passes(s.la, s.lo, s.hz, pos, mode="list", stats=s.stats), script={"passes": 3},
        refuse=[("mrtx_horizon_passes", 1)], raises=s_error())
    add(T + "horizon_passes bad mode", lambda s: s.rt.horizon_passes(s.la, s.lo, s.hz, pos, mode="table"), raises=ValueError)
    add(T + "horizon_passes bad positions", lambda s: s.rt.horizon_passes(s.la, s.lo, s.hz, pos[:, :, :2]), raises=ValueError)

    for mode in ("summary", "full", "flux"):
        both(f"surface_temperature {mode}", lambda s, hz, kw, mode=mode: s.rt.surface_temperature(s.la, s.lo, hz, s.ep, s.flux, model=s.model(),
                                                                                                  mode=mode, chunk_bytes=3 * 4 * 3, stats=s.stats, **kw))
    add(T + "surface_temperature default model", lambda s: s.rt.surface_temperature(s.la, s.lo, s.hz, s.ep, s.flux, stats=s.stats))
    add(T + "surface_temperature bad mode", lambda s: s.rt.surface_temperature(s.la, s.lo, s.hz, s.ep, s.flux, mode="column"), raises=ValueError)
    add(T + "surface_temperature bad flux", lambda s: s.rt.surface_temperature(s.la, s.lo, s.hz, s.ep, s.flux[:2]), raises=ValueError)
    add(T + "surface_temperature no points", lambda s: s.rt.surface_temperature([], [], np.zeros((0, N_AZ), np.float32), s.ep, s.flux), raises=s_error())

    add(T + "view_hits", lambda s: s.rt.view_hits(s.la, s.lo, k=16, stats=s.stats))
    add(T + "view_hits uneven chunks", lambda s: s.rt.view_hits(s.la, s.lo, k=16, chunk_bytes=3 * 4 * 33, stats=s.stats))
    add(T + "view_hits no points", lambda s: s.rt.view_hits([], [], k=16, stats=s.stats), raises=s_error())

    ix = np.random.default_rng(6).integers(-1, 4, (N, 3))
    ex = np.random.default_rng(7).normal(size=(4, M, 2)).astype(np.float32)
    add(T + "scatter_flux", lambda s: s.rt.scatter_flux(ix, ex, 0.1, 0.95, stats=s.stats))
    add(T + "scatter_flux device", lambda s: s.rt.scatter_flux(ix, s.dev(ex), 0.1, 0.95, n_hits=4, m=M, out=s.empty(4 * N * M), stats=s.stats))
    add(T + "scatter_flux device no sizes", lambda s: s.rt.scatter_flux(ix, s.dev(ex), 0.1, 0.95), raises=ValueError)
    add(T + "scatter_flux bad index", lambda s: s.rt.scatter_flux(ix[0], ex, 0.1, 0.95), raises=ValueError)
    add(T + "scatter_flux bad exitance", lambda s: s.rt.scatter_flux(ix, ex[0], 0.1, 0.95), raises=ValueError)
    add(T + "scatter_flux out small", lambda s: s.rt.scatter_flux(ix, ex, 0.1, 0.95, out=s.empty(4)), raises=ValueError)

    xf = np.random.default_rng(8).normal(size=(N, M)).astype(np.float32)
    for mode in ("full", "summary", "flux", "exitance"):
        both(f"surface_temperature_scatter {mode}",
             lambda s, hz, kw, mode=mode: s.rt.surface_temperature_scatter(s.la, s.lo, hz, s.ep, s.flux, model=s.model(), mode=mode, stats=s.stats, **kw))
    add(T + "surface_temperature_scatter extra host", lambda s: s.rt.surface_temperature_scatter(s.la, s.lo, s.hz, s.ep, s.flux, extra_flux=xf, stats=s.stats))
    add(T + "surface_temperature_scatter extra device out",
        lambda s: s.rt.surface_temperature_scatter(s.la, s.lo, s.hz, s.ep, s.flux, model=s.model(), mode="exitance", extra_flux=s.dev(xf),
                                                   out=s.empty(4 * N * 3 * 2), stats=s.stats))
    add(T + "surface_temperature_scatter out small",
        lambda s: s.rt.surface_temperature_scatter(s.la, s.lo, s.hz, s.ep, s.flux, model=s.model(), mode="full", out=s.empty(4 * N * 3 - 4)), raises=ValueError)
    add(T + "surface_temperature_scatter bad mode", lambda s: s.rt.surface_temperature_scatter(s.la, s.lo, s.hz, s.ep, s.flux, mode="column"), raises=ValueError)
    add(T + "surface_temperature_scatter bad flux", lambda s: s.rt.surface_temperature_scatter(s.la, s.lo, s.hz, s.ep, s.flux[:1]), raises=ValueError)

    b4 = (1.0, 2.0, 3.0, 4.0)
    for mode in ("full", "summary", "flux", "exitance", "column", "volatile"):
        sp = b4 if mode == "volatile" else None
        both(f"thermal_column {mode}", lambda s, hz, kw, mode=mode, sp=sp: s.rt.thermal_column(s.la, s.lo, hz, s.ep, s.flux, model=s.model(), mode=mode,
                                                                                               species=sp, stats=s.stats, **kw))
        add(T + f"thermal_column {mode} occulted",
            lambda s, mode=mode, sp=sp: s.rt.thermal_column(s.la, s.lo, s.hz, s.ep, s.flux, model=s.model(), mode=mode, species=sp,
                                                            occultation=(s.ep2, s.ep), stats=s.stats))
    add(T + "thermal_column extra out", lambda s: s.rt.thermal_column(s.la, s.lo, s.hz, s.ep, s.flux, model=s.model(), extra_flux=xf,
                                                                      out=s.empty(4 * N * 3 * s.model().n_nodes), stats=s.stats))
    add(T + "thermal_column extra device occulted out",
        lambda s: s.rt.thermal_column(s.la, s.lo, s.hz, s.ep, s.flux, model=s.model(), mode="volatile", species=s.rmod._lib.MrtxVolatile(b4),
                                      extra_flux=s.dev(xf), out=s.empty(16 * N * s.model().n_nodes), occultation=(s.ep, s.ep2), stats=s.stats))
    add(T + "thermal_column default species", lambda s: s.rt.thermal_column(s.la, s.lo, s.hz, s.ep, s.flux, mode="volatile", species=volatile_species(s)))
    add(T + "thermal_column out small", lambda s: s.rt.thermal_column(s.la, s.lo, s.hz, s.ep, s.flux, model=s.model(), out=s.empty(8)), raises=ValueError)
    add(T + "thermal_column bad mode", lambda s: s.rt.thermal_column(s.la, s.lo, s.hz, s.ep, s.flux, mode="nodes"), raises=ValueError)
    add(T + "thermal_column bad mode with species", lambda s: s.rt.thermal_column(s.la, s.lo, s.hz, s.ep, s.flux, mode="nodes", species=b4), raises=ValueError)
    add(T + "thermal_column species without volatile", lambda s: s.rt.thermal_column(s.la, s.lo, s.hz, s.ep, s.flux, species=b4), raises=ValueError)
    add(T + "thermal_column volatile without species", lambda s: s.rt.thermal_column(s.la, s.lo, s.hz, s.ep, s.flux, mode="volatile"), raises=ValueError)
    add(T + "thermal_column bad flux", lambda s: s.rt.thermal_column(s.la, s.lo, s.hz, s.ep, s.flux[:3]), raises=ValueError)
    add(T + "thermal_column occultation rows", lambda s: s.rt.thermal_column(s.la, s.lo, s.hz, s.ep, s.flux, occultation=(s.ep2[:2], s.ep)), raises=ValueError)

    add(T + "viewshed unbanded", lambda s: s.rt.viewshed((1.0, 2.0, 3.0), **grid, target_height_m=2.0, mast_max_m=8.0, n_bis=3, stats=s.stats))
    add(T + "viewshed banded", lambda s: s.rt.viewshed((1.0, 2.0, 3.0), **grid, rows=(1, 6), band_bytes=4 * 5 * 2, stats=s.stats))
    add(T + "viewshed bad observer", lambda s: s.rt.viewshed((1.0, 2.0), **grid), raises=ValueError)
    add(T + "line_of_sight shared", lambda s: s.rt.line_of_sight(s.la, s.lo, (1.0, 2.0, 3.0), target_height_m=1.5, mast_max_m=4.0, n_bis=2,
                                                                 chunk_bytes=12, stats=s.stats))
    add(T + "line_of_sight per target", lambda s: s.rt.line_of_sight(s.la, s.lo, np.stack([s.la, s.lo, s.la * 0 + 2.0], -1), chunk_bytes=12, stats=s.stats))
    add(T + "line_of_sight no points", lambda s: s.rt.line_of_sight([], [], (1.0, 2.0, 3.0), stats=s.stats))
    add(T + "line_of_sight bad observer", lambda s: s.rt.line_of_sight(s.la, s.lo, np.zeros((2, 3))), raises=ValueError)

    win, wrapped = (2, 3, 4, 5), (2, 0, 4, 16, 2, 1)
    add(T + "traverse_nodes", lambda s: (s.dem().traverse_nodes(win), s.rt.traverse_nodes(wrapped)))
    add(T + "traverse_nodes no dem", lambda s: s.rt.traverse_nodes(win), raises=s_error())
    add(T + "snap_to_nodes", lambda s: (s.dem().snap_to_nodes(win, [60.0, 50.0], [-140.0, -120.0]), s.rt.snap_to_nodes(wrapped, [50.0], [170.0])))
    add(T + "snap_to_nodes outside", lambda s: s.dem().snap_to_nodes(win, [-60.0], [0.0]), raises=ValueError)
    nodes = np.array([[0, 0], [3, 4]])
    pen = np.random.default_rng(9).random((4, 5)).astype(np.float32)
    add(T + "traverse sources", lambda s: s.dem().traverse(win, sources=[[60.0, -140.0], [50.0, -120.0]], stats=s.stats), script={"visits": 11})
    add(T + "traverse nodes penalty", lambda s: s.dem().traverse(win, nodes=nodes, penalty=pen, start_cost=[1.0, 2.0], max_slope_deg=15.0, climb_cost=4.0,
                                                                 descent_cost=1.0, radius_m=1000.0, heights=False, stats=s.stats), script={"visits": 5})
    add(T + "traverse one node device penalty wrapped", lambda s: s.dem().traverse(wrapped, nodes=[1, 2], penalty=s.dev(np.ones((4, 16), np.float32)), start_cost=3.0))
    add(T + "traverse both", lambda s: s.dem().traverse(win, sources=[[60.0, -140.0]], nodes=nodes), raises=ValueError)
    add(T + "traverse neither", lambda s: s.dem().traverse(win), raises=ValueError)
    add(T + "traverse float nodes", lambda s: s.dem().traverse(win, nodes=[[0.5, 1.0]]), raises=ValueError)
    add(T + "traverse nodes shape", lambda s: s.dem().traverse(win, nodes=np.zeros((2, 3), int)), raises=ValueError)
    add(T + "traverse sources shape", lambda s: s.dem().traverse(win, sources=np.zeros((2, 3))), raises=ValueError)
    add(T + "traverse penalty shape", lambda s: s.dem().traverse(win, nodes=nodes, penalty=pen[:3]), raises=ValueError)
    add(T + "traverse penalty buffer small", lambda s: s.dem().traverse(win, nodes=nodes, penalty=s.empty(4 * 19)), raises=ValueError)
    add(T + "traverse refused", lambda s: s.dem().traverse(win, nodes=nodes), refuse=[("mrtx_traverse", 0)], raises=s_error())
    av = np.random.default_rng(10).integers(0, 2 ** 62, (4, 5, 2), dtype=np.uint64)
    add(T + "traverse_timed", lambda s: s.dem().traverse_timed(win, nodes=nodes, stats=s.stats), script={"visits": 4})
    add(T + "traverse_timed avail", lambda s: s.dem().traverse_timed(win, nodes=nodes, start_tick=[5, 9], avail=av, n_epochs=100, ticks_per_epoch=60,
                                                                     ticks_per_cost=2.5, penalty=pen, stats=s.stats))
    add(T + "traverse_timed avail flat", lambda s: s.dem().traverse_timed(win, sources=[[60.0, -140.0]], avail=av.reshape(20, 2), start_tick=7))
    add(T + "traverse_timed device", lambda s: s.dem().traverse_timed(win, nodes=nodes, avail=s.dev(av), n_epochs=128, penalty=s.dev(pen), stats=s.stats))
    add(T + "traverse_timed device no epochs", lambda s: s.dem().traverse_timed(win, nodes=nodes, avail=s.dev(av)), raises=ValueError)
    add(T + "traverse_timed device small", lambda s: s.dem().traverse_timed(win, nodes=nodes, avail=s.dev(av), n_epochs=129), raises=ValueError)
    add(T + "traverse_timed avail shape", lambda s: s.dem().traverse_timed(win, nodes=nodes, avail=av[:3]), raises=ValueError)
    add(T + "traverse_timed avail words", lambda s: s.dem().traverse_timed(win, nodes=nodes, avail=av, n_epochs=64), raises=ValueError)
    add(T + "traverse_heights", lambda s: s.dem().traverse_heights(win, stats=s.stats))

    add(T + "relief nodes", lambda s: s.dem().relief(win, footprint_nodes=(2, 3), radius_m=1000.0, stats=s.stats))
    add(T + "relief metres two bands", lambda s: s.dem().relief(win, footprint_m=100.0, radius_m=1000.0, stats=s.stats), script={"scales": (20.0, 40.0, 20.0)})
    add(T + "relief both", lambda s: s.dem().relief(win, footprint_m=100.0, footprint_nodes=(1, 1)), raises=ValueError)
    add(T + "relief neither", lambda s: s.dem().relief(win), raises=ValueError)
    add(T + "relief wrapped", lambda s: s.dem().relief(wrapped, footprint_nodes=(1, 1)), raises=ValueError)
    add(T + "relief bad footprint", lambda s: s.dem().relief(win, footprint_m=-1.0), raises=ValueError)
    add(T + "landing_share nodes", lambda s: s.rt.landing_share(s.dem().relief(win, footprint_nodes=(1, 1)), 10.0, 0.5, ellipse_nodes=(1, 2), stats=s.stats))
    add(T + "landing_share metres", lambda s: s.rt.landing_share(s.dem().relief(win, footprint_nodes=(1, 1), radius_m=1000.0), 10.0, 0.5, ellipse_m=200.0),
        script={"scales": (20.0, 40.0, 20.0)})
    add(T + "landing_share both", lambda s: s.rt.landing_share(s.dem().relief(win, footprint_nodes=(1, 1)), 10.0, 0.5, ellipse_m=1.0, ellipse_nodes=(1, 1)),
        raises=ValueError)


def s_error():
    """MoonRTError by name: the class itself belongs to the tree under test."""
    return "MoonRTError"


def volatile_species(s):
    from moonrtx_amd import volatiles
    return volatiles.H2O


# ---- the lattice methods ----------------------------------------------------------------------------------------------
def lattice():
    L = "lattice."
    R, Cc = 5, 6

    def sides(name, host, device, **kw):        # a method with host tables and with DeviceBuffers
        add(L + name + " host", host, **kw)
        add(L + name + " device", device, **kw)

    # regions
    for n in (0, 3):
        sides(f"regions field {n}", lambda s: s.rt.regions(field=s.field((R, Cc)), lo=-0.5, hi=0.5, stats=s.stats),
              lambda s: s.rt.regions(field=s.dev(s.field((R, Cc))), shape=(R, Cc), lo=-0.5, hi=0.5, stats=s.stats), script={"n_regions": n})
    sides("regions channels", lambda s: s.rt.regions(field=s.field((3, 4, 2)), channel=1, connectivity=8, wrap=True, row_weights=[1, 2, 3], unit_m2=4.0),
          lambda s: s.rt.regions(field=s.dev(s.field((3, 4, 2)), 1), shape=(3, 4, 2), channel=1, connectivity=8, wrap=True, row_weights=[1, 2, 3], unit_m2=4.0),
          script={"n_regions": 2})
    sides("regions mask", lambda s: s.rt.regions(mask=s.ints((8, 9), 0, 2), stats=s.stats),
          lambda s: s.rt.regions(mask=s.dev(s.ints((8, 9), 0, 2, np.uint8)), shape=(8, 9), stats=s.stats), script={"n_regions": 4})
    for k, what in enumerate(("label", "stats")):
        sides(f"regions {what} refused", lambda s: s.rt.regions(mask=s.ints((R, Cc), 0, 2)),
              lambda s: s.rt.regions(mask=s.dev(s.ints((R, Cc), 0, 2, np.uint8)), shape=(R, Cc)), script={"n_regions": 2},
              refuse=[("mrtx_regions_" + what, 0)], raises=s_error())
    add(L + "regions both", lambda s: s.rt.regions(field=s.field((R, Cc)), mask=s.ints((R, Cc))), raises=ValueError)
    add(L + "regions neither", lambda s: s.rt.regions(), raises=ValueError)
    add(L + "regions no shape", lambda s: s.rt.regions(field=s.dev(s.field((R, Cc)))), raises=ValueError)
    add(L + "regions field dims", lambda s: s.rt.regions(field=s.field((R,))), raises=ValueError)
    add(L + "regions mask dims", lambda s: s.rt.regions(mask=s.ints((R, Cc, 2))), raises=ValueError)
    add(L + "regions buffer small", lambda s: s.rt.regions(field=s.dev(s.field((R, Cc))), shape=(R, Cc + 1)), raises=ValueError)
    add(L + "regions mask buffer small", lambda s: s.rt.regions(mask=s.dev(s.ints((R, Cc), 0, 2, np.uint8)), shape=(R + 1, Cc)), raises=ValueError)
    add(L + "regions weights shape", lambda s: s.rt.regions(mask=s.ints((R, Cc)), row_weights=[1, 2]), raises=ValueError)
    add(L + "regions weights float", lambda s: s.rt.regions(mask=s.ints((R, Cc)), row_weights=np.ones(R)), raises=ValueError)
    add(L + "regions weights range", lambda s: s.rt.regions(mask=s.ints((R, Cc)), row_weights=[1, 2, 3, 4, 2 ** 32]), raises=ValueError)
    add(L + "regions weights negative", lambda s: s.rt.regions(mask=s.ints((R, Cc)), row_weights=[1, 2, 3, 4, -1]), raises=ValueError)

    # region_statistics
    def zonal(s, dev, shape=(R, Cc, 2), n=3, **kw):
        lab, f = s.ints(shape[:2]), s.field(shape)
        if dev:
            return s.rt.region_statistics(s.dev(lab), n, s.dev(f), shape=shape, stats=s.stats, **kw)
        return s.rt.region_statistics(lab, n, f if shape[2] > 1 else f[:, :, 0], stats=s.stats, **kw)
    for name, kw in (("plain", {}), ("weights hist", dict(row_weights=np.arange(R), hist=(1, 4, -1.0, 1.0), scale=8.0, wrap=True)),
                     ("hist", dict(hist=(0, 2, 0.0, 2.0))), ("none", dict(n=0)), ("none hist", dict(n=0, hist=(0, 3, 0.0, 1.0))),
                     ("one channel", dict(shape=(3, 4, 1)))):
        sides("region_statistics " + name, lambda s, kw=kw: zonal(s, False, **kw), lambda s, kw=kw: zonal(s, True, **kw))
    sides("region_statistics refused", lambda s: zonal(s, False, hist=(0, 2, 0.0, 2.0)), lambda s: zonal(s, True, hist=(0, 2, 0.0, 2.0)),
          refuse=[("mrtx_regions_zonal", 0)], raises=s_error())
    add(L + "region_statistics mixed", lambda s: s.rt.region_statistics(s.ints((R, Cc)), 2, s.dev(s.field((R, Cc))), shape=(R, Cc, 1)), raises=ValueError)
    add(L + "region_statistics mixed 2", lambda s: s.rt.region_statistics(s.dev(s.ints((R, Cc))), 2, s.field((R, Cc)), shape=(R, Cc, 1)), raises=ValueError)
    add(L + "region_statistics no shape", lambda s: s.rt.region_statistics(s.dev(s.ints((R, Cc))), 2, s.dev(s.field((R, Cc)))), raises=ValueError)
    add(L + "region_statistics short shape", lambda s: s.rt.region_statistics(s.dev(s.ints((R, Cc))), 2, s.dev(s.field((R, Cc))), shape=(R, Cc)), raises=ValueError)
    add(L + "region_statistics field dims", lambda s: s.rt.region_statistics(s.ints((R, Cc)), 2, s.field((R,))), raises=ValueError)
    add(L + "region_statistics shapes differ", lambda s: s.rt.region_statistics(s.ints((R, Cc)), 2, s.field((R, Cc + 1))), raises=ValueError)
    add(L + "region_statistics labels dims", lambda s: s.rt.region_statistics(s.ints((R, Cc, 1)), 2, s.field((R, Cc))), raises=ValueError)
    add(L + "region_statistics label buffer small", lambda s: s.rt.region_statistics(s.dev(s.ints((R, Cc - 1))), 2, s.dev(s.field((R, Cc))), shape=(R, Cc, 1)),
        raises=ValueError)
    add(L + "region_statistics field buffer small", lambda s: s.rt.region_statistics(s.dev(s.ints((R, Cc))), 2, s.dev(s.field((R, Cc))), shape=(R, Cc, 2)),
        raises=ValueError)
    add(L + "region_statistics weights", lambda s: zonal(s, False, row_weights=[1, 2]), raises=ValueError)
    add(L + "region_statistics weights range", lambda s: zonal(s, True, row_weights=[1, 2, 3, 4, 2 ** 32]), raises=ValueError)
    add(L + "region_statistics hist bins", lambda s: zonal(s, False, hist=(0, 0, 0.0, 1.0)), raises=ValueError)
    add(L + "region_statistics hist range", lambda s: zonal(s, True, hist=(0, 2, 1.0, 1.0)), raises=ValueError)

    # region_shapes
    def shapes(s, dev, n=3, **kw):
        lab = s.ints((R, Cc))
        return s.rt.region_shapes(s.dev(lab), n, shape=(R, Cc), stats=s.stats, **kw) if dev else s.rt.region_shapes(lab, n, stats=s.stats, **kw)
    for name, kw in (("plain", {}), ("sides", dict(side_ew=np.arange(R) + 1, side_ns=np.arange(R + 1) + 2, connectivity=8, wrap=True)), ("none", dict(n=0))):
        sides("region_shapes " + name, lambda s, kw=kw: shapes(s, False, **kw), lambda s, kw=kw: shapes(s, True, **kw))
    sides("region_shapes refused", lambda s: shapes(s, False), lambda s: shapes(s, True), refuse=[("mrtx_regions_shape", 0)], raises=s_error())
    add(L + "region_shapes one side", lambda s: shapes(s, False, side_ew=np.ones(R, int)), raises=ValueError)
    add(L + "region_shapes other side", lambda s: shapes(s, True, side_ns=np.ones(R + 1, int)), raises=ValueError)
    add(L + "region_shapes side length", lambda s: shapes(s, False, side_ew=np.ones(R, int), side_ns=np.ones(R, int)), raises=ValueError)
    add(L + "region_shapes no shape", lambda s: s.rt.region_shapes(s.dev(s.ints((R, Cc))), 2), raises=ValueError)

    # proximity and region_reach
    def prox(s, dev, to="set", rows=R, cols=Cc, **kw):
        lab, pos = s.ints((rows, cols)), s.ints((rows, cols, 3), -100, 100)
        if dev:
            return s.rt.proximity(s.dev(lab), s.dev(pos), to=to, shape=(rows, cols), stats=s.stats, **kw)
        return s.rt.proximity(lab, pos.astype(np.int64), to=to, stats=s.stats, **kw)
    for to in ("set", "outside"):
        sides("proximity " + to, lambda s, to=to: prox(s, False, to, unit_m=2.0), lambda s, to=to: prox(s, True, to, unit_m=2.0), script={"pairs": 99})
    sides("proximity small", lambda s: prox(s, False, rows=3, cols=4), lambda s: prox(s, True, rows=3, cols=4))
    sides("proximity refused", lambda s: prox(s, False), lambda s: prox(s, True), refuse=[("mrtx_proximity", 0)], raises=s_error())
    add(L + "proximity bad to", lambda s: prox(s, False, "inside"), raises=ValueError)
    add(L + "proximity mixed", lambda s: s.rt.proximity(s.dev(s.ints((R, Cc))), s.ints((R, Cc, 3)), shape=(R, Cc)), raises=ValueError)
    add(L + "proximity mixed 2", lambda s: s.rt.proximity(s.ints((R, Cc)), s.dev(s.ints((R, Cc, 3)))), raises=ValueError)
    add(L + "proximity no shape", lambda s: s.rt.proximity(s.dev(s.ints((R, Cc))), s.dev(s.ints((R, Cc, 3)))), raises=ValueError)
    add(L + "proximity position buffer small", lambda s: s.rt.proximity(s.dev(s.ints((R, Cc))), s.dev(s.ints((R, Cc, 2))), shape=(R, Cc)), raises=ValueError)
    add(L + "proximity positions shape", lambda s: s.rt.proximity(s.ints((R, Cc)), s.ints((R, Cc, 2))), raises=ValueError)
    add(L + "proximity positions float", lambda s: s.rt.proximity(s.ints((R, Cc)), s.field((R, Cc, 3))), raises=ValueError)
    add(L + "proximity coordinate", lambda s: s.rt.proximity(s.ints((R, Cc)), np.full((R, Cc, 3), 2 ** 29 + 1)), raises=ValueError)
    add(L + "region_reach map", lambda s: s.rt.region_reach(s.ints((R, Cc)), 3, prox(s, False), stats=s.stats))
    add(L + "region_reach pair device labels", lambda s: s.rt.region_reach(s.dev(s.ints((R, Cc))), 2, (s.ints((R, Cc), 0, 50, np.uint64), s.ints((R, Cc))),
                                                                           shape=(R, Cc), stats=s.stats))
    add(L + "region_reach none", lambda s: s.rt.region_reach(s.ints((R, Cc)), 0, (s.ints((R, Cc), 0, 50), s.ints((R, Cc)))))
    add(L + "region_reach shapes differ", lambda s: s.rt.region_reach(s.ints((R, Cc)), 2, (s.ints((R, Cc + 1), 0, 5), s.ints((R, Cc)))), raises=ValueError)
    add(L + "region_reach refused", lambda s: s.rt.region_reach(s.ints((R, Cc)), 2, (s.ints((R, Cc), 0, 5), s.ints((R, Cc)))),
        refuse=[("mrtx_regions_reach", 0)], raises=s_error())

    # region_outlines
    def outl(s, dev, n=3, **kw):
        lab = s.ints((R, Cc))
        return s.rt.region_outlines(s.dev(lab), n, shape=(R, Cc), stats=s.stats, **kw) if dev else s.rt.region_outlines(lab, n, stats=s.stats, **kw)
    for name, kw, script in (("plain", {}, {"rings": 2, "vertices": 9}), ("all weights", dict(corners=False, row_weights=np.arange(R), wrap=True, connectivity=8),
                                                                          {"rings": 1, "vertices": 4}), ("none", dict(n=0), {})):
        sides("region_outlines " + name, lambda s, kw=kw: outl(s, False, **kw), lambda s, kw=kw: outl(s, True, **kw), script=script)
    for k, what in enumerate(("count", "fill")):
        sides(f"region_outlines {what} refused", lambda s: outl(s, False), lambda s: outl(s, True), script={"rings": 2, "vertices": 9},
              refuse=[("mrtx_regions_outline", k)], raises=s_error())
    add(L + "region_outlines weights", lambda s: outl(s, False, row_weights=np.ones(R + 1, int)), raises=ValueError)
    add(L + "region_outlines label buffer small", lambda s: s.rt.region_outlines(s.dev(s.ints((R, Cc))), 2, shape=(R + 1, Cc)), raises=ValueError)

    # contours
    lv = np.array([-1, 0, 2])

    def cont(s, dev, levels=lv, rows=R, cols=Cc, **kw):
        z = s.ints((rows, cols), -5, 5)
        return s.rt.contours(s.dev(z), levels, shape=(rows, cols), stats=s.stats, **kw) if dev else s.rt.contours(z.astype(np.int64), levels, stats=s.stats, **kw)
    for name, kw, script in (("plain", {}, {"lines": 3, "vertices": 10}), ("wrapped", dict(wrap=True, rows=8, cols=9), {"lines": 1, "vertices": 1}), ("none", {}, {})):
        sides("contours " + name, lambda s, kw=kw: cont(s, False, **kw), lambda s, kw=kw: cont(s, True, **kw), script=script)
    for k, what in enumerate(("count", "fill")):
        sides(f"contours {what} refused", lambda s: cont(s, False), lambda s: cont(s, True), script={"lines": 3, "vertices": 10},
              refuse=[("mrtx_contours", k)], raises=s_error())
    add(L + "contours no levels", lambda s: cont(s, False, levels=[]), raises=ValueError)
    add(L + "contours level table", lambda s: cont(s, True, levels=[[1, 2]]), raises=ValueError)
    add(L + "contours float levels", lambda s: cont(s, False, levels=[0.5]), raises=ValueError)
    add(L + "contours levels leave int32", lambda s: cont(s, True, levels=[0, 2 ** 31]), raises=ValueError)
    add(L + "contours z dims", lambda s: s.rt.contours(s.ints((R,)), lv), raises=ValueError)
    add(L + "contours z float", lambda s: s.rt.contours(s.field((R, Cc)), lv), raises=ValueError)
    add(L + "contours z leaves int32", lambda s: s.rt.contours(np.full((R, Cc), 2 ** 31), lv), raises=ValueError)
    add(L + "contours no shape", lambda s: s.rt.contours(s.dev(s.ints((R, Cc))), lv), raises=ValueError)
    add(L + "contours buffer small", lambda s: s.rt.contours(s.dev(s.ints((R, Cc))), lv, shape=(R, Cc + 1)), raises=ValueError)

    # fill_depressions, basins
    def outlets_of(s, kind, rows=R, cols=Cc):
        o = s.ints((rows, cols), 0, 2)
        return {"absent": None, "host": o * 7, "device": None if kind != "device" else s.dev(o.astype(np.uint8))}[kind]

    def fill(s, dev, outlets="absent", rows=R, cols=Cc, **kw):
        z, o = s.ints((rows, cols), -50, 50), outlets_of(s, outlets, rows, cols)
        if dev:
            return s.rt.fill_depressions(s.dev(z), outlets=o, shape=(rows, cols), stats=s.stats, **kw)
        return s.rt.fill_depressions(z.astype(np.int64), outlets=o, stats=s.stats, **kw)
    for kind in ("absent", "host", "device"):
        sides("fill_depressions outlets " + kind, lambda s, kind=kind: fill(s, False, kind, unit_m=0.5), lambda s, kind=kind: fill(s, True, kind, unit_m=0.5),
              script={"visits": 6})
    sides("fill_depressions options", lambda s: fill(s, False, rows=3, cols=4, edge_outlets=False, connectivity=4, wrap=True),
          lambda s: fill(s, True, rows=3, cols=4, edge_outlets=False, connectivity=4, wrap=True))
    sides("fill_depressions refused", lambda s: fill(s, False), lambda s: fill(s, True), refuse=[("mrtx_fill", 0)], raises=s_error())
    add(L + "fill_depressions heights dims", lambda s: s.rt.fill_depressions(s.ints((R,))), raises=ValueError)
    add(L + "fill_depressions heights float", lambda s: s.rt.fill_depressions(s.field((R, Cc))), raises=ValueError)
    add(L + "fill_depressions heights leave int32", lambda s: s.rt.fill_depressions(np.full((R, Cc), -2 ** 31 - 1)), raises=ValueError)
    add(L + "fill_depressions no shape", lambda s: s.rt.fill_depressions(s.dev(s.ints((R, Cc)))), raises=ValueError)
    add(L + "fill_depressions buffer small", lambda s: s.rt.fill_depressions(s.dev(s.ints((R, Cc))), shape=(R + 1, Cc)), raises=ValueError)
    add(L + "fill_depressions outlets shape", lambda s: s.rt.fill_depressions(s.ints((R, Cc)), outlets=s.ints((R, Cc + 1))), raises=ValueError)
    add(L + "fill_depressions outlet buffer small", lambda s: s.rt.fill_depressions(s.ints((R, Cc)), outlets=s.empty(R * Cc - 1)), raises=ValueError)

    def basins(s, kind, n=3, **kw):
        lab, z, f = s.ints((R, Cc)), s.ints((R, Cc), -9, 9), s.ints((R, Cc), -9, 9)
        if kind == "map":
            from moonrtx_amd import basins as bs
            return s.rt.basins(lab, n, bs.FillMap(z, f, 0.5, 4, True), stats=s.stats, **kw)
        if kind == "pair":
            return s.rt.basins(lab, n, (z, f), stats=s.stats, **kw)
        if kind == "device":
            return s.rt.basins(s.dev(lab), n, (s.dev(z), s.dev(f)), shape=(R, Cc), stats=s.stats, **kw)
        return s.rt.basins(lab, n, (z, s.dev(f, 2)), stats=s.stats, **kw)             # "mixed": one table on the device
    for kind in ("map", "pair", "device", "mixed"):
        add(L + "basins " + kind, lambda s, kind=kind: basins(s, kind))
        add(L + "basins options " + kind, lambda s, kind=kind: basins(s, kind, row_weights=np.arange(R) + 1, connectivity=8, wrap=False))
        add(L + "basins none " + kind, lambda s, kind=kind: basins(s, kind, n=0))
        add(L + "basins refused " + kind, lambda s, kind=kind: basins(s, kind), refuse=[("mrtx_fill_basins", 0)], raises=s_error())
    add(L + "basins fill shape", lambda s: s.rt.basins(s.ints((R, Cc)), 2, (s.ints((R, Cc)), s.ints((R, Cc + 1)))), raises=ValueError)
    add(L + "basins heights buffer small", lambda s: s.rt.basins(s.ints((R, Cc)), 2, (s.empty(4 * R * Cc - 4), s.ints((R, Cc)))), raises=ValueError)
    add(L + "basins weights", lambda s: basins(s, "pair", row_weights=[1]), raises=ValueError)

    # bowls, peaks
    def bowls(s, dev, outlets="absent", call="bowls", **kw):
        z, o = s.ints((R, Cc), -50, 50), outlets_of(s, outlets)
        if dev:
            return getattr(s.rt, call)(s.dev(z), outlets=o, shape=(R, Cc), stats=s.stats, **kw)
        return getattr(s.rt, call)(z.astype(np.int64), outlets=o, stats=s.stats, **kw)
    for kind in ("absent", "host", "device"):
        sides("bowls outlets " + kind, lambda s, kind=kind: bowls(s, False, kind, unit_m=0.25), lambda s, kind=kind: bowls(s, True, kind, unit_m=0.25),
              script={"bowls": 3, "rounds": 2})
    for name, kw, script in (("no labels", dict(labels=False), {"bowls": 2, "rounds": 1}), ("none", {}, {}), ("none no labels", dict(labels=False), {}),
                             ("options", dict(edge_outlets=False, connectivity=4, wrap=True, invert=True, row_weights=np.arange(R) + 1), {"bowls": 1}),
                             ("peaks", dict(call="peaks", row_weights=np.arange(R)), {"bowls": 4, "rounds": 3})):
        sides("bowls " + name, lambda s, kw=kw: bowls(s, False, **kw), lambda s, kw=kw: bowls(s, True, **kw), script=script)
    for k, what in enumerate(("count", "fill")):
        sides(f"bowls {what} refused", lambda s: bowls(s, False, "host"), lambda s: bowls(s, True, "host"), script={"bowls": 3},
              refuse=[("mrtx_bowls", k)], raises=s_error())
        add(L + f"bowls {what} refused no labels device", lambda s: bowls(s, True, labels=False), script={"bowls": 3}, refuse=[("mrtx_bowls", k)], raises=s_error())
    add(L + "bowls heights dims", lambda s: s.rt.bowls(s.ints((R, Cc, 1))), raises=ValueError)
    add(L + "bowls no shape", lambda s: s.rt.bowls(s.dev(s.ints((R, Cc)))), raises=ValueError)
    add(L + "bowls buffer small", lambda s: s.rt.bowls(s.dev(s.ints((R, Cc))), shape=(R, Cc + 1)), raises=ValueError)
    add(L + "bowls outlets shape", lambda s: s.rt.bowls(s.ints((R, Cc)), outlets=s.ints((R + 1, Cc))), raises=ValueError)
    add(L + "bowls outlet buffer small", lambda s: s.rt.bowls(s.dev(s.ints((R, Cc))), shape=(R, Cc), outlets=s.empty(R * Cc - 1)), raises=ValueError)
    add(L + "bowls weights", lambda s: bowls(s, False, row_weights=np.ones(R)), raises=ValueError)


# ---- writing it down --------------------------------------------------------------------------------------------------
def describe(x, fake, rmod, depth=0):
    """What a method returned, as text: arrays by dtype, shape and CRC32, objects by their attributes."""
    if isinstance(x, np.ndarray):
        return f"array {x.dtype.str if x.dtype.names is None else x.dtype.descr} {x.shape} crc {zlib.crc32(np.ascontiguousarray(x).tobytes()):08x}"
    if isinstance(x, rmod.DeviceBuffer):
        import ctypes as C
        return f"DeviceBuffer {fake.where(x.ptr)} {x.nbytes} crc {zlib.crc32(C.string_at(x.ptr, x.nbytes)):08x}"
    if isinstance(x, (tuple, list)):
        return "[" + ", ".join(describe(v, fake, rmod, depth + 1) for v in x) + "]"
    if isinstance(x, dict):
        return "{" + ", ".join(f"{k}: {describe(v, fake, rmod, depth + 1)}" for k, v in sorted(x.items())) + "}"
    if hasattr(x, "__dict__") and depth < 3:
        return type(x).__name__ + describe({k: v for k, v in vars(x).items()}, fake, rmod, depth + 1)
    if isinstance(x, (np.integer, np.floating, np.bool_)):
        x = x.item()
    return repr(x) if isinstance(x, (int, float, str, bool, type(None))) else type(x).__name__


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("out", help="the file to write")
    ap.add_argument("--tree", help="the checkout whose moonrtx_amd to trace instead of this tree's")
    args = ap.parse_args()
    sys.path[:0] = [os.path.abspath(args.tree or ROOT), os.path.join(ROOT, "tests")]
    from fake_moonrt import FakeLib
    from moonrtx_amd import _lib
    fake = FakeLib()
    _lib.load = lambda: fake
    from moonrtx_amd import renderer as rmod

    download = rmod.DeviceBuffer.download

    def logged_download(self, dtype, shape):
        fake.log.append(("download as", np.dtype(dtype).str if np.dtype(dtype).names is None else "record", tuple(int(v) for v in np.atleast_1d(shape))))
        return download(self, dtype, shape)
    rmod.DeviceBuffer.download = logged_download

    terrain()
    lattice()
    lines, n_calls = [], 0
    for name, run, script, refuse, raises in SCENARIOS:
        fake.reset()
        s = Scene(rmod, fake)
        fake.script, fake.refuse = dict(script), set(refuse)
        lines.append(f"== {name}")
        try:
            end = "returns " + describe(run(s), fake, rmod)
            failed = None
        except Exception as e:                      # whatever the method raised is part of the record
            end, failed = f"raises {type(e).__name__}: {e}", e
        want = getattr(raises, "__name__", raises)
        if (type(failed).__name__ if failed is not None else None) != want:
            raise SystemExit(f"scenario {name!r}: expected {want or 'a result'}, got {end}") from failed
        # the record ends where the method ended: what it left allocated is written down, and neither the scenario's own
        # buffers nor what the garbage collector frees once the exception is dropped belong to it
        mark, own = len(fake.log), {fake.where(b.ptr) for b in s.bufs if b.ptr}
        left = [k for k in fake.live() if f"dev{k}+0" not in own]
        failed = None
        for b in s.bufs:
            b.free()
        del fake.log[mark:]
        for e in fake.log:
            lines.append(json.dumps(e, default=str))
        n_calls += len(fake.calls())
        lines.append(end)
        lines.append("stats " + describe(s.stats, fake, rmod))
        if left:
            lines.append(f"left allocated {left}")
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"{n_calls} library calls in {len(SCENARIOS)} scenarios written to {args.out}")


if __name__ == "__main__":
    main()
