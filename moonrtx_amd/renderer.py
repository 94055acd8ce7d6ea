"""MoonRT: object wrapper over the C ABI of libmoonrt.so (include/moonrt.h).

One instance == one `mrtx_ctx` == what the reference holds in `self.rt` (moon_renderer.py:571-575),
minus the Tk window.  The PlotOptiX-named surface (set_data / set_displacement / setup_camera / ...)
lives in moonrtx_amd/tkoptix.py and is a thin adapter over this class.
"""
import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import MrtxConfig, MrtxParams, MrtxPowerModel, MrtxStats, vec3


class MoonRTError(RuntimeError):
    pass


class DeviceBuffer:
    """A raw device allocation owned by the host side (inputs built on the GPU: synthetic DEMs...)."""

    def __init__(self, nbytes, device=0):
        self._lib = _lib.load()
        self.device = int(device)
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        rc = self._lib.mrtx_dev_alloc(self.device, self.nbytes, C.byref(p))
        if rc != 0 or not p.value:
            raise MoonRTError(f"device allocation of {self.nbytes} bytes failed (code {rc})")
        self.ptr = p.value

    def download(self, dtype, shape):
        out = np.empty(shape, dtype)
        if out.nbytes > self.nbytes:
            raise ValueError("download larger than the buffer")
        rc = self._lib.mrtx_dev_download(self.device, out.ctypes.data, self.ptr, out.nbytes)
        if rc != 0:
            raise MoonRTError(f"device download failed (code {rc})")
        return out

    def upload(self, array, offset=0):
        a = np.ascontiguousarray(array)
        if offset < 0 or offset + a.nbytes > self.nbytes:
            raise ValueError("upload outside the buffer")
        rc = self._lib.mrtx_dev_upload(self.device, self.ptr + int(offset), a.ctypes.data, a.nbytes)
        if rc != 0:
            raise MoonRTError(f"device upload failed (code {rc})")

    def free(self):
        if self.ptr:
            self._lib.mrtx_dev_free(self.device, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class MoonRT:
    def __init__(self, width, height, device=0, rank=0, world=1, tile=(0, 0)):
        """`tile` = (0, 0): the library's default sharding / culling tile (16 x 16 on one or two GPUs, 32 x 32 from four ranks up)."""
        self._lib = _lib.load()
        self.width, self.height = int(width), int(height)
        self.rank, self.world = int(rank), int(world)
        cfg = MrtxConfig(int(device), self.width, self.height, self.rank, self.world, int(tile[0]), int(tile[1]))
        ctx = C.c_void_p()
        rc = self._lib.mrtx_create(C.byref(cfg), C.byref(ctx))
        self._ctx = ctx
        if rc != 0:
            msg = self._lib.mrtx_last_error(ctx).decode() if ctx.value else "invalid configuration"
            if ctx.value:
                self._lib.mrtx_destroy(ctx)
            self._ctx = None
            raise MoonRTError(f"mrtx_create failed ({rc}): {msg}")
        self.params = MrtxParams()
        self._lib.mrtx_default_params(C.byref(self.params))
        self._keepalive = {}
        import os
        if os.environ.get("MOONRT_DEFAULT_FLAGS"):      # test / debugging aid: e.g. 1 = maintain the sample counters
            self.set_params(flags=int(os.environ["MOONRT_DEFAULT_FLAGS"]))

    # ---- plumbing
    def _check(self, rc, what):
        if rc != 0:
            raise MoonRTError(f"{what} failed ({rc}): {self._lib.mrtx_last_error(self._ctx).decode()}")

    def close(self):
        if self._ctx is not None:
            self._lib.mrtx_destroy(self._ctx)
            self._ctx = None
            self._keepalive.clear()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- resources
    def upload_dem(self, elevation):
        a = np.ascontiguousarray(elevation, np.float32)
        if a.ndim != 2:
            raise ValueError("elevation must be a 2-D float32 array")
        self._check(self._lib.mrtx_upload_dem(self._ctx, a.ctypes.data, a.shape[0], a.shape[1]), "mrtx_upload_dem")
        self._keepalive.pop("dem", None)
        self._dem_shape = (int(a.shape[0]), int(a.shape[1]))

    def bind_dem(self, buf, h, w):
        """Ingest a device-resident float32 (h, w) DEM; the context makes its own row-pair copy (8 B per texel)."""
        self._check(self._lib.mrtx_bind_dem_device(self._ctx, buf.ptr, h, w), "mrtx_bind_dem_device")
        self._dem_shape = (int(h), int(w))

    def upload_color(self, rgba):
        if rgba is None:
            self._check(self._lib.mrtx_upload_color(self._ctx, None, 0, 0), "mrtx_upload_color")
            self._color_shape = None
            return
        a = np.ascontiguousarray(rgba, np.uint8)
        if a.ndim != 3 or a.shape[2] != 4:
            raise ValueError("colour texture must be (h, w, 4) uint8")
        self._check(self._lib.mrtx_upload_color(self._ctx, a.ctypes.data, a.shape[0], a.shape[1]), "mrtx_upload_color")
        self._keepalive.pop("color", None)
        self._color_shape = (int(a.shape[0]), int(a.shape[1]))

    def bind_color(self, buf, h, w):
        self._check(self._lib.mrtx_bind_color_device(self._ctx, buf.ptr if buf else None, h, w), "mrtx_bind_color_device")
        self._color_shape = (int(h), int(w)) if buf else None

    def upload_background(self, rgba):
        if rgba is None:
            self._check(self._lib.mrtx_upload_background(self._ctx, None, 0, 0), "mrtx_upload_background")
            return
        a = np.ascontiguousarray(rgba, np.uint8)
        if a.ndim != 3 or a.shape[2] != 4:
            raise ValueError("background must be (h, w, 4) uint8")
        self._check(self._lib.mrtx_upload_background(self._ctx, a.ctypes.data, a.shape[0], a.shape[1]),
                    "mrtx_upload_background")

    def upload_overlay(self, rgba):
        """Frame-sized RGBA8 texture composited over the tone-mapped image (the "Overlay" post-process); None removes it."""
        if rgba is None:
            self._check(self._lib.mrtx_upload_overlay(self._ctx, None, 0, 0), "mrtx_upload_overlay")
            return
        a = np.ascontiguousarray(rgba, np.uint8)
        if a.shape != (self.height, self.width, 4):
            raise ValueError("the overlay must be (height, width, 4) uint8")
        self._check(self._lib.mrtx_upload_overlay(self._ctx, a.ctypes.data, a.shape[0], a.shape[1]), "mrtx_upload_overlay")

    # ---- scene state
    def set_params(self, **kw):
        for k, v in kw.items():
            if k == "const_albedo":
                self.params.const_albedo = (C.c_float * 3)(*[float(t) for t in v])
            elif hasattr(self.params, k):
                setattr(self.params, k, v)
            else:
                raise KeyError(f"unknown renderer parameter {k!r}")
        self._check(self._lib.mrtx_set_params(self._ctx, C.byref(self.params)), "mrtx_set_params")

    def set_camera(self, eye, target, up, vfov_deg):
        self._check(self._lib.mrtx_set_camera(self._ctx, vec3(eye), vec3(target), vec3(up), float(vfov_deg)),
                    "mrtx_set_camera")

    def set_moon_frame(self, center, radius, u, v):
        self._check(self._lib.mrtx_set_moon_frame(self._ctx, vec3(center), float(radius), vec3(u), vec3(v)),
                    "mrtx_set_moon_frame")

    def set_light(self, pos, radius, radiance):
        self._check(self._lib.mrtx_set_light(self._ctx, vec3(pos), float(radius), float(radiance)), "mrtx_set_light")

    def set_sun_disk(self, pos, radius, radiance):
        self._check(self._lib.mrtx_set_sun_disk(self._ctx, vec3(pos), float(radius), float(radiance)),
                    "mrtx_set_sun_disk")

    def set_capsules(self, capsules):
        """Overlay tubes: (n, 12) float32 (see moonrtx_amd.overlays.graph_to_capsules); None / empty removes them."""
        if capsules is None or len(capsules) == 0:
            self._check(self._lib.mrtx_set_capsules(self._ctx, None, 0), "mrtx_set_capsules")
            return
        a = np.ascontiguousarray(capsules, np.float32).reshape(-1, 12)
        self._check(self._lib.mrtx_set_capsules(self._ctx, a.ctypes.data, a.shape[0]), "mrtx_set_capsules")

    def apply_scene(self, s):
        """Push a moonrtx_amd.scene.SceneDesc (everything except textures)."""
        self.set_params(scene_epsilon=s.scene_epsilon, marching_step=s.marching_step,
                        marching_step_eps=s.marching_step_eps, tonemap_exposure=s.exposure,
                        tonemap_gamma=s.gamma, spp_per_launch=s.spp_per_launch, max_spp=s.max_spp,
                        seed=s.seed, const_albedo=s.const_albedo, path_seg_min=s.path_seg_min,
                        path_seg_max=s.path_seg_max)
        self.set_camera(s.eye, s.target, s.up, s.vfov_deg)
        self.set_moon_frame(s.center, s.radius, s.u, s.v)
        self.set_light(s.light_pos, s.light_radius, s.light_radiance)
        self.set_sun_disk(s.sun_pos, s.sun_radius, s.sun_radiance)

    # ---- rendering
    def reset(self):
        self._check(self._lib.mrtx_reset_accum(self._ctx), "mrtx_reset_accum")

    def render(self, n_blocks=1):
        st = MrtxStats()
        self._check(self._lib.mrtx_render(self._ctx, int(n_blocks), C.byref(st)), "mrtx_render")
        return {name: getattr(st, name) for name, _ in MrtxStats._fields_ if name != "reserved"}

    def render_part(self, n_blocks, part, n_parts):
        """One part of the tile list (mrtx_render_part): the exchange moves part k while part k+1 renders."""
        st = MrtxStats()
        self._check(self._lib.mrtx_render_part(self._ctx, int(n_blocks), int(part), int(n_parts), C.byref(st)), "mrtx_render_part")
        return {name: getattr(st, name) for name, _ in MrtxStats._fields_ if name != "reserved"}

    def samples_done(self):
        n = C.c_uint32()
        self._check(self._lib.mrtx_samples_done(self._ctx, C.byref(n)), "mrtx_samples_done")
        return n.value

    def read_linear(self):
        out = np.empty((self.height, self.width, 4), np.float32)
        self._check(self._lib.mrtx_read_linear(self._ctx, out.ctypes.data), "mrtx_read_linear")
        return out

    def read_rgba8(self, out=None):
        """The tone-mapped frame; `out` (a C-contiguous (H, W, 4) uint8 array) is reused when given."""
        if out is None:
            out = np.empty((self.height, self.width, 4), np.uint8)
        elif out.shape != (self.height, self.width, 4) or out.dtype != np.uint8 or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous (height, width, 4) uint8 array")
        self._check(self._lib.mrtx_read_rgba8(self._ctx, out.ctypes.data), "mrtx_read_rgba8")
        return out

    def read_rgb16(self):
        """The tone-mapped frame at 16 bits per sample, (H, W, 3) uint16 -- save_image(bps="Bps16")."""
        out = np.empty((self.height, self.width, 3), np.uint16)
        self._check(self._lib.mrtx_read_rgb16(self._ctx, out.ctypes.data), "mrtx_read_rgb16")
        return out

    def read_hit(self, x, y):
        """One texel of the hit buffer: (hx, hy, hz, hd), hd <= 0 == miss."""
        out = (C.c_float * 4)()
        self._check(self._lib.mrtx_read_hit(self._ctx, int(x), int(y), out), "mrtx_read_hit")
        return float(out[0]), float(out[1]), float(out[2]), float(out[3])

    def read_hits(self):
        out = np.empty((self.height, self.width, 4), np.float32)
        self._check(self._lib.mrtx_read_hits(self._ctx, out.ctypes.data), "mrtx_read_hits")
        return out

    # ---- Sun illumination of the terrain
    @staticmethod
    def sun_samples(n):
        """The (u2, u3) float32 table of n Sun samples the illumination stage uses, (n, 2)."""
        out = np.empty((int(n), 2), np.float32)
        if _lib.load().mrtx_illum_sun_samples(int(n), out.ctypes.data) != 0:
            raise ValueError("n_sun must be 1, 2, 4, ..., 64")
        return out

    @staticmethod
    def grid_nodes(lat=(90.0, -90.0), lon=(-180.0, 180.0), shape=(180, 360)):
        """float64 (lat, lon) in degrees of the nodes of a map, the centres of its cells, computed as the library computes
        them -- a point list at these coordinates gives the map's values bit for bit."""
        (la_n, la_s), (lo_w, lo_e), (h, w) = (float(lat[0]), float(lat[1])), (float(lon[0]), float(lon[1])), shape
        dlat, dlon = (la_n - la_s) / h, (lo_e - lo_w) / w
        return la_n - (np.arange(h) + 0.5) * dlat, lo_w + (np.arange(w) + 0.5) * dlon

    def illumination_map(self, lat=(90.0, -90.0), lon=(-180.0, 180.0), shape=(180, 360), n_sun=16, rows=None, stats=None,
                         band_bytes=256 << 20):
        """(rows, w, 4) float32 map of (lit, irr, mu, D) over lat = (north, south), lon = (west, east) in degrees with
        shape = (h, w) cells; rows = (first, end) computes that band only (default: all).  Bands of at most band_bytes go
        through one device buffer.  `stats`, if a dict, receives the summed counters of the launches."""
        h, w = int(shape[0]), int(shape[1])
        r0, r1 = (0, h) if rows is None else (int(rows[0]), int(rows[1]))
        g = _lib.MrtxIllumGrid(float(lat[0]), float(lat[1]), float(lon[0]), float(lon[1]), h, w, r0, r1, int(n_sun), 0)
        return self._band_map("mrtx_illum_grid", g, np.empty((max(r1 - r0, 0), w, 4), np.float32), 16, band_bytes, stats)

    def _band_map(self, name, g, out, node_bytes, band_bytes, stats):
        """Rows [g.row_begin, g.row_end) of a map of node_bytes per node into `out` through the grid call `name`: in one call
        straight into `out` when they fit in band_bytes, else in bands of that size through one device buffer."""
        r0, r1, w = g.row_begin, g.row_end, g.w
        step = max(1, int(band_bytes) // (node_bytes * max(w, 1)))
        call = getattr(self._lib, name)
        if r1 - r0 <= step:      # one band: straight into the host array
            st = MrtxStats()
            self._check(call(self._ctx, C.byref(g), None, out.ctypes.data, C.byref(st)), name)
            self._add_stats(stats, st)
            return out
        buf = DeviceBuffer(node_bytes * step * w, self.config()["device"])
        try:
            for a in range(r0, r1, step):
                g.row_begin, g.row_end = a, min(a + step, r1)
                st = MrtxStats()
                self._check(call(self._ctx, C.byref(g), buf.ptr, None, C.byref(st)), name)
                self._add_stats(stats, st)
                out[a - r0:g.row_end - r0] = buf.download(np.float32, (g.row_end - a,) + out.shape[1:])
        finally:
            buf.free()
        return out

    def illumination_at(self, lat_deg, lon_deg, n_sun=16, stats=None):
        """(N, 4) float32 (lit, irr, mu, D) at N selenographic points (degrees): the status bar's Sun altitude
        (renderer_status.py:121-157) on the real terrain."""
        la = np.atleast_1d(np.asarray(lat_deg, np.float64)).ravel()
        lo = np.atleast_1d(np.asarray(lon_deg, np.float64)).ravel()
        if la.shape != lo.shape:
            raise ValueError("lat_deg and lon_deg must have the same number of points")
        pts = np.ascontiguousarray(np.stack([la, lo], -1))
        out = np.empty((la.size, 4), np.float32)
        st = MrtxStats()
        self._check(self._lib.mrtx_illum_points(self._ctx, pts.ctypes.data, la.size, int(n_sun), out.ctypes.data, C.byref(st)),
                    "mrtx_illum_points")
        self._add_stats(stats, st)
        return out

    def illumination_series(self, lat_deg, lon_deg, epochs, n_sun=16, first=None, count=None, stats=None, chunk_bytes=256 << 20):
        """(N, count, 4) float32 (lit, irr, mu, D) at N points over many dates: entry (p, j) is what
        illumination_at gives at point p after the light and Moon frame of epoch first[p] + j were set, bit for bit.
        `epochs`: the (m, 14) float64 array of ephemeris.sun_epochs, or a sequence of SceneDesc.  first = None: every point
        reads epochs [0, count) (count defaults to m); otherwise N window starts and count is required.  Calls hold at most
        chunk_bytes of output each (points split between calls); `stats`, if a dict, receives the summed counters."""
        la, lo = self._points(lat_deg, lon_deg)
        ep = self._epochs(epochs)
        if first is None:
            count = ep.shape[0] if count is None else int(count)
        else:
            if count is None:
                raise ValueError("count is required with first")
            first = np.ascontiguousarray(np.atleast_1d(np.asarray(first)).ravel(), np.int32)
            if first.shape != la.shape:
                raise ValueError("first must hold one window start per point")
            count = int(count)
        pts = np.ascontiguousarray(np.stack([la, lo], -1))
        out = np.empty((la.size, max(count, 0), 4), np.float32)
        for a, b in self._chunks(la.size, max(count, 1), chunk_bytes, 16, empty_call=False):
            st = MrtxStats()
            fp = None if first is None else first[a:].ctypes.data
            self._check(self._lib.mrtx_illum_series(self._ctx, pts[a:].ctypes.data, b - a, ep.ctypes.data, ep.shape[0], fp, count,
                                                    int(n_sun), None, out[a:].ctypes.data, C.byref(st)), "mrtx_illum_series")
            self._add_stats(stats, st)
        return out

    @staticmethod
    def _points(lat_deg, lon_deg):
        la = np.atleast_1d(np.asarray(lat_deg, np.float64)).ravel()
        lo = np.atleast_1d(np.asarray(lon_deg, np.float64)).ravel()
        if la.shape != lo.shape:
            raise ValueError("lat_deg and lon_deg must have the same number of points")
        return la, lo

    @staticmethod
    def _epochs(epochs):
        from .ephemeris import epoch_of_scene
        if not isinstance(epochs, np.ndarray):
            epochs = np.array([epoch_of_scene(e) for e in epochs], np.float64).reshape(-1, 14)
        ep = np.ascontiguousarray(epochs, np.float64)
        if ep.ndim != 2 or ep.shape[1] != 14:
            raise ValueError("epochs must be an (m, 14) array (ephemeris.sun_epochs) or a sequence of SceneDesc")
        return ep

    @staticmethod
    def horizon_azimuths(n_az):
        """Azimuths of the n_az horizon samples, degrees from north through east: a * 360 / n_az."""
        n = int(n_az)
        if n < 4 or n > 4096 or n & (n - 1):
            raise ValueError(f"n_az must be 4, 8, ..., 4096 (got {n_az})")
        return np.arange(n, dtype=np.float64) * (360.0 / n)

    def horizon(self, lat_deg, lon_deg, n_az=256, n_bis=14, stats=None, out=None, chunk_bytes=256 << 20, height_m=None,
                radius_m=1737400.0):
        """(N, n_az) float32: the terrain's horizon elevation, degrees, seen from N points (degrees) at horizon_azimuths(n_az),
        found by n_bis bisection probes that are each an illumination sample's visibility decision.
        out = a DeviceBuffer of at least N * n_az * 4 bytes: the horizons are written there (point-major) and `out` is
        returned.  Calls hold at most chunk_bytes of output each (points split between calls); `stats`, if a dict, receives
        the summed counters.  height_m (one value, or one per point, metres in [0, 1e4]): the horizon seen from a mast top that
        high above each point, line_of_sight's raised end (section 3.15; radius_m = the metres of D = 1); a height of 0 gives
        the ground's horizon bit for bit, None makes the ground-only call."""
        la, lo = self._points(lat_deg, lon_deg)
        n_az = int(n_az)
        pts = np.ascontiguousarray(np.stack([la, lo], -1))
        hts = None
        if height_m is not None:
            hts = np.asarray(height_m, np.float64)
            if hts.ndim == 0:
                hts = np.full(la.size, float(hts))
            hts = np.ascontiguousarray(hts.ravel())
            if hts.size != la.size:
                raise ValueError("height_m must be one height or one per point")
        if out is not None and out.nbytes < la.size * max(n_az, 0) * 4:
            raise ValueError("the device buffer is smaller than N x n_az float32")
        host = np.empty((la.size, max(n_az, 0)), np.float32) if out is None else None
        for a, b in self._chunks(la.size, max(n_az, 1), chunk_bytes):
            st = MrtxStats()
            dev = None if out is None else out.ptr + a * n_az * 4
            hp = None if out is not None else host[a:].ctypes.data
            if hts is None:
                self._check(self._lib.mrtx_horizon_points(self._ctx, pts[a:].ctypes.data, b - a, n_az, int(n_bis), dev, hp,
                                                          C.byref(st)), "mrtx_horizon_points")
            else:
                self._check(self._lib.mrtx_horizon_raised(self._ctx, pts[a:].ctypes.data, hts[a:].ctypes.data, float(radius_m),
                                                          b - a, n_az, int(n_bis), dev, hp, C.byref(st)), "mrtx_horizon_raised")
            self._add_stats(stats, st)
        return out if out is not None else host

    WINDOW_COLUMNS = ("share_a", "longest_out_a", "share_b", "longest_out_b", "share_both", "longest_both", "first_both",
                      "longest_out_both")

    def horizon_windows(self, lat_deg, lon_deg, horizon, epochs_a, epochs_b, min_a=0.5, min_b=1.0, n_az=None, stats=None,
                        chunk_bytes=256 << 20):
        """Two bodies against the horizons of `horizon`, reduced per point on the device: with f_a,
        f_b horizon_sun's fractions for the epoch tables epochs_a, epochs_b (the same m dates), ok_a = f_a >= min_a,
        ok_b = f_b >= min_b and both = ok_a and ok_b, the (N, 8) float32 columns WINDOW_COLUMNS: the share of epochs with ok_a
        and the longest run of epochs without it, the same for b, the share with both, the longest run with both and the index
        of its first epoch (the earliest such run; -1 if there is none), the longest run without both.  Runs are in epochs.
        `horizon` as for horizon_sun.  No (N, m) table exists anywhere; calls hold at most chunk_bytes of horizons and
        output."""
        la, lo = self._points(lat_deg, lon_deg)
        ea, eb = self._epochs(epochs_a), self._epochs(epochs_b)
        if ea.shape != eb.shape:
            raise ValueError("epochs_a and epochs_b must hold the same number of epochs")
        m = ea.shape[0]
        n_az, hz_at = self._horizon_arg(horizon, la.size, n_az)
        pts = np.ascontiguousarray(np.stack([la, lo], -1))
        res = np.empty((la.size, 8), np.float32)
        for a, b in self._chunks(la.size, max(int(n_az), 0) + 8, chunk_bytes):
            st = MrtxStats()
            dh, hh = hz_at(a)
            self._check(self._lib.mrtx_horizon_windows(self._ctx, pts[a:].ctypes.data, b - a, n_az, dh, hh, ea.ctypes.data,
                                                       eb.ctypes.data, m, float(min_a), float(min_b), None,
                                                       res[a:].ctypes.data, C.byref(st)), "mrtx_horizon_windows")
            self._add_stats(stats, st)
        return res

    def horizon_mask(self, lat_deg, lon_deg, horizon, epochs_a, epochs_b=None, min_a=0.5, min_b=1.0, n_az=None, out=None,
                     stats=None, chunk_bytes=256 << 20, out_offset=0):
        """horizon_windows' joint predicate kept as bits (mrtx_horizon_mask): an (N, W64) uint64
        array, W64 = (m + 63) // 64, in which bit k & 63 of word k >> 6 of row p says that at epoch k point p has
        f_a >= min_a and f_b >= min_b (f = horizon_sun's fractions; equality counts as met).  epochs_b = None: ok_a alone.
        The bits past epoch m - 1 are 0.  out = a DeviceBuffer: the words are written there from byte out_offset (a multiple
        of 8) on, point-major, and `out` is returned.  `horizon` as for horizon_sun; calls hold at most chunk_bytes of
        horizons and output.  moonrtx_amd.traverse.unpack_mask turns rows into booleans."""
        la, lo = self._points(lat_deg, lon_deg)
        ea = self._epochs(epochs_a)
        eb = None if epochs_b is None else self._epochs(epochs_b)
        if eb is not None and ea.shape != eb.shape:
            raise ValueError("epochs_a and epochs_b must hold the same number of epochs")
        m = ea.shape[0]
        w64 = (m + 63) // 64
        n_az, hz_at = self._horizon_arg(horizon, la.size, n_az)
        pts = np.ascontiguousarray(np.stack([la, lo], -1))
        out_offset = int(out_offset)
        if out is not None and (out_offset < 0 or out_offset % 8 or out.nbytes < out_offset + la.size * w64 * 8):
            raise ValueError("the device buffer is smaller than N x W64 uint64 from out_offset (a multiple of 8) on")
        res = np.empty((la.size, w64), np.uint64) if out is None else None
        for a, b in self._chunks(la.size, max(int(n_az), 0) + 2 * max(w64, 1), chunk_bytes):
            st = MrtxStats()
            dh, hh = hz_at(a)
            dev = None if out is None else out.ptr + out_offset + a * w64 * 8
            hp = None if out is not None else res[a:].ctypes.data
            self._check(self._lib.mrtx_horizon_mask(self._ctx, pts[a:].ctypes.data, b - a, n_az, dh, hh, ea.ctypes.data,
                                                    None if eb is None else eb.ctypes.data, m, float(min_a), float(min_b),
                                                    dev, hp, C.byref(st)), "mrtx_horizon_mask")
            self._add_stats(stats, st)
        return out if out is not None else res

    POWER_COLUMNS = ("generated", "net", "storage_need", "drawdown_first", "drawdown_last", "min_charge", "epochs_unmet",
                     "energy_unmet")
    PANELS = {"track": _lib.PANEL_TRACK, "fixed": _lib.PANEL_FIXED, "azimuth": _lib.PANEL_AZIMUTH}

    @staticmethod
    def power_scale(gen_w, load_w):
        """The largest cpw_log2 in [-20, 20] that keeps both tables, as float32 watts times 2^cpw_log2, at or below 2^28 counts
        (DESIGN.md section 3.17); ValueError if even 2^-20 counts per watt does not."""
        top = max(float(np.max(np.asarray(gen_w, np.float64).astype(np.float32), initial=0.0)),
                  float(np.max(np.asarray(load_w, np.float64).astype(np.float32), initial=0.0)))
        if not top > 0.0:
            return 20
        if not math.isfinite(top):
            raise ValueError("gen_w and load_w must be finite")
        mant, exp = math.frexp(top)             # top = mant * 2^exp, mant in [0.5, 1)
        e = (29 if mant == 0.5 else 28) - exp
        if e < -20:
            raise ValueError("gen_w or load_w exceeds 2^28 counts at 2^-20 counts per watt")
        return min(e, 20)

    def power_budget(self, lat_deg, lon_deg, horizon, epochs, gen_w, load_w, panel="track", normal_enu=None, cpw_log2=None,
                     capacity=0, initial=None, mode="summary", n_az=None, stats=None, chunk_bytes=256 << 20):
        """The energy balance of a solar-powered asset at N points against the horizons of `horizon`, in integer counts of
        2^-cpw_log2 W x the epoch spacing.  gen_w[k]: the watts the array delivers facing the whole
        Sun at epoch k; load_w[k]: the watts drawn (one value or one per epoch).  panel: "track" (two-axis), "fixed" (normal
        normal_enu in each point's east, north, up) or "azimuth" (a vertical panel turned toward the Sun).  capacity and
        initial are counts (initial=None: full); cpw_log2=None picks power_scale's.  mode "summary": (N, 8) int64 columns
        POWER_COLUMNS -- the generated and the net energy, the least capacity that starting full never empties, the first and
        last epoch of that drawdown (-1: none), the lowest state of charge, the epochs whose load was not met and the energy
        not delivered; mode "full": (N, m) int32 generated counts G_k.  `horizon` as for horizon_sun; SUMMARY forms no (N, m)
        table anywhere."""
        la, lo = self._points(lat_deg, lon_deg)
        ep = self._epochs(epochs)
        m = ep.shape[0]
        gen = np.ascontiguousarray(np.broadcast_to(np.asarray(gen_w, np.float64), (m,)))
        load = np.ascontiguousarray(np.broadcast_to(np.asarray(load_w, np.float64), (m,)))
        if mode not in ("summary", "full"):
            raise ValueError(f"mode must be 'summary' or 'full' (got {mode!r})")
        if panel not in self.PANELS:
            raise ValueError(f"panel must be one of {sorted(self.PANELS)} (got {panel!r})")
        if (panel == "fixed") != (normal_enu is not None):
            raise ValueError("normal_enu goes with panel='fixed', and only with it")
        md = MrtxPowerModel()
        md.panel = self.PANELS[panel]
        md.normal_enu[:] = [float(x) for x in (normal_enu if normal_enu is not None else (0.0, 0.0, 1.0))]
        md.cpw_log2 = self.power_scale(gen, load) if cpw_log2 is None else int(cpw_log2)
        md.capacity = int(capacity)
        md.initial = int(capacity) if initial is None else int(initial)
        n_az, hz_at = self._horizon_arg(horizon, la.size, n_az)
        pts = np.ascontiguousarray(np.stack([la, lo], -1))
        full = mode == "full"
        res = np.empty((la.size, m), np.int32) if full else np.empty((la.size, 8), np.int64)
        for a, b in self._chunks(la.size, max(m, 1) if full else max(int(n_az), 0) + 16, chunk_bytes):
            st = MrtxStats()
            dh, hh = hz_at(a)
            self._check(self._lib.mrtx_power_budget(self._ctx, pts[a:].ctypes.data, b - a, n_az, dh, hh, ep.ctypes.data,
                                                    gen.ctypes.data, load.ctypes.data, m, C.byref(md), 0 if full else 1, None,
                                                    res[a:].ctypes.data, C.byref(st)), "mrtx_power_budget")
            self._add_stats(stats, st)
        return res

    def horizon_sun(self, lat_deg, lon_deg, horizon, epochs, summary=False, stats=None, n_az=None, chunk_bytes=256 << 20):
        """The Sun against the horizons of `horizon`: per (point, epoch) the fraction of the light's
        disc above the point's horizon.  `horizon`: the (N, n_az) array of MoonRT.horizon, or a DeviceBuffer holding it
        (then n_az is required); `epochs` as for illumination_series.  summary=False: (N, m) float32 fractions;
        summary=True: (N, 4) float32 (mean fraction, share of epochs with any of the disc up, share with all of it up,
        longest run of consecutive epochs with none of it up, in epochs).  FULL calls hold at most chunk_bytes of output."""
        la, lo = self._points(lat_deg, lon_deg)
        ep = self._epochs(epochs)
        m = ep.shape[0]
        n_az, hz_at = self._horizon_arg(horizon, la.size, n_az)
        pts = np.ascontiguousarray(np.stack([la, lo], -1))
        width = 4 if summary else m
        res = np.empty((la.size, width), np.float32)
        for a, b in self._chunks(la.size, None if summary else max(m, 1), chunk_bytes):
            st = MrtxStats()
            dh, hh = hz_at(a)
            self._check(self._lib.mrtx_horizon_sun(self._ctx, pts[a:].ctypes.data, b - a, n_az, dh, hh, ep.ctypes.data, m,
                                                   1 if summary else 0, None, res[a:].ctypes.data, C.byref(st)),
                        "mrtx_horizon_sun")
            self._add_stats(stats, st)
        return res

    OCCULTATION_COLUMNS = ("mean", "min", "share_partial", "share_total", "longest_partial", "first_partial", "longest_total",
                           "eclipses")

    def occultation(self, lat_deg, lon_deg, source_epochs, body_epochs, summary=False, stats=None, chunk_bytes=256 << 20):
        """The Earth's occultation of the Sun: per (point, epoch) the share g of the source's disc
        that the body's disc leaves uncovered, seen from the point's vertex.  source_epochs: ephemeris.far_sun_epochs (the Sun
        at its true distance); body_epochs: ephemeris.earth_epochs, for the same m dates.  summary=False: (N, m) float32 g;
        summary=True: the (N, 8) float32 columns OCCULTATION_COLUMNS -- the mean and the least g, the shares of epochs with
        g < 1 and with g == 0, the longest run of epochs with g < 1 and its first epoch (the earliest such run; -1 if none),
        the longest run with g == 0, and the number of separate runs of g < 1 (the eclipses the point saw) -- with no (N, m)
        table anywhere.  The geometric discs only: no atmosphere.  FULL calls hold at most chunk_bytes of output."""
        la, lo = self._points(lat_deg, lon_deg)
        es, eb = self._epochs(source_epochs), self._epochs(body_epochs)
        if es.shape != eb.shape:
            raise ValueError("source_epochs and body_epochs must hold the same number of epochs")
        m = es.shape[0]
        pts = np.ascontiguousarray(np.stack([la, lo], -1))
        res = np.empty((la.size, 8 if summary else m), np.float32)
        for a, b in self._chunks(la.size, None if summary else max(m, 1), chunk_bytes):
            st = MrtxStats()
            self._check(self._lib.mrtx_occultation(self._ctx, pts[a:].ctypes.data, b - a, es.ctypes.data, eb.ctypes.data, m,
                                                   1 if summary else 0, None, res[a:].ctypes.data, C.byref(st)),
                        "mrtx_occultation")
            self._add_stats(stats, st)
        return res

    PASS_COLUMNS = _lib.PASS_COLUMNS
    PASS_MODES = {"full": _lib.PASSES_FULL, "summary": _lib.PASSES_SUMMARY, "list": _lib.PASSES_LIST}

    def horizon_passes(self, lat_deg, lon_deg, horizon, positions_m, *, height_m=None, min_elev_deg=0.0, mode="summary",
                       n_az=None, radius_m=1737400.0, stats=None, chunk_bytes=256 << 20):
        """Relay orbiters against the horizons of `horizon` (mrtx_horizon_passes).  positions_m:
        (S, m, 3) or (m, 3) float64 metres in the Moon-fixed frame (orbits.fixed_from_latlon's axes), S <= 256 satellites at the
        same m epochs.  A satellite is in view where its margin g = es - max(horizon at its azimuth, min_elev_deg) is > 0; the
        direction is taken from the mast top height_m above each point (one value or one per point; None: the ground, the same
        bits as 0).  mode "full": (N, S, m, 4) float32 (elevation deg, azimuth deg in [0, 360), range m, g), the antenna
        pointing table; "summary": the (N, 8) float32 columns PASS_COLUMNS -- the share of epochs with a satellite in view, the
        longest outage and the longest contact in epochs, that contact's first epoch (-1: none), the number of contacts, the
        highest elevation in view (-90: none), the mean number in view and the share with two or more -- with no (N, S, m)
        table anywhere; "list": a _lib.PASS_DTYPE array, one record per pass in ascending (point, sat, first), counted in one
        call and filled by a second.  `horizon` as for horizon_sun; calls hold at most chunk_bytes of horizons and output."""
        la, lo = self._points(lat_deg, lon_deg)
        if mode not in self.PASS_MODES:
            raise ValueError(f"mode must be one of {sorted(self.PASS_MODES)} (got {mode!r})")
        pos = np.asarray(positions_m, np.float64)
        if pos.ndim == 2:
            pos = pos[None]
        if pos.ndim != 3 or pos.shape[2] != 3:
            raise ValueError("positions_m must be (S, m, 3) or (m, 3)")
        pos = np.ascontiguousarray(pos)
        S, m = int(pos.shape[0]), int(pos.shape[1])
        hts = None
        if height_m is not None:
            hts = np.ascontiguousarray(np.broadcast_to(np.asarray(height_m, np.float64).ravel(), (la.size,)))
        n_az, hz_at = self._horizon_arg(horizon, la.size, n_az)
        pts = np.ascontiguousarray(np.stack([la, lo], -1))
        k = _lib.MrtxPasses(S, m, self.PASS_MODES[mode], 0, float(radius_m), float(min_elev_deg))
        per = max(S * m, 1)
        if mode == "full":
            res = np.empty((la.size, S, m, 4), np.float32)
            step = max(1, min(int(chunk_bytes) // (16 * per), (1 << 27) // per))
        elif mode == "summary":
            res = np.empty((la.size, 8), np.float32)
            step = max(1, int(chunk_bytes) // (4 * (max(int(n_az), 0) + 8)))
        else:
            res = []
            step = max(1, min(int(chunk_bytes) // (4 * max(int(n_az), 0) + 12 * S), (1 << 27) // max(S, 1)))
        total = C.c_uint64(0)
        for a in range(0, max(la.size, 1), step):
            b = min(a + step, la.size)
            dh, hh = hz_at(a)
            hp = None if hts is None else hts[a:].ctypes.data
            st = MrtxStats()

            def call(out_ptr, cap):
                self._check(self._lib.mrtx_horizon_passes(self._ctx, C.byref(k), pts[a:].ctypes.data, hp, b - a, n_az, dh, hh,
                                                          pos.ctypes.data, None, out_ptr, cap, C.byref(total), C.byref(st)),
                            "mrtx_horizon_passes")
                self._add_stats(stats, st)
            if mode != "list":
                call(res[a:].ctypes.data, 0)
                continue
            call(None, 0)
            if isinstance(stats, dict):
                stats["count_ms"] = stats.get("count_ms", 0.0) + st.kernel_ms
            part = np.zeros(max(int(total.value), 1), _lib.PASS_DTYPE)
            need = int(total.value)
            call(part.ctypes.data, need)
            if isinstance(stats, dict):
                stats["fill_ms"] = stats.get("fill_ms", 0.0) + st.kernel_ms
            part = part[:need]
            part["point"] += a
            res.append(part)
        return np.concatenate(res) if mode == "list" else res

    @staticmethod
    def thermal_grid(spacing_s=3600.0, spinup_lunations=None, resets=None, F=None):
        """The MrtxThermalModel of the default regolith for epochs `spacing_s` apart: the layer
        tables, n_sub steps per epoch from the stable step at F (default 0.5), spin-up blocks of one lunation.  Defaults:
        thermal.SPINUP_LUNATIONS lunations of spin-up, reset after each of the first thermal.RESETS."""
        from . import thermal
        return thermal.model(spacing_s, thermal.SPINUP_LUNATIONS if spinup_lunations is None else spinup_lunations,
                             thermal.RESETS if resets is None else resets, thermal.F_STEP if F is None else F)

    def surface_temperature(self, lat_deg, lon_deg, horizon, epochs, flux, model=None, mode="summary", stats=None, n_az=None,
                            chunk_bytes=256 << 20):
        """Regolith surface temperatures driven by the Sun against the horizons of `horizon`.
        `horizon`: the (N, n_az) array of MoonRT.horizon, or a DeviceBuffer holding it (then n_az is required); `epochs` as
        for horizon_sun, evenly spaced by model.spacing_s, the first model.n_spin of them spin-up; `flux`: the solar flux
        per epoch, W m^-2 (ephemeris.sun_flux); `model`: thermal_grid() (hourly epochs) unless given.
        mode "summary": (N, 4) float32 (max, min, mean surface temperature, mean bottom-node temperature over the recorded
        epochs); "full": (N, m - n_spin) float32 surface temperatures; "flux": (N, m) float32 absorbed flux, no stepping.
        FULL and FLUX calls hold at most chunk_bytes of output each; `stats`, if a dict, also receives newton_cap_hits."""
        modes = {"full": 0, "summary": 1, "flux": 2}
        if mode not in modes:
            raise ValueError(f"mode must be one of {sorted(modes)} (got {mode!r})")
        la, lo = self._points(lat_deg, lon_deg)
        ep = self._epochs(epochs)
        m = ep.shape[0]
        fl = np.ascontiguousarray(np.asarray(flux, np.float64).ravel())
        if fl.size != m:
            raise ValueError("flux must hold one value per epoch")
        model = self.thermal_grid() if model is None else model
        n_az, hz_at = self._horizon_arg(horizon, la.size, n_az)
        pts = np.ascontiguousarray(np.stack([la, lo], -1))
        width = {"full": max(m - int(model.n_spin), 1), "summary": 4, "flux": m}[mode]
        res = np.empty((la.size, width), np.float32)
        for a, b in self._chunks(la.size, None if mode == "summary" else width, chunk_bytes):
            st = MrtxStats()
            dh, hh = hz_at(a)
            self._check(self._lib.mrtx_thermal(self._ctx, pts[a:].ctypes.data, b - a, n_az, dh, hh, ep.ctypes.data,
                                               fl.ctypes.data, m, C.byref(model), modes[mode], None, res[a:].ctypes.data,
                                               C.byref(st)), "mrtx_thermal")
            self._add_stats(stats, st, {"newton_cap_hits": "reserved"})
        return res

    @staticmethod
    def view_samples(k):
        """The (uh1, uh2) float32 table of the k view directions of view_hits, (k, 2)."""
        out = np.empty((int(k), 2), np.float32)
        if _lib.load().mrtx_view_dir_samples(int(k), out.ctypes.data) != 0:
            raise ValueError("K must be 16, 32, ..., 1024")
        return out

    def view_hits(self, lat_deg, lon_deg, k=64, stats=None, chunk_bytes=256 << 20):
        """What terrain N points see: K fixed cosine-weighted rays per point, each marched as a path's
        continuation ray.  Returns (hits, share): (N, K, 2) float32 (lat, lon) in degrees of each ray's first terrain hit, NaN
        for sky, and (N,) float32 terrain view factors (hits / K).  Calls hold at most chunk_bytes of output each."""
        la, lo = self._points(lat_deg, lon_deg)
        k = int(k)
        pts = np.ascontiguousarray(np.stack([la, lo], -1))
        hits = np.empty((la.size, max(k, 0), 2), np.float32)
        share = np.empty(la.size, np.float32)
        width = 2 * max(k, 1) + 1
        for a, b in self._chunks(la.size, width, chunk_bytes):
            buf = np.empty((b - a) * width, np.float32) if b > a else np.empty(width, np.float32)
            st = MrtxStats()
            self._check(self._lib.mrtx_view_hits(self._ctx, pts[a:].ctypes.data, b - a, k, None, buf.ctypes.data, C.byref(st)),
                        "mrtx_view_hits")
            hits[a:b] = buf[:(b - a) * 2 * k].reshape(b - a, k, 2)
            share[a:b] = buf[(b - a) * 2 * k:(b - a) * width]
            self._add_stats(stats, st, {"bounce_rays": "bounce_rays"})
        return hits, share

    def scatter_flux(self, index, exitance, albedo_h, emissivity, n_hits=None, m=None, out=None, stats=None):
        """The gather of DESIGN.md section 3.11: (N, m) float32 Q_sec[p, e] = (1/K) sum over index[p, j] >= 0, in j order, of
        (1 - albedo_h) M_vis + emissivity M_ir of that hit at epoch e.  `index`: (N, K) int32 into the hit list, -1 for sky;
        `exitance`: the (n_hits, m, 2) float32 EXITANCE of surface_temperature_scatter, or a DeviceBuffer holding it (then
        n_hits and m are required).  out = a DeviceBuffer of at least N * m * 4 bytes: Q_sec is written there, `out` returned."""
        ix = np.ascontiguousarray(index, np.int32)
        if ix.ndim != 2:
            raise ValueError("index must be an (N, K) array")
        n, k = ix.shape
        if isinstance(exitance, DeviceBuffer):
            if n_hits is None or m is None:
                raise ValueError("n_hits and m are required with a device buffer")
            n_hits, m = int(n_hits), int(m)
            dev, host, length = exitance.ptr, None, exitance.nbytes // 4
        else:
            ex = np.ascontiguousarray(exitance, np.float32)
            if ex.ndim != 3 or ex.shape[2] != 2:
                raise ValueError("exitance must be an (n_hits, m, 2) array")
            n_hits, m = ex.shape[0], ex.shape[1]
            dev, host, length = None, ex.ctypes.data, ex.size
        if out is not None and out.nbytes < n * m * 4:
            raise ValueError("the device buffer is smaller than N x m float32")
        res = np.empty((n, m), np.float32) if out is None else None
        st = MrtxStats()
        self._check(self._lib.mrtx_scatter_flux(self._ctx, ix.ctypes.data, n, k, dev, host, length, n_hits, m, float(albedo_h),
                                                float(emissivity), None if out is None else out.ptr,
                                                None if res is None else res.ctypes.data, C.byref(st)), "mrtx_scatter_flux")
        self._add_stats(stats, st)
        return out if out is not None else res

    def surface_temperature_scatter(self, lat_deg, lon_deg, horizon, epochs, flux, model=None, mode="summary", extra_flux=None,
                                    stats=None, n_az=None, out=None):
        """surface_temperature with the additions of DESIGN.md section 3.11, in one call.  `extra_flux`: None, an (N, m)
        float32 array or a DeviceBuffer holding one, added to Q_abs in every epoch.  Modes as surface_temperature's, plus
        "exitance": (N, m - n_spin, 2) float32 (M_vis, M_ir) per recorded epoch.  out = a DeviceBuffer: the output is written
        there and `out` returned."""
        modes = {"full": 0, "summary": 1, "flux": 2, "exitance": 3}
        if mode not in modes:
            raise ValueError(f"mode must be one of {sorted(modes)} (got {mode!r})")
        la, lo = self._points(lat_deg, lon_deg)
        ep = self._epochs(epochs)
        m = ep.shape[0]
        fl = np.ascontiguousarray(np.asarray(flux, np.float64).ravel())
        if fl.size != m:
            raise ValueError("flux must hold one value per epoch")
        model = self.thermal_grid() if model is None else model
        n_az, hz_at = self._horizon_arg(horizon, la.size, n_az)
        dh, hh = hz_at(0)
        dx = hx = None
        x_len = 0
        if isinstance(extra_flux, DeviceBuffer):
            dx, x_len = extra_flux.ptr, extra_flux.nbytes // 4
        elif extra_flux is not None:
            xf = np.ascontiguousarray(extra_flux, np.float32)
            hx, x_len = xf.ctypes.data, xf.size
        pts = np.ascontiguousarray(np.stack([la, lo], -1))
        rec = max(m - int(model.n_spin), 1)
        shape = {"full": (la.size, rec), "summary": (la.size, 4), "flux": (la.size, m), "exitance": (la.size, rec, 2)}[mode]
        if out is not None and out.nbytes < int(np.prod(shape)) * 4:
            raise ValueError("the device buffer is smaller than the output")
        res = np.empty(shape, np.float32) if out is None else None
        st = MrtxStats()
        self._check(self._lib.mrtx_thermal_scatter(self._ctx, pts.ctypes.data, la.size, n_az, dh, hh, ep.ctypes.data,
                                                   fl.ctypes.data, m, C.byref(model), modes[mode], dx, hx, x_len,
                                                   None if out is None else out.ptr, None if res is None else res.ctypes.data,
                                                   C.byref(st)), "mrtx_thermal_scatter")
        self._add_stats(stats, st, {"newton_cap_hits": "reserved"})
        return out if out is not None else res

    @staticmethod
    def thermal_depths(model=None):
        """The node depths z_i of a MrtxThermalModel in metres, (n_nodes,) float64: z_0 = 0 and z_{i+1} = z_i + dz[i] (the
        model of thermal_grid() unless given)."""
        model = MoonRT.thermal_grid() if model is None else model
        n = int(model.n_nodes)
        return np.concatenate([[0.0], np.cumsum(np.array(model.dz[:n - 1], np.float64))])

    def thermal_column(self, lat_deg, lon_deg, horizon, epochs, flux, model=None, mode="column", extra_flux=None, species=None,
                       stats=None, n_az=None, out=None, occultation=None):
        """surface_temperature_scatter with the subsurface modes of DESIGN.md section 3.16, in one call.  Its modes ("full",
        "summary", "flux", "exitance") give its bits; "column": (N, m - n_spin, n_nodes) float32, every node's temperature
        after each recorded epoch (node 0 is "full"); "volatile": (N, n_nodes, 2) float64 (E_mean, T_max) per node, the mean
        over the recorded epochs of the free sublimation rate of `species` (a volatiles.Species, an MrtxVolatile or its four
        coefficients; kg m^-2 s^-1) and the node's highest temperature.  thermal_depths(model) gives the nodes' depths.
        out = a DeviceBuffer: the output is written there and `out` returned.  occultation = (source_epochs, body_epochs) as
        for MoonRT.occultation, m rows each: every epoch's disc fraction, spin-up included, is multiplied by that call's g at
        the point (section 3.18); None is the call without it."""
        modes = {"full": 0, "summary": 1, "flux": 2, "exitance": 3, "column": 4, "volatile": 5}
        if mode not in modes:
            raise ValueError(f"mode must be one of {sorted(modes)} (got {mode!r})")
        if (mode == "volatile") != (species is not None):
            raise ValueError("species is required in mode 'volatile' and must be None otherwise")
        sp = None
        if species is not None:
            from . import volatiles
            sp = species if isinstance(species, _lib.MrtxVolatile) else volatiles.law(species)
        la, lo = self._points(lat_deg, lon_deg)
        ep = self._epochs(epochs)
        m = ep.shape[0]
        fl = np.ascontiguousarray(np.asarray(flux, np.float64).ravel())
        if fl.size != m:
            raise ValueError("flux must hold one value per epoch")
        model = self.thermal_grid() if model is None else model
        n_az, hz_at = self._horizon_arg(horizon, la.size, n_az)
        dh, hh = hz_at(0)
        dx = hx = None
        x_len = 0
        if isinstance(extra_flux, DeviceBuffer):
            dx, x_len = extra_flux.ptr, extra_flux.nbytes // 4
        elif extra_flux is not None:
            xf = np.ascontiguousarray(extra_flux, np.float32)
            hx, x_len = xf.ctypes.data, xf.size
        pts = np.ascontiguousarray(np.stack([la, lo], -1))
        rec, nn = max(m - int(model.n_spin), 1), max(int(model.n_nodes), 1)
        shape = {"full": (la.size, rec), "summary": (la.size, 4), "flux": (la.size, m), "exitance": (la.size, rec, 2),
                 "column": (la.size, rec, nn), "volatile": (la.size, nn, 2)}[mode]
        dtype = np.float64 if mode == "volatile" else np.float32
        if out is not None and out.nbytes < int(np.prod(shape)) * np.dtype(dtype).itemsize:
            raise ValueError("the device buffer is smaller than the output")
        res = np.empty(shape, dtype) if out is None else None
        st = MrtxStats()
        if occultation is not None:
            os_, ob_ = (self._epochs(e) for e in occultation)
            if os_.shape != ep.shape or ob_.shape != ep.shape:
                raise ValueError("the occultation tables must hold one row per epoch")
            self._check(self._lib.mrtx_thermal_occulted(self._ctx, pts.ctypes.data, la.size, n_az, dh, hh, ep.ctypes.data,
                                                        fl.ctypes.data, m, C.byref(model), modes[mode], dx, hx, x_len,
                                                        None if sp is None else C.byref(sp), os_.ctypes.data, ob_.ctypes.data,
                                                        None if out is None else out.ptr,
                                                        None if res is None else res.ctypes.data, C.byref(st)),
                        "mrtx_thermal_occulted")
            self._add_stats(stats, st, {"newton_cap_hits": "reserved"})
            return out if out is not None else res
        self._check(self._lib.mrtx_thermal_column(self._ctx, pts.ctypes.data, la.size, n_az, dh, hh, ep.ctypes.data,
                                                  fl.ctypes.data, m, C.byref(model), modes[mode], dx, hx, x_len,
                                                  None if sp is None else C.byref(sp), None if out is None else out.ptr,
                                                  None if res is None else res.ctypes.data, C.byref(st)),
                    "mrtx_thermal_column")
        self._add_stats(stats, st, {"newton_cap_hits": "reserved"})
        return out if out is not None else res

    # ---- Terrain line of sight
    @staticmethod
    def _observer(observer):
        o = np.asarray(observer, np.float64)
        if o.shape != (3,):
            raise ValueError("observer must be one (lat, lon, height_m) triple")
        return o

    def viewshed(self, observer, lat=(90.0, -90.0), lon=(-180.0, 180.0), shape=(180, 360), target_height_m=0.0, mast_max_m=0.0,
                 n_bis=0, radius_m=1737400.0, rows=None, stats=None, band_bytes=256 << 20):
        """(rows, w) float32 map over the nodes of illumination_map's grid: per node the extra mast height, metres, at which a
        target raised target_height_m there sees the observer (lat, lon, height_m): 0 where it does already, +inf where even
        mast_max_m does not (n_bis = 0: a plain viewshed, 0 or +inf); otherwise the bisection's n_bis probes narrow it to
        mast_max_m / 2^(n_bis - 1).  radius_m = the metres of D = 1 (1737400 * the DEM's radius_scale).  Bands of at most
        band_bytes go through one device buffer; `stats`, if a dict, receives the summed counters."""
        o = self._observer(observer)
        h, w = int(shape[0]), int(shape[1])
        r0, r1 = (0, h) if rows is None else (int(rows[0]), int(rows[1]))
        g = _lib.MrtxSightGrid(o[0], o[1], o[2], float(target_height_m), float(mast_max_m), float(radius_m), float(lat[0]),
                               float(lat[1]), float(lon[0]), float(lon[1]), h, w, r0, r1, int(n_bis), 0)
        return self._band_map("mrtx_sight_grid", g, np.empty((max(r1 - r0, 0), w), np.float32), 4, band_bytes, stats)

    def line_of_sight(self, lat_deg, lon_deg, observer, target_height_m=0.0, mast_max_m=0.0, n_bis=0, radius_m=1737400.0,
                      stats=None, chunk_bytes=256 << 20):
        """(N,) float32 extra mast heights, metres, of N targets (degrees) toward `observer`: one (lat, lon, height_m) triple
        shared by all, or an (N, 3) array, one per target.  As viewshed; a target on a grid node gives that node's value.
        Calls hold at most chunk_bytes of output each (targets split between calls)."""
        la, lo = self._points(lat_deg, lon_deg)
        obs = np.asarray(observer, np.float64)
        if obs.shape == (3,):
            obs = obs.reshape(1, 3)
        elif obs.shape != (la.size, 3):
            raise ValueError("observer must be one (lat, lon, height_m) triple or one per target, (N, 3)")
        obs = np.ascontiguousarray(obs)
        shared = obs.shape[0] == 1
        pts = np.ascontiguousarray(np.stack([la, lo], -1))
        out = np.empty(la.size, np.float32)
        for a, b in self._chunks(la.size, 1, chunk_bytes, empty_call=False):
            st = MrtxStats()
            op, no = (obs.ctypes.data, 1) if shared else (obs[a:].ctypes.data, b - a)
            self._check(self._lib.mrtx_sight_points(self._ctx, pts[a:].ctypes.data, b - a, op, no, float(target_height_m),
                                                    float(mast_max_m), float(radius_m), int(n_bis), None, out[a:].ctypes.data,
                                                    C.byref(st)), "mrtx_sight_points")
            self._add_stats(stats, st)
        return out

    # ---- Least-cost traverses
    def _dem_hw(self):
        hw = getattr(self, "_dem_shape", None)
        if hw is None:
            raise MoonRTError("no displacement map: call upload_dem or bind_dem first")
        return hw

    def traverse_nodes(self, window):
        """(lat, lon, grid) of a traverse window (row0, col0, rows, cols[, stride[, wrap]]) on the DEM in place: lat (rows,)
        and lon (cols,) float64 degrees of its nodes, the texel centres (lon in [-180, 180)), and grid = dict(lat=, lon=,
        shape=), the arguments with which illumination_map / viewshed sample the same positions node for node (their
        longitudes continue past 180 where the window does; with stride > 1 a window on the DEM's first or last row puts
        lat beyond +-90, which those calls refuse)."""
        from .traverse import window_dict
        w = window_dict(window)
        H, W = self._dem_hw()
        s = w["stride"]
        lat = 90.0 - (w["row0"] + np.arange(w["rows"]) * s + 0.5) * (180.0 / H)
        lon = -180.0 + ((w["col0"] + np.arange(w["cols"]) * s) % W + 0.5) * (360.0 / W)
        la_n = 90.0 - (w["row0"] + 0.5 - 0.5 * s) * (180.0 / H)
        lo_w = -180.0 + (w["col0"] + 0.5 - 0.5 * s) * (360.0 / W)
        grid = {"lat": (la_n, la_n - w["rows"] * s * (180.0 / H)), "lon": (lo_w, lo_w + w["cols"] * s * (360.0 / W)),
                "shape": (w["rows"], w["cols"])}
        return lat, lon, grid

    def snap_to_nodes(self, window, lat_deg, lon_deg):
        """(N, 2) int32 (i, j) of the window nodes nearest to N points: the row whose centre latitude is nearest, the column
        whose centre longitude is nearest around the circle (halves round up to the larger index); ValueError if one lies
        outside the window."""
        from .traverse import window_dict
        w = window_dict(window)
        H, W = self._dem_hw()
        s = w["stride"]
        la = np.atleast_1d(np.asarray(lat_deg, np.float64))
        lo = np.atleast_1d(np.asarray(lon_deg, np.float64))
        i = np.floor(((90.0 - la) * (H / 180.0) - 0.5 - w["row0"]) / s + 0.5).astype(np.int64)
        cc = ((lo + 180.0) * (W / 360.0) - 0.5 - w["col0"]) % W           # texel columns east of col0
        j = np.floor(cc / s + 0.5).astype(np.int64)
        if w["wrap"]:
            j %= w["cols"]
        else:       # nearer to the window's first column going round the circle the other way
            j = np.where(j >= w["cols"], np.where((W - cc) / s <= 0.5, 0, j), j)
        bad = (i < 0) | (i >= w["rows"]) | (j < 0) | (j >= w["cols"])
        if bad.any():
            k = int(np.argmax(bad))
            raise ValueError(f"point ({la[k]}, {lo[k]}) lies outside the window")
        return np.ascontiguousarray(np.stack([i, j], -1).astype(np.int32))

    # what traverse and traverse_timed share: the sources as nodes, the edge lengths, the penalty argument, the stats
    def _traverse_sources(self, w, sources, nodes):
        """(N, 2) int32 (i, j) from exactly one of `sources` ((lat, lon) degrees, snapped) and `nodes`."""
        if (sources is None) == (nodes is None):
            raise ValueError("give exactly one of sources ((lat, lon) degrees) and nodes ((i, j) indices)")
        if nodes is not None:
            ij = np.asarray(nodes)
            if not np.issubdtype(ij.dtype, np.integer):
                raise ValueError("nodes must be integer (i, j) indices")
            ij = np.ascontiguousarray(ij.reshape(-1, 2) if ij.ndim == 1 else ij, np.int32)
        else:
            ll = np.asarray(sources, np.float64)
            ll = ll.reshape(1, -1) if ll.ndim == 1 else ll
            if ll.ndim != 2 or ll.shape[1] != 2:
                raise ValueError("sources must be (N, 2) (lat, lon) degrees")
            ij = self.snap_to_nodes(w, ll[:, 0], ll[:, 1])
        if ij.ndim != 2 or ij.shape[1] != 2:
            raise ValueError("nodes must be (N, 2) (i, j) indices")
        return ij

    def _traverse_lengths(self, t, H, W):
        lengths = np.empty((max(t.rows, 1), 3), np.float32)
        rc = self._lib.mrtx_traverse_lengths(C.byref(t), H, W, lengths.ctypes.data)
        if rc != 0:
            raise MoonRTError(f"mrtx_traverse_lengths failed ({rc}): bad window or lengths")
        return lengths

    @staticmethod
    def _traverse_penalty(w, penalty):
        """(dev_penalty, host_penalty, the host map or None) of a penalty argument; the map must outlive the call."""
        dev_pen = host_pen = pen = None
        if isinstance(penalty, DeviceBuffer):
            if penalty.nbytes < 4 * w["rows"] * w["cols"]:
                raise ValueError("the penalty buffer is smaller than rows x cols float32")
            dev_pen = penalty.ptr
        elif penalty is not None:
            pen = np.ascontiguousarray(penalty, np.float32)
            if pen.shape != (w["rows"], w["cols"]):
                raise ValueError(f"penalty must be a (rows, cols) = {(w['rows'], w['cols'])} map")
            host_pen = pen.ctypes.data
        return dev_pen, host_pen, pen

    @staticmethod
    def _traverse_stats(stats, st, visits):
        if isinstance(stats, dict):
            stats["kernel_ms"] = stats.get("kernel_ms", 0) + st.kernel_ms
            stats["launches"] = stats.get("launches", 0) + st.launches
            stats["tile_visits"] = stats.get("tile_visits", 0) + int(visits.value)

    def traverse(self, window, sources=None, penalty=None, max_slope_deg=20.0, climb_cost=8.0, descent_cost=0.0,
                 radius_m=1737400.0, start_cost=None, stats=None, nodes=None, heights=True):
        """The least-cost field over a window (row0, col0, rows, cols[, stride[, wrap]]) of the DEM's texel lattice
        (mrtx_traverse) from its sources: `sources` = an (N, 2) array of (lat, lon) degrees, each
        snapped to its nearest node (snap_to_nodes), or `nodes` = an (N, 2) array of explicit (i, j) nodes -- exactly one of
        the two; start_cost = N start costs (default 0).  penalty: None, a (rows, cols) float32 map or a DeviceBuffer
        holding one (see moonrtx_amd.traverse for builders).  The effort of a step is its length plus climb_cost per metre
        climbed and descent_cost per metre descended (the defaults: Naismith's rule, 8 m of walking per metre of ascent);
        steps steeper than max_slope_deg are not driven.  radius_m = the metres of D = 1.  Returns a
        moonrtx_amd.traverse.TraverseField; with `heights` it holds the window's node heights (mrtx_traverse_heights), so that
        routes read their heights from the field and not from the context, which may be closed or hold another DEM by then.
        `stats`, if a dict, receives kernel_ms, launches and tile_visits of the traverse."""
        from . import traverse as tv
        w = tv.window_dict(window)
        H, W = self._dem_hw()
        ij = self._traverse_sources(w, sources, nodes)
        cost0 = None if start_cost is None else np.ascontiguousarray(np.broadcast_to(np.asarray(start_cost, np.float64),
                                                                                      (ij.shape[0],)))
        t = self._traverse_window(w, radius_m, tv.max_slope_grade(max_slope_deg), climb_cost, descent_cost)
        lengths = self._traverse_lengths(t, H, W)
        dev_pen, host_pen, pen = self._traverse_penalty(w, penalty)
        cost = np.empty((w["rows"], w["cols"]), np.float64)
        pred = np.empty((w["rows"], w["cols"]), np.uint8)
        visits = C.c_uint64()
        st = MrtxStats()
        self._check(self._lib.mrtx_traverse(self._ctx, C.byref(t), ij.ctypes.data, None if cost0 is None else cost0.ctypes.data,
                                            ij.shape[0], dev_pen, host_pen, None, cost.ctypes.data, None, pred.ctypes.data,
                                            C.byref(visits), C.byref(st)), "mrtx_traverse")
        self._traverse_stats(stats, st, visits)
        lat, lon, _ = self.traverse_nodes(w)
        D = self.traverse_heights(w) if heights else None
        return tv.TraverseField(cost, pred, w, lengths, radius_m, lat, lon, D=D)

    def traverse_timed(self, window, sources=None, nodes=None, start_tick=None, avail=None, n_epochs=None, ticks_per_epoch=3600,
                       ticks_per_cost=5.0, penalty=None, max_slope_deg=20.0, climb_cost=8.0, descent_cost=0.0,
                       radius_m=1737400.0, stats=None):
        """The earliest-arrival field over a traverse window (mrtx_traverse_timed): time in integer
        ticks, an edge of `traverse`'s weight w lasting ceil(w * ticks_per_cost) ticks (at least 1), epoch e covering the
        ticks [e, e + 1) * ticks_per_epoch, and an edge driven only while every epoch it touches is available at both of
        its ends; waiting at a node is free.  window, sources / nodes, penalty and the effort model as for `traverse`;
        start_tick = the sources' start ticks (default 0).  avail: None (always drivable), an (rows, cols, W64) or
        (rows * cols, W64) uint64 array in horizon_mask's layout, or a DeviceBuffer holding one (moonrtx_amd.traverse.
        drive_mask); n_epochs = the epochs it covers (default W64 * 64 for an array, required for a buffer).  Returns a
        moonrtx_amd.traverse.TimedField; `stats`, if a dict, receives kernel_ms, launches and tile_visits."""
        from . import traverse as tv
        w = tv.window_dict(window)
        H, W = self._dem_hw()
        ij = self._traverse_sources(w, sources, nodes)
        tick0 = None if start_tick is None else np.ascontiguousarray(np.broadcast_to(np.asarray(start_tick, np.uint64),
                                                                                      (ij.shape[0],)))
        max_grade = tv.max_slope_grade(max_slope_deg)
        t = self._traverse_window(w, radius_m, max_grade, climb_cost, descent_cost)
        lengths = self._traverse_lengths(t, H, W)
        N = w["rows"] * w["cols"]
        dev_pen, host_pen, pen = self._traverse_penalty(w, penalty)
        dev_av = host_av = av = None
        if isinstance(avail, DeviceBuffer):
            if n_epochs is None:
                raise ValueError("n_epochs is required with a device buffer")
            if avail.nbytes < 8 * N * tv.mask_words(n_epochs):
                raise ValueError("the availability buffer is smaller than rows x cols x W64 uint64")
            dev_av = avail.ptr
        elif avail is not None:
            av = np.ascontiguousarray(avail, np.uint64)
            if av.ndim not in (2, 3) or av.size % max(N, 1) or av.shape[:-1] not in ((N,), (w["rows"], w["cols"])):
                raise ValueError("avail must be a (rows, cols, W64) or (rows * cols, W64) uint64 array")
            n_epochs = av.shape[-1] * 64 if n_epochs is None else int(n_epochs)
            if av.shape[-1] != tv.mask_words(n_epochs):
                raise ValueError(f"{n_epochs} epochs take {tv.mask_words(n_epochs)} words per node (got {av.shape[-1]})")
            av = av.reshape(w["rows"], w["cols"], -1)
            host_av = av.ctypes.data
        tt = _lib.MrtxTraverseTimed(float(ticks_per_cost), int(ticks_per_epoch), 0 if avail is None else int(n_epochs), 0)
        arrival = np.empty((w["rows"], w["cols"]), np.uint64)
        pred = np.empty((w["rows"], w["cols"]), np.uint8)
        visits = C.c_uint64()
        st = MrtxStats()
        self._check(self._lib.mrtx_traverse_timed(self._ctx, C.byref(t), C.byref(tt), ij.ctypes.data,
                                                  None if tick0 is None else tick0.ctypes.data, ij.shape[0], dev_pen, host_pen,
                                                  dev_av, host_av, None, arrival.ctypes.data, None, pred.ctypes.data,
                                                  C.byref(visits), C.byref(st)), "mrtx_traverse_timed")
        self._traverse_stats(stats, st, visits)
        lat, lon, _ = self.traverse_nodes(w)
        if dev_pen is not None:
            pen = penalty.download(np.float32, (w["rows"], w["cols"]))
        return tv.TimedField(arrival, pred, w, lengths, radius_m, lat, lon, D=self.traverse_heights(w),
                             ticks_per_cost=ticks_per_cost, ticks_per_epoch=ticks_per_epoch,
                             n_epochs=None if avail is None else n_epochs, max_grade=max_grade, climb_cost=climb_cost,
                             descent_cost=descent_cost, penalty=pen, avail=av)

    @staticmethod
    def _traverse_window(w, radius_m=1737400.0, max_grade=1.0, climb_cost=0.0, descent_cost=0.0):
        return _lib.MrtxTraverse(w["row0"], w["col0"], w["rows"], w["cols"], w["stride"], w["wrap"], float(radius_m),
                                 float(max_grade), float(climb_cost), float(descent_cost), 0)

    def traverse_heights(self, window, stats=None):
        """(rows, cols) float32 D of a traverse window's nodes, copied from the context's DEM (mrtx_traverse_heights):
        (D - 1) x radius_m is a node's height above the sphere in metres."""
        from .traverse import window_dict
        w = window_dict(window)
        D = np.empty((w["rows"], w["cols"]), np.float32)
        st = MrtxStats()
        self._check(self._lib.mrtx_traverse_heights(self._ctx, C.byref(self._traverse_window(w)), None, D.ctypes.data,
                                                    C.byref(st)), "mrtx_traverse_heights")
        self._add_stats(stats, st)
        return D

    # ---- Terrain relief: slope, roughness, landing hazard
    def relief(self, window, footprint_m=None, footprint_nodes=None, radius_m=1737400.0, stats=None):
        """Slope and roughness under a footprint, per node of a window (row0, col0, rows, cols[, stride]) of the DEM's texel
        lattice (mrtx_relief).  Exactly one of footprint_nodes = (ri, rj), the footprint's half-heights
        in lattice nodes (1 .. 32), and footprint_m, its width in metres: then ri follows from the N-S spacing of the rows, and
        the window is split into row bands over which rj = max(1, round(footprint_m / 2 / L_ew)) is constant, one call per
        band (a footprint reads the DEM, not the window, so the bands join exactly).  radius_m = the metres of D = 1.
        Returns a moonrtx_amd.relief.ReliefMap; `stats`, if a dict, receives the summed counters."""
        from . import relief as rl
        w = rl.window_dict(window)
        if w["wrap"]:
            raise ValueError("a relief window is never wrapped: its footprints read across the seam by themselves")
        H, W = self._dem_hw()
        if (footprint_m is None) == (footprint_nodes is None):
            raise ValueError("give exactly one of footprint_m and footprint_nodes = (ri, rj)")
        if footprint_nodes is not None:
            ri, rj = (int(v) for v in footprint_nodes)
            bands = [(0, w["rows"], rj)]
        else:
            ri, bands = rl.footprint_bands(self._lib, w, footprint_m, radius_m, (H, W))
        table = np.empty((w["rows"], w["cols"], 4), np.float32)
        for a, n, rj in bands:
            st = MrtxStats()
            t = rl.relief_window(w, ri, rj, radius_m, rows=(a, n))
            self._check(self._lib.mrtx_relief(self._ctx, C.byref(t), None, table[a:].ctypes.data, C.byref(st)), "mrtx_relief")
            self._add_stats(stats, st)
        lat, lon, _ = self.traverse_nodes(w)
        return rl.ReliefMap(table, w, radius_m, ri, bands, w["cols"] * w["stride"] == W, lat, lon)

    def landing_share(self, relief, max_slope_deg, max_rms_m, ellipse_m=None, ellipse_nodes=None, stats=None):
        """The safe share of a landing ellipse around every node of a ReliefMap (mrtx_relief_share): (rows, cols) float32,
        the fraction of the map's nodes in the (2 Ri + 1) x (2 Rj + 1) box around the node with slope <= max_slope_deg and
        roughness <= max_rms_m (NaN nodes are unsafe; nodes outside the map do not count, and the columns join across +-180
        when the map goes round the circle).  Exactly one of ellipse_nodes = (Ri, Rj), 0 .. 1024, and ellipse_m, the box's
        width in metres, turned into nodes with the map's N-S spacing and the E-W spacing of its middle row."""
        from . import relief as rl
        from .traverse import max_slope_grade
        w = relief.window
        if (ellipse_m is None) == (ellipse_nodes is None):
            raise ValueError("give exactly one of ellipse_m and ellipse_nodes = (Ri, Rj)")
        if ellipse_nodes is not None:
            Ri, Rj = (int(v) for v in ellipse_nodes)
        else:
            k = rl.scales(self._lib, rl.relief_window(w, radius_m=relief.radius_m), self._dem_hw())
            half = 0.5 * float(ellipse_m) / relief.radius_m
            Ri, Rj = int(math.floor(half * k[0, 1] + 0.5)), int(math.floor(half * k[w["rows"] // 2, 0] + 0.5))
        s = _lib.MrtxReliefShare(w["rows"], w["cols"], Ri, Rj, 1 if relief.closes_circle and w["cols"] >= 3 else 0, 0,
                                 max_slope_grade(max_slope_deg), float(max_rms_m))
        table = np.ascontiguousarray(relief.table, np.float32)
        out = np.empty((w["rows"], w["cols"]), np.float32)
        st = MrtxStats()
        self._check(self._lib.mrtx_relief_share(self._ctx, C.byref(s), None, table.ctypes.data, None, out.ctypes.data,
                                                C.byref(st)), "mrtx_relief_share")
        self._add_stats(stats, st)
        return out

    # ---- Connected regions of a per-node map
    def regions(self, field=None, mask=None, channel=0, lo=-math.inf, hi=math.inf, connectivity=4, wrap=False,
                row_weights=None, stats=None, shape=None, unit_m2=None):
        """The connected regions of a set of lattice nodes (mrtx_regions_label, mrtx_regions_stats).  Exactly one of `field`,
        (rows, cols) or (rows, cols, n_ch) float32: the nodes with lo <= field[..., channel] <= hi, compared as float32 (NaN
        is out), and `mask`, (rows, cols) uint8: the nonzero nodes.  Either may be a numpy array or a DeviceBuffer (then give
        shape = (rows, cols[, n_ch]); labels and catalogue are made in device tables and downloaded).  connectivity 4 or 8;
        wrap joins the last column to the first (cols >= 3).  row_weights: (rows,) uint32 node areas (regions.row_weights),
        or None: every node weighs 1; unit_m2: their unit, remembered by the map.  Needs no DEM.  Returns a
        moonrtx_amd.regions.RegionMap; `stats`, if a dict, receives the summed counters and label_ms / catalogue_ms."""
        from . import regions as rg
        if (field is None) == (mask is None):
            raise ValueError("give exactly one of field and mask")
        src = field if field is not None else mask
        on_device = isinstance(src, DeviceBuffer)
        if on_device:
            if shape is None:
                raise ValueError("a DeviceBuffer needs shape = (rows, cols[, n_ch])")
            shp = tuple(int(v) for v in shape)
        else:
            src = np.ascontiguousarray(src, np.float32 if field is not None else np.uint8)
            shp = src.shape
        if field is not None and len(shp) == 2:
            shp = shp + (1,)
        if len(shp) != (3 if field is not None else 2):
            raise ValueError("field must be (rows, cols) or (rows, cols, n_ch), mask (rows, cols)")
        rows, cols = shp[0], shp[1]
        n_ch = shp[2] if field is not None else 1
        if on_device and src.nbytes < rows * cols * (4 * n_ch if field is not None else 1):
            raise ValueError("the DeviceBuffer is smaller than its shape")
        weights = None
        if row_weights is not None:
            weights = np.ascontiguousarray(row_weights)
            if weights.shape != (rows,) or not np.issubdtype(weights.dtype, np.integer) or \
                    (weights.size and (weights.min() < 0 or weights.max() > rg.WEIGHT_MAX)):
                raise ValueError("row_weights must be (rows,) integers in 0 .. 2^32 - 1")
            weights = weights.astype(np.uint32)
        r = _lib.MrtxRegions(rows, cols, 1 if wrap else 0, int(connectivity), n_ch, int(channel), float(lo), float(hi), 0)
        n = C.c_uint32(0)
        st, st2 = MrtxStats(), MrtxStats()
        wp = weights.ctypes.data if weights is not None else None
        if on_device:
            lab = DeviceBuffer(max(4 * rows * cols, 4), src.device)
            args = (src.ptr, None, None, None) if field is not None else (None, None, src.ptr, None)
            self._check(self._lib.mrtx_regions_label(self._ctx, C.byref(r), *args, lab.ptr, None, C.byref(n), C.byref(st)),
                        "mrtx_regions_label")
            rec = DeviceBuffer(max(56 * n.value, 56), src.device)
            self._check(self._lib.mrtx_regions_stats(self._ctx, rows, cols, r.wrap, lab.ptr, None, n.value, wp, rec.ptr, None,
                                                     C.byref(st2)), "mrtx_regions_stats")
            labels = lab.download(np.int32, (rows, cols))
            table = rec.download(rg.REGION_DTYPE, (n.value,))
            lab.free()
            rec.free()
        else:
            labels = np.empty((rows, cols), np.int32)
            args = (None, src.ctypes.data, None, None) if field is not None else (None, None, None, src.ctypes.data)
            self._check(self._lib.mrtx_regions_label(self._ctx, C.byref(r), *args, None, labels.ctypes.data, C.byref(n),
                                                     C.byref(st)), "mrtx_regions_label")
            table = np.zeros(max(n.value, 1), rg.REGION_DTYPE)
            self._check(self._lib.mrtx_regions_stats(self._ctx, rows, cols, r.wrap, None, labels.ctypes.data, n.value, wp, None,
                                                     table.ctypes.data, C.byref(st2)), "mrtx_regions_stats")
            table = table[:n.value]
        self._add_stats(stats, st)
        self._add_stats(stats, st2)
        if isinstance(stats, dict):
            stats["label_ms"] = stats.get("label_ms", 0.0) + st.kernel_ms
            stats["catalogue_ms"] = stats.get("catalogue_ms", 0.0) + st2.kernel_ms
            stats["label_launches"] = stats.get("label_launches", 0) + st.launches
        return rg.RegionMap(labels, table, wrap, unit_m2)

    # ---- Zonal statistics and outlines of labelled regions
    @staticmethod
    def _label_arg(labels, shape):
        """(device pointer, host pointer, rows, cols, keepalive) of a label table: (rows, cols) int32 or a DeviceBuffer."""
        if isinstance(labels, DeviceBuffer):
            if shape is None:
                raise ValueError("a DeviceBuffer needs shape = (rows, cols)")
            rows, cols = int(shape[0]), int(shape[1])
            if labels.nbytes < 4 * rows * cols:
                raise ValueError("the label DeviceBuffer is smaller than its shape")
            return labels.ptr, None, rows, cols, labels
        a = np.ascontiguousarray(labels, np.int32)
        if a.ndim != 2:
            raise ValueError("labels must be (rows, cols)")
        return None, a.ctypes.data, int(a.shape[0]), int(a.shape[1]), a

    @staticmethod
    def _row_table(table, n, what):
        if table is None:
            return None
        t = np.ascontiguousarray(table)
        if t.shape != (n,) or not np.issubdtype(t.dtype, np.integer) or (t.size and (t.min() < 0 or t.max() > 2 ** 32 - 1)):
            raise ValueError(f"{what} must be ({n},) integers in 0 .. 2^32 - 1")
        return t.astype(np.uint32)

    def region_statistics(self, labels, n_regions, field, row_weights=None, scale=1.0, hist=None, wrap=False, shape=None,
                          stats=None):
        """What is inside each region of a label table (mrtx_regions_zonal): count, NaN count, exact fixed-point sums (q =
        llrint(x * scale)), area-weighted sums, and the extremes with their places, per region and channel.  labels: (rows,
        cols) int32 or a DeviceBuffer (then give shape = (rows, cols)); field: (rows, cols) or (rows, cols, n_ch) float32 or a
        DeviceBuffer (then shape = (rows, cols, n_ch)); both from one side: with a DeviceBuffer among them the records are
        made in device tables and downloaded.  row_weights: (rows,) uint32 node areas or None.  hist = (channel, n_bins, lo,
        hi): also the weight of every region per value band.  Returns a (n_regions, n_ch) array of regions.ZONAL_DTYPE, and
        with hist the pair (records, (n_regions, n_bins + 2) uint64).  Raises MoonRTError when a weighted sum may have
        wrapped (regions.check_wsum): lower scale then."""
        from . import regions as rg
        n_regions = int(n_regions)
        dev_f = isinstance(field, DeviceBuffer)
        dev_l = isinstance(labels, DeviceBuffer)
        if dev_f != dev_l:
            raise ValueError("labels and field must both be numpy arrays or both DeviceBuffers")
        if dev_f:
            if shape is None or len(shape) != 3:
                raise ValueError("DeviceBuffers need shape = (rows, cols, n_ch)")
            n_ch = int(shape[2])
        else:
            field = np.ascontiguousarray(field, np.float32)
            if field.ndim == 2:
                field = field[:, :, None]
            if field.ndim != 3:
                raise ValueError("field must be (rows, cols) or (rows, cols, n_ch)")
            n_ch = int(field.shape[2])
        lab_d, lab_h, rows, cols, _keep = self._label_arg(labels, shape)
        if dev_f:
            if field.nbytes < 4 * rows * cols * n_ch:
                raise ValueError("the field DeviceBuffer is smaller than its shape")
        elif field.shape[:2] != (rows, cols):
            raise ValueError("field and labels differ in shape")
        weights = self._row_table(row_weights, rows, "row_weights")
        hist_ch, n_bins, lo, inv_w = 0, 0, 0.0, 1.0
        if hist is not None:
            hist_ch, n_bins, lo, hi = int(hist[0]), int(hist[1]), float(hist[2]), float(hist[3])
            if n_bins < 1 or not hi > lo:
                raise ValueError("hist = (channel, n_bins >= 1, lo, hi > lo)")
            inv_w = n_bins / (hi - lo)
        z = _lib.MrtxZonalSpec(rows, cols, 1 if wrap else 0, n_ch, float(scale), hist_ch, n_bins, lo, inv_w, 0)
        wp = weights.ctypes.data if weights is not None else None
        st = MrtxStats()
        width = n_bins + 2
        if dev_f:
            rec = DeviceBuffer(max(56 * n_regions * n_ch, 56), field.device)
            hb = DeviceBuffer(max(8 * n_regions * width, 8), field.device) if n_bins else None
            try:
                self._check(self._lib.mrtx_regions_zonal(self._ctx, C.byref(z), lab_d, None, n_regions, field.ptr, None, wp,
                                                         rec.ptr, None, hb.ptr if hb else None, None, C.byref(st)),
                            "mrtx_regions_zonal")
                table = rec.download(rg.ZONAL_DTYPE, (n_regions, n_ch))
                h = hb.download(np.uint64, (n_regions, width)) if hb else None
            finally:
                rec.free()
                if hb:
                    hb.free()
        else:
            table = np.zeros((max(n_regions, 1), n_ch), rg.ZONAL_DTYPE)
            h = np.zeros((max(n_regions, 1), width), np.uint64) if n_bins else None
            self._check(self._lib.mrtx_regions_zonal(self._ctx, C.byref(z), None, lab_h, n_regions, None, field.ctypes.data, wp,
                                                     None, table.ctypes.data, None, h.ctypes.data if n_bins else None,
                                                     C.byref(st)), "mrtx_regions_zonal")
            table = table[:n_regions]
            h = h[:n_regions] if n_bins else None
        self._add_stats(stats, st)
        try:
            rg.check_wsum(table, float(scale))
        except OverflowError as e:
            raise MoonRTError(str(e)) from e
        return (table, h) if n_bins else table

    def region_shapes(self, labels, n_regions, connectivity=4, wrap=False, side_ew=None, side_ns=None, shape=None, stats=None):
        """The outline of each region of a label table (mrtx_regions_shape): perimeter, boundary-side counts, the bit-quad
        counts and the Euler number (components minus holes in the given connectivity).  labels: (rows, cols) int32 or a
        DeviceBuffer (then give shape = (rows, cols)).  side_ew (rows,) and side_ns (rows + 1,) uint32 side lengths
        (regions.side_weights), both or neither: with neither every side counts 1.  Returns (n_regions,) regions.SHAPE_DTYPE."""
        from . import regions as rg
        n_regions = int(n_regions)
        lab_d, lab_h, rows, cols, _keep = self._label_arg(labels, shape)
        if (side_ew is None) != (side_ns is None):
            raise ValueError("give both of side_ew and side_ns or neither")
        ew = self._row_table(side_ew, rows, "side_ew")
        ns = self._row_table(side_ns, rows + 1, "side_ns")
        ewp, nsp = (ew.ctypes.data, ns.ctypes.data) if ew is not None else (None, None)
        st = MrtxStats()
        if lab_d is not None:
            rec = DeviceBuffer(max(32 * n_regions, 32), labels.device)
            try:
                self._check(self._lib.mrtx_regions_shape(self._ctx, rows, cols, 1 if wrap else 0, int(connectivity), lab_d, None,
                                                         n_regions, ewp, nsp, rec.ptr, None, C.byref(st)), "mrtx_regions_shape")
                table = rec.download(rg.SHAPE_DTYPE, (n_regions,))
            finally:
                rec.free()
        else:
            table = np.zeros(max(n_regions, 1), rg.SHAPE_DTYPE)
            self._check(self._lib.mrtx_regions_shape(self._ctx, rows, cols, 1 if wrap else 0, int(connectivity), None, lab_h,
                                                     n_regions, ewp, nsp, None, table.ctypes.data, C.byref(st)),
                        "mrtx_regions_shape")
            table = table[:n_regions]
        self._add_stats(stats, st)
        return table

    # ---- Proximity maps and the reach of labelled regions
    def proximity(self, labels, positions, to="set", shape=None, stats=None, unit_m=None):
        """Every node's nearest feature node and the exact squared distance to it (mrtx_proximity), between node positions in
        three dimensions: to="set" measures to the nodes with label >= 0, to="outside" to those with label < 0; ties go to
        the least node index.  labels: (rows, cols) int32 or a DeviceBuffer; positions: (rows, cols, 3) int32
        (regions.node_positions), every coordinate within +-2^29, or a DeviceBuffer; both from one side, and with
        DeviceBuffers give shape = (rows, cols): the tables are then made on the device and downloaded.  unit_m: the metres
        of one unit of the positions, for the map's distances in metres.  Returns regions.ProximityMap.  stats gains
        launches, kernel_ms and pairs, the number of distance evaluations."""
        from . import regions as rg
        modes = {"set": _lib.PROX_TO_SET, "outside": _lib.PROX_TO_OUTSIDE}
        if to not in modes:
            raise ValueError('to must be "set" or "outside"')
        dev = isinstance(positions, DeviceBuffer)
        if dev != isinstance(labels, DeviceBuffer):
            raise ValueError("labels and positions must both be numpy arrays or both DeviceBuffers")
        lab_d, lab_h, rows, cols, _keep = self._label_arg(labels, shape)
        n = rows * cols
        p = _lib.MrtxProximity(rows, cols, modes[to], 0)
        st = MrtxStats()
        pairs = C.c_uint64(0)
        if dev:
            if positions.nbytes < 12 * n:
                raise ValueError("the position DeviceBuffer is smaller than its shape")
            near_b = DeviceBuffer(4 * n, positions.device)
            d2_b = DeviceBuffer(8 * n, positions.device)
            try:
                self._check(self._lib.mrtx_proximity(self._ctx, C.byref(p), positions.ptr, None, lab_d, None, near_b.ptr, None,
                                                     d2_b.ptr, None, C.byref(pairs), C.byref(st)), "mrtx_proximity")
                nearest = near_b.download(np.int32, (rows, cols))
                dist2 = d2_b.download(np.uint64, (rows, cols))
            finally:
                near_b.free()
                d2_b.free()
        else:
            pos = np.ascontiguousarray(positions)
            if pos.shape != (rows, cols, 3) or not np.issubdtype(pos.dtype, np.integer):
                raise ValueError("positions must be (rows, cols, 3) integers")
            if pos.size and (pos.min() < -rg.COORD_MAX or pos.max() > rg.COORD_MAX):
                raise ValueError("a coordinate leaves +-2^29: choose a larger unit")
            pos = pos.astype(np.int32)
            nearest = np.empty((rows, cols), np.int32)
            dist2 = np.empty((rows, cols), np.uint64)
            self._check(self._lib.mrtx_proximity(self._ctx, C.byref(p), None, pos.ctypes.data, None, lab_h, None,
                                                 nearest.ctypes.data, None, dist2.ctypes.data, C.byref(pairs), C.byref(st)),
                        "mrtx_proximity")
        self._add_stats(stats, st)
        if isinstance(stats, dict):
            stats["pairs"] = stats.get("pairs", 0) + int(pairs.value)
        return rg.ProximityMap(nearest, dist2, unit_m)

    def region_reach(self, labels, n_regions, prox, shape=None, stats=None):
        """The extremes of a proximity map over each region of a label table (mrtx_regions_reach): the greatest and least
        dist2 of the region's nodes, the least node index attaining each, and the nearest feature of the closest node.
        labels: (rows, cols) int32 or a DeviceBuffer (then give shape = (rows, cols)); prox: a regions.ProximityMap or a pair
        (dist2, nearest) of arrays.  On a to="outside" map of the regions' own labels d2_max and max_at are the radius and
        the centre of the largest circle in each region; on a to="set" map of another set d2_min, min_at and min_nearest say
        how close each region comes to it.  Returns (n_regions,) regions.REACH_DTYPE."""
        from . import regions as rg
        n_regions = int(n_regions)
        lab_d, lab_h, rows, cols, _keep = self._label_arg(labels, shape)
        d2, near = (prox.dist2, prox.nearest) if isinstance(prox, rg.ProximityMap) else prox
        d2 = np.ascontiguousarray(d2, np.uint64)
        near = np.ascontiguousarray(near, np.int32)
        if d2.shape != (rows, cols) or near.shape != (rows, cols):
            raise ValueError("the proximity map and labels differ in shape")
        table = np.zeros(max(n_regions, 1), rg.REACH_DTYPE)
        st = MrtxStats()
        self._check(self._lib.mrtx_regions_reach(self._ctx, rows, cols, lab_d, lab_h, n_regions, None, d2.ctypes.data, None,
                                                 near.ctypes.data, None, table.ctypes.data, C.byref(st)), "mrtx_regions_reach")
        self._add_stats(stats, st)
        return table[:n_regions]

    # ---- Region outlines
    def region_outlines(self, labels, n_regions, connectivity=4, wrap=False, corners=True, row_weights=None, shape=None,
                        stats=None):
        """The ordered boundary rings of each region of a label table (mrtx_regions_outline): every ring from its least side
        on, the region on its right, holes as rings of their own, x unwrapped along a ring that crosses the seam.  labels:
        (rows, cols) int32 or a DeviceBuffer (then give shape = (rows, cols), and the tables are made on the device and
        downloaded).  corners: only the vertices at which a ring turns (else one per boundary side).  row_weights: (rows,)
        uint32 node areas for MrtxRing.warea, or None.  One call counts, a second fills tables of exactly that size.  Returns
        regions.Outlines."""
        from . import regions as rg
        n_regions = int(n_regions)
        lab_d, lab_h, rows, cols, _keep = self._label_arg(labels, shape)
        weights = self._row_table(row_weights, rows, "row_weights")
        wp = weights.ctypes.data if weights is not None else None
        o = _lib.MrtxOutline(rows, cols, 1 if wrap else 0, int(connectivity), _lib.OUTLINE_CORNERS if corners else _lib.OUTLINE_ALL, 0)
        nr, nv = C.c_uint64(0), C.c_uint64(0)
        st, st2 = MrtxStats(), MrtxStats()
        self._check(self._lib.mrtx_regions_outline(self._ctx, C.byref(o), lab_d, lab_h, n_regions, wp, None, None, 0, None, None, 0,
                                                   C.byref(nr), C.byref(nv), C.byref(st)), "mrtx_regions_outline")
        self._add_stats(stats, st)
        n_r, n_v = int(nr.value), int(nv.value)
        if lab_d is not None:
            rb = DeviceBuffer(max(48 * n_r, 48), labels.device)
            vb = DeviceBuffer(max(8 * n_v, 8), labels.device)
            try:
                self._check(self._lib.mrtx_regions_outline(self._ctx, C.byref(o), lab_d, None, n_regions, wp, rb.ptr, None, n_r, vb.ptr,
                                                           None, n_v, C.byref(nr), C.byref(nv), C.byref(st2)), "mrtx_regions_outline")
                rings = rb.download(rg.RING_DTYPE, (n_r,))
                vertices = vb.download(np.int32, (n_v, 2))
            finally:
                rb.free()
                vb.free()
        else:
            rings = np.zeros(max(n_r, 1), rg.RING_DTYPE)
            vertices = np.zeros((max(n_v, 1), 2), np.int32)
            self._check(self._lib.mrtx_regions_outline(self._ctx, C.byref(o), None, lab_h, n_regions, wp, None, rings.ctypes.data, n_r,
                                                       None, vertices.ctypes.data, n_v, C.byref(nr), C.byref(nv), C.byref(st2)),
                        "mrtx_regions_outline")
            rings, vertices = rings[:n_r], vertices[:n_v]
        self._add_stats(stats, st2)
        if isinstance(stats, dict):
            stats["count_ms"] = stats.get("count_ms", 0.0) + st.kernel_ms
            stats["fill_ms"] = stats.get("fill_ms", 0.0) + st2.kernel_ms
        return rg.Outlines(rings, vertices, rows, cols, wrap)

    # ---- Contour lines
    def contours(self, z, levels, wrap=False, shape=None, stats=None):
        """The contour lines of a lattice of integer heights at a table of levels (mrtx_contours): every line an ordered run
        of crossed edges with the above side (z >= level) on its right, closed, or open where it meets the lattice's edge or
        a void node.  z: (rows, cols) int32 within +-2^30 (basins.quantise_heights), contours.VOID where there is no node, or
        a DeviceBuffer (then give shape = (rows, cols); the tables are made on the device and downloaded together with the
        heights).  levels: strictly ascending int32 (contours.levels_for), at most 65536.  One call counts, a second fills
        tables of exactly that size.  Needs no DEM.  Returns contours.Contours; stats gains launches, kernel_ms, count_ms and
        fill_ms."""
        from . import contours as ct
        dev = isinstance(z, DeviceBuffer)
        if dev:
            if shape is None:
                raise ValueError("a DeviceBuffer needs shape = (rows, cols)")
            rows, cols = int(shape[0]), int(shape[1])
        else:
            h = np.asarray(z)
            if h.ndim != 2:
                raise ValueError("z must be (rows, cols)")
            rows, cols = int(h.shape[0]), int(h.shape[1])
        z_d, z_h, z_keep = self._int32_arg(z, (rows, cols), "z")
        lv = np.asarray(levels)
        if lv.ndim != 1 or not 1 <= lv.size <= _lib.CONTOUR_MAX_LEVELS or not np.issubdtype(lv.dtype, np.integer):
            raise ValueError(f"levels must be 1 .. {_lib.CONTOUR_MAX_LEVELS} integers")
        if lv.min() < -2 ** 31 or lv.max() > 2 ** 31 - 1:
            raise ValueError("levels leave int32")
        lv = np.ascontiguousarray(lv, np.int32)
        k = _lib.MrtxContours(rows, cols, 1 if wrap else 0, int(lv.size), 0)
        nl, nv = C.c_uint64(0), C.c_uint64(0)
        st, st2 = MrtxStats(), MrtxStats()
        self._check(self._lib.mrtx_contours(self._ctx, C.byref(k), z_d, z_h, lv.ctypes.data, None, None, 0, None, None, 0,
                                            C.byref(nl), C.byref(nv), C.byref(st)), "mrtx_contours")
        self._add_stats(stats, st)
        n_l, n_v = int(nl.value), int(nv.value)
        if dev:
            lb = DeviceBuffer(max(32 * n_l, 32), z.device)
            vb = DeviceBuffer(max(4 * n_v, 4), z.device)
            try:
                self._check(self._lib.mrtx_contours(self._ctx, C.byref(k), z_d, None, lv.ctypes.data, lb.ptr, None, n_l, vb.ptr, None,
                                                    n_v, C.byref(nl), C.byref(nv), C.byref(st2)), "mrtx_contours")
                lines = lb.download(_lib.CONTOUR_LINE_DTYPE, (n_l,))
                vertices = vb.download(np.int32, (n_v,))
                heights = z.download(np.int32, (rows, cols))
            finally:
                lb.free()
                vb.free()
        else:
            lines = np.zeros(max(n_l, 1), _lib.CONTOUR_LINE_DTYPE)
            vertices = np.zeros(max(n_v, 1), np.int32)
            self._check(self._lib.mrtx_contours(self._ctx, C.byref(k), None, z_h, lv.ctypes.data, None, lines.ctypes.data, n_l, None,
                                                vertices.ctypes.data, n_v, C.byref(nl), C.byref(nv), C.byref(st2)), "mrtx_contours")
            lines, vertices = lines[:n_l], vertices[:n_v]
            heights = z_keep
        self._add_stats(stats, st2)
        if isinstance(stats, dict):
            stats["count_ms"] = stats.get("count_ms", 0.0) + st.kernel_ms
            stats["fill_ms"] = stats.get("fill_ms", 0.0) + st2.kernel_ms
        return ct.Contours(lines, vertices, heights, lv, wrap)

    # ---- Terrain depressions
    @staticmethod
    def _int32_arg(table, shape, what):
        """(device pointer, host pointer, keepalive) of a (rows, cols) int32 table: a numpy array or a DeviceBuffer."""
        if isinstance(table, DeviceBuffer):
            if table.nbytes < 4 * shape[0] * shape[1]:
                raise ValueError(f"the {what} DeviceBuffer is smaller than its shape")
            return table.ptr, None, table
        a = np.ascontiguousarray(table)
        if a.shape != tuple(shape) or not np.issubdtype(a.dtype, np.integer):
            raise ValueError(f"{what} must be ({shape[0]}, {shape[1]}) integers")
        if a.size and (a.min() < -2 ** 31 or a.max() > 2 ** 31 - 1):
            raise ValueError(f"{what} leaves int32")
        a = a.astype(np.int32)
        return None, a.ctypes.data, a

    def fill_depressions(self, heights, outlets=None, edge_outlets=True, connectivity=8, wrap=False, shape=None, stats=None,
                         unit_m=None):
        """The level up to which every node of a lattice of integer heights is closed (mrtx_fill): the least, over all paths
        to an outlet, of the greatest height on the path.  heights: (rows, cols) int32 within +-2^30 (basins.quantise_heights)
        or a DeviceBuffer (then give shape = (rows, cols); the fill is made in a device table and downloaded together with
        the heights).  Outlets: with edge_outlets the lattice's border rows and, without wrap, its border columns; and the
        nonzero nodes of `outlets`, (rows, cols) uint8 or a DeviceBuffer, if given.  unit_m: the metres of one unit of
        height, remembered by the map.  Needs no DEM.  Returns a moonrtx_amd.basins.FillMap; stats gains launches, kernel_ms
        and visits."""
        from . import basins as bs
        dev = isinstance(heights, DeviceBuffer)
        if dev:
            if shape is None:
                raise ValueError("a DeviceBuffer needs shape = (rows, cols)")
            rows, cols = int(shape[0]), int(shape[1])
        else:
            h = np.asarray(heights)
            if h.ndim != 2:
                raise ValueError("heights must be (rows, cols)")
            rows, cols = int(h.shape[0]), int(h.shape[1])
        z_d, z_h, z_keep = self._int32_arg(heights, (rows, cols), "heights")
        o_d = o_h = o_keep = None
        if isinstance(outlets, DeviceBuffer):
            if outlets.nbytes < rows * cols:
                raise ValueError("the outlet DeviceBuffer is smaller than its shape")
            o_d = outlets.ptr
        elif outlets is not None:
            o_keep = np.ascontiguousarray(np.asarray(outlets) != 0, np.uint8)
            if o_keep.shape != (rows, cols):
                raise ValueError("outlets and heights differ in shape")
            o_h = o_keep.ctypes.data
        f = _lib.MrtxFill(rows, cols, 1 if wrap else 0, int(connectivity), 1 if edge_outlets else 0, 0)
        st = MrtxStats()
        visits = C.c_uint64(0)
        if dev:
            fb = DeviceBuffer(max(4 * rows * cols, 4), heights.device)
            try:
                self._check(self._lib.mrtx_fill(self._ctx, C.byref(f), z_d, None, o_d, o_h, fb.ptr, None, C.byref(visits),
                                                C.byref(st)), "mrtx_fill")
                fill = fb.download(np.int32, (rows, cols))
                z = heights.download(np.int32, (rows, cols))
            finally:
                fb.free()
        else:
            fill = np.empty((rows, cols), np.int32)
            self._check(self._lib.mrtx_fill(self._ctx, C.byref(f), None, z_h, o_d, o_h, None, fill.ctypes.data, C.byref(visits),
                                            C.byref(st)), "mrtx_fill")
            z = z_keep
        self._add_stats(stats, st)
        if isinstance(stats, dict):
            stats["visits"] = stats.get("visits", 0) + int(visits.value)
        return bs.FillMap(z, fill, unit_m, int(connectivity), bool(wrap))

    def basins(self, labels, n_regions, fillmap, row_weights=None, connectivity=None, wrap=None, shape=None, stats=None):
        """One record per region of a label table over a fill (mrtx_fill_basins): weight, volume, the extremes of the fill,
        the greatest depth and its place, and the pour point, the neighbour outside the region of least (fill, index).
        labels: (rows, cols) int32, any table, or a DeviceBuffer (then give shape = (rows, cols)); fillmap: a basins.FillMap,
        or a pair (z, fill) of (rows, cols) int32 arrays or DeviceBuffers; connectivity and wrap default to the map's (8 and
        False for a pair).  With a DeviceBuffer among the tables the records are made in a device table and downloaded.
        row_weights: (rows,) uint32 node areas or None.  Returns (n_regions,) basins.BASIN_DTYPE."""
        from . import basins as bs
        n_regions = int(n_regions)
        lab_d, lab_h, rows, cols, _keep = self._label_arg(labels, shape)
        if isinstance(fillmap, bs.FillMap):
            z, fill = fillmap.z, fillmap.fill
            connectivity = fillmap.connectivity if connectivity is None else connectivity
            wrap = fillmap.wrap if wrap is None else wrap
        else:
            z, fill = fillmap
            connectivity = 8 if connectivity is None else connectivity
            wrap = False if wrap is None else wrap
        z_d, z_h, _kz = self._int32_arg(z, (rows, cols), "heights")
        f_d, f_h, _kf = self._int32_arg(fill, (rows, cols), "fill")
        weights = self._row_table(row_weights, rows, "row_weights")
        wp = weights.ctypes.data if weights is not None else None
        st = MrtxStats()
        on_dev = [b for b in (labels, z, fill) if isinstance(b, DeviceBuffer)]
        if on_dev:
            rec = DeviceBuffer(max(48 * n_regions, 48), on_dev[0].device)
            try:
                self._check(self._lib.mrtx_fill_basins(self._ctx, rows, cols, 1 if wrap else 0, int(connectivity), lab_d, lab_h,
                                                       n_regions, z_d, z_h, f_d, f_h, wp, rec.ptr, None, C.byref(st)),
                            "mrtx_fill_basins")
                table = rec.download(bs.BASIN_DTYPE, (n_regions,))
            finally:
                rec.free()
        else:
            table = np.zeros(max(n_regions, 1), bs.BASIN_DTYPE)
            self._check(self._lib.mrtx_fill_basins(self._ctx, rows, cols, 1 if wrap else 0, int(connectivity), None, lab_h,
                                                   n_regions, None, z_h, None, f_h, wp, None, table.ctypes.data, C.byref(st)),
                        "mrtx_fill_basins")
            table = table[:n_regions]
        self._add_stats(stats, st)
        return table

    # ---- The depression hierarchy
    def bowls(self, heights, outlets=None, edge_outlets=True, connectivity=8, wrap=False, invert=False, row_weights=None,
              labels=True, shape=None, stats=None, unit_m=None):
        """The nested closed bowls of a lattice of integer heights (mrtx_bowls): one record per bowl with its floor, its spill
        point, its parent, weight and volume, and per node the innermost bowl that holds it.  heights, outlets, edge_outlets,
        connectivity, wrap and unit_m as in fill_depressions (a DeviceBuffer needs shape = (rows, cols); the tables are then
        made on the device and downloaded).  invert: the same for -heights, levels reported in the caller's heights: summits,
        key cols and prominences.  row_weights: (rows,) uint32 node areas or None.  labels = False leaves the label table out.
        One call counts, a second fills a table of exactly that size.  Needs no DEM.  Returns a moonrtx_amd.basins.BowlTree;
        stats gains launches, kernel_ms, rounds and bowls."""
        from . import basins as bs
        dev = isinstance(heights, DeviceBuffer)
        if dev:
            if shape is None:
                raise ValueError("a DeviceBuffer needs shape = (rows, cols)")
            rows, cols = int(shape[0]), int(shape[1])
        else:
            h = np.asarray(heights)
            if h.ndim != 2:
                raise ValueError("heights must be (rows, cols)")
            rows, cols = int(h.shape[0]), int(h.shape[1])
        z_d, z_h, z_keep = self._int32_arg(heights, (rows, cols), "heights")
        o_d = o_h = o_keep = None
        if isinstance(outlets, DeviceBuffer):
            if outlets.nbytes < rows * cols:
                raise ValueError("the outlet DeviceBuffer is smaller than its shape")
            o_d = outlets.ptr
        elif outlets is not None:
            o_keep = np.ascontiguousarray(np.asarray(outlets) != 0, np.uint8)
            if o_keep.shape != (rows, cols):
                raise ValueError("outlets and heights differ in shape")
            o_h = o_keep.ctypes.data
        weights = self._row_table(row_weights, rows, "row_weights")
        wp = weights.ctypes.data if weights is not None else None
        blk = _lib.MrtxBowls(rows, cols, 1 if wrap else 0, int(connectivity), 1 if edge_outlets else 0, 1 if invert else 0)
        st, st2 = MrtxStats(), MrtxStats()
        nb, rounds = C.c_uint64(0), C.c_uint64(0)
        self._check(self._lib.mrtx_bowls(self._ctx, C.byref(blk), z_d, z_h, o_d, o_h, wp, None, None, 0, None, None, C.byref(nb),
                                         C.byref(rounds), C.byref(st)), "mrtx_bowls")
        self._add_stats(stats, st)
        n = int(nb.value)
        table = None
        if dev:
            rb = DeviceBuffer(max(64 * n, 64), heights.device)
            lb = DeviceBuffer(max(4 * rows * cols, 4), heights.device) if labels else None
            try:
                self._check(self._lib.mrtx_bowls(self._ctx, C.byref(blk), z_d, None, o_d, o_h, wp, rb.ptr, None, n,
                                                 lb.ptr if labels else None, None, C.byref(nb), C.byref(rounds), C.byref(st2)),
                            "mrtx_bowls")
                records = rb.download(bs.BOWL_DTYPE, (n,))
                if labels:
                    table = lb.download(np.int32, (rows, cols))
                z = heights.download(np.int32, (rows, cols))
            finally:
                rb.free()
                if lb is not None:
                    lb.free()
        else:
            records = np.zeros(max(n, 1), bs.BOWL_DTYPE)
            table = np.empty((rows, cols), np.int32) if labels else None
            self._check(self._lib.mrtx_bowls(self._ctx, C.byref(blk), None, z_h, o_d, o_h, wp, None, records.ctypes.data, n, None,
                                             table.ctypes.data if labels else None, C.byref(nb), C.byref(rounds), C.byref(st2)),
                        "mrtx_bowls")
            records = records[:n]
            z = z_keep
        self._add_stats(stats, st2)
        if isinstance(stats, dict):
            stats["rounds"] = stats.get("rounds", 0) + int(rounds.value)
            stats["bowls"] = stats.get("bowls", 0) + n
            stats["count_ms"] = stats.get("count_ms", 0.0) + st.kernel_ms
        return bs.BowlTree(records, table, z, unit_m, int(connectivity), bool(wrap), bool(invert))

    def peaks(self, heights, **kw):
        """bowls(invert=True): every summit with its key col (spill_at, spill_level), its prominence (floor_level -
        spill_level) and its parent peak."""
        kw["invert"] = True
        return self.bowls(heights, **kw)

    @staticmethod
    def _add_stats(acc, st, extra=None):
        """Sum the counters of one call into the dict `acc` (if it is one); extra = {key: MrtxStats field} of the call's own."""
        if isinstance(acc, dict):
            for k in ("shadow_rays", "height_samples", "dem_fetches", "mip_fetches", "kernel_ms", "launches"):
                acc[k] = acc.get(k, 0) + getattr(st, k)
            for k, field in (extra or {}).items():
                acc[k] = acc.get(k, 0) + int(getattr(st, field))

    @staticmethod
    def _chunks(n, per, chunk_bytes, out_bytes=4, empty_call=True):
        """The [a, b) point ranges of a point query's calls: each holds at most chunk_bytes and 2^31 outputs, `per` outputs of
        out_bytes per point (per = None: one call for all).  With N = 0 the query makes one call with no points when
        empty_call, which the library refuses (horizon, horizon_sun, surface_temperature, view_hits: an empty query is an
        error), and no call otherwise (illumination_series, line_of_sight: an empty result)."""
        step = max(n, 1) if per is None else max(1, min(int(chunk_bytes) // (out_bytes * per), (1 << 31) // per))
        return [(a, min(a + step, n)) for a in range(0, max(n, 1) if empty_call else n, step)]

    @staticmethod
    def _horizon_arg(horizon, n, n_az):
        """(n_az, at) of a `horizon` argument -- the (N, n_az) float32 array of MoonRT.horizon, or a DeviceBuffer holding it
        (then n_az is required) -- with at(a) = the (device, host) pointers of the horizons from point a on."""
        if isinstance(horizon, DeviceBuffer):
            if n_az is None:
                raise ValueError("n_az is required with a device buffer")
            n_az = int(n_az)
            if horizon.nbytes < n * n_az * 4:
                raise ValueError("the device buffer is smaller than N x n_az float32")
            return n_az, lambda a: (horizon.ptr + a * n_az * 4, None)
        hz = np.ascontiguousarray(horizon, np.float32)
        if hz.ndim != 2 or hz.shape[0] != n:
            raise ValueError("horizon must be an (N, n_az) array")
        return hz.shape[1], lambda a: (None, hz[a:].ctypes.data)

    def config(self):
        """The configuration the context runs with, defaults filled in (mrtx_get_config): device, width, height, rank, world,
        tile_w, tile_h."""
        cfg = MrtxConfig()
        self._check(self._lib.mrtx_get_config(self._ctx, C.byref(cfg)), "mrtx_get_config")
        return {name: int(getattr(cfg, name)) for name, _ in MrtxConfig._fields_}

    # ---- multi-GPU exchange
    def set_gather_hits(self, on):
        """Whether the hit buffer travels with the radiance in pack / unpack (mrtx_set_gather_hits; alike on every rank)."""
        self._check(self._lib.mrtx_set_gather_hits(self._ctx, 1 if on else 0), "mrtx_set_gather_hits")

    def shard_bytes(self, rank=None):
        n = C.c_uint64()
        self._check(self._lib.mrtx_shard_bytes(self._ctx, self.rank if rank is None else rank, C.byref(n)),
                    "mrtx_shard_bytes")
        return n.value

    def shard_bytes_active(self):
        """Bytes one rank's shard occupies for the scene as it stands (only tiles the sky cull keeps)."""
        n = C.c_uint64()
        self._check(self._lib.mrtx_shard_bytes_active(self._ctx, C.byref(n)), "mrtx_shard_bytes_active")
        return n.value

    def shard_parts(self, wanted):
        n = C.c_int32()
        self._check(self._lib.mrtx_shard_parts(self._ctx, int(wanted), C.byref(n)), "mrtx_shard_parts")
        return n.value

    def pack_part(self, dev_ptr, part, n_parts, stream=None):
        """Pack part `part` of the shard; returns (byte offset, byte length) of the piece inside the shard buffer."""
        off, ln = C.c_uint64(), C.c_uint64()
        self._check(self._lib.mrtx_pack_part(self._ctx, dev_ptr, int(part), int(n_parts), C.byref(off), C.byref(ln), stream),
                    "mrtx_pack_part")
        return off.value, ln.value

    def pack_shard(self, dev_ptr, stream=None):
        self._check(self._lib.mrtx_pack_shard(self._ctx, dev_ptr, stream), "mrtx_pack_shard")

    def unpack_shard(self, src_rank, dev_ptr, stream=None):
        self._check(self._lib.mrtx_unpack_shard(self._ctx, int(src_rank), dev_ptr, stream), "mrtx_unpack_shard")

    def unpack_all(self, dev_ptrs):
        """dev_ptrs[r] = device address of rank r's packed shard (entry 0 ignored); one sync for all peers."""
        arr = (C.c_void_p * len(dev_ptrs))(*[C.c_void_p(p) for p in dev_ptrs])
        self._check(self._lib.mrtx_unpack_all(self._ctx, arr, len(dev_ptrs)), "mrtx_unpack_all")

    def device_ptr(self, which):
        p, n = C.c_void_p(), C.c_uint64()
        self._check(self._lib.mrtx_device_ptr(self._ctx, which, C.byref(p), C.byref(n)), "mrtx_device_ptr")
        return p.value, n.value

    MIP_INFO = ("mip_shift", "mip_h", "mip_w", "m2_shift", "m2_h", "m2_w", "hm_shift", "hm_h", "hm_w")

    def mip_info(self):
        """The shifts and sizes of the march's skip structures (mrtx_mip_info) as a dict of MIP_INFO; all zero while nothing is
        built (before the first marching call, and again after a new DEM)."""
        out = (C.c_int32 * 9)()
        self._check(self._lib.mrtx_mip_info(self._ctx, out), "mrtx_mip_info")
        return dict(zip(self.MIP_INFO, (int(v) for v in out)))

    def read_structure(self, which):
        """A device structure the marches read, downloaded in its documented shape, or None while it
        does not exist: BUF_DEM (h+4, w+4, 2) float32, BUF_COLOR (h+1, w+4, 2) uint32, BUF_MIP (mip_h+2, mip_w+2, 2) float32,
        BUF_MIP2 (m2_h+2, m2_w+2) float32, BUF_HMIP (hm_h, hm_w) float32."""
        ptr, nbytes = self.device_ptr(which)
        if not ptr:
            return None
        i = self.mip_info()
        if which == _lib.BUF_DEM:
            h, w = self._dem_hw()
            dtype, shape = np.float32, (h + 4, w + 4, 2)
        elif which == _lib.BUF_COLOR:
            h, w = self._color_shape
            dtype, shape = np.uint32, (h + 1, w + 4, 2)
        elif which == _lib.BUF_MIP:
            dtype, shape = np.float32, (i["mip_h"] + 2, i["mip_w"] + 2, 2)
        elif which == _lib.BUF_MIP2:
            dtype, shape = np.float32, (i["m2_h"] + 2, i["m2_w"] + 2)
        elif which == _lib.BUF_HMIP:
            dtype, shape = np.float32, (i["hm_h"], i["hm_w"])
        else:
            raise ValueError(f"buffer {which} has no documented layout to read")
        out = np.empty(shape, dtype)
        if out.nbytes > nbytes:
            raise MoonRTError(f"buffer {which} holds {nbytes} bytes, its layout needs {out.nbytes}")
        rc = self._lib.mrtx_dev_download(self.config()["device"], out.ctypes.data, ptr, out.nbytes)
        if rc != 0:
            raise MoonRTError(f"device download failed (code {rc})")
        return out


# ---- context-free device helpers ------------------------------------------------------------------
def _err_call(fn, *args):
    lib = _lib.load()
    buf = C.create_string_buffer(256)
    rc = getattr(lib, fn)(*args, buf, 256)
    if rc != 0:
        raise MoonRTError(f"{fn} failed ({rc}): {buf.value.decode()}")


def synth_ldem(h, w, seed=0x4D525458, device=0):
    """Seeded synthetic int16 LDEM-like source, generated on the device."""
    buf = DeviceBuffer(h * w * 2, device)
    _err_call("mrtx_synth_ldem", device, buf.ptr, h, w, seed & 0xFFFFFFFF)
    return buf


def synth_color(h, w, seed=0x4D525458, device=0):
    buf = DeviceBuffer(h * w * 4, device)
    _err_call("mrtx_synth_color", device, buf.ptr, h, w, seed & 0xFFFFFFFF)
    return buf


def dem_from_ldem(src_buf, h, w, downscale=1, device=0):
    """Device restatement of load_elevation_data (data_loader.py:166-247).

    `src_buf` holds the int16 (h*downscale, w*downscale) source; returns (float32 DeviceBuffer (h, w),
    radius_scale)."""
    lib = _lib.load()
    dst = DeviceBuffer(h * w * 4, device)
    scale = C.c_float()
    buf = C.create_string_buffer(256)
    rc = lib.mrtx_dem_from_ldem(device, src_buf.ptr, h, w, downscale, dst.ptr, C.byref(scale), buf, 256)
    if rc != 0:
        raise MoonRTError(f"mrtx_dem_from_ldem failed ({rc}): {buf.value.decode()}")
    return dst, float(scale.value)


def probe_latlon(a, b, c, device=0):
    """Device evaluation of the renderer's (lat, lon) primitive for moon-frame points (a, b, c)."""
    lib = _lib.load()
    a, b, c = (np.ascontiguousarray(v, np.float32).ravel() for v in (a, b, c))
    lat = np.empty_like(a); lon = np.empty_like(a)
    rc = lib.mrtx_probe_latlon(device, a.ctypes.data, b.ctypes.data, c.ctypes.data, lat.ctypes.data,
                               lon.ctypes.data, a.size)
    if rc != 0:
        raise MoonRTError(f"mrtx_probe_latlon failed ({rc})")
    return lat, lon
