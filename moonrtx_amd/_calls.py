"""What every stage of the Python binding shares: the error type, the device allocation and the base class of the call
classes (terrain_calls.py, lattice_calls.py, renderer.py)."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import MrtxConfig


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


class Calls:
    """The plumbing of a class whose methods call the library on `self._lib` with the context `self._ctx`."""

    def _check(self, rc, what):
        if rc != 0:
            raise MoonRTError(f"{what} failed ({rc}): {self._lib.mrtx_last_error(self._ctx).decode()}")

    @staticmethod
    def _add_stats(acc, st, extra=None):
        """Sum the counters of one call into the dict `acc` (if it is one); extra = {key: MrtxStats field} of the call's own."""
        if isinstance(acc, dict):
            for k in ("shadow_rays", "height_samples", "dem_fetches", "mip_fetches", "kernel_ms", "launches"):
                acc[k] = acc.get(k, 0) + getattr(st, k)
            for k, field in (extra or {}).items():
                acc[k] = acc.get(k, 0) + int(getattr(st, field))

    def config(self):
        """The configuration the context runs with, defaults filled in (mrtx_get_config): device, width, height, rank, world,
        tile_w, tile_h."""
        cfg = MrtxConfig()
        self._check(self._lib.mrtx_get_config(self._ctx, C.byref(cfg)), "mrtx_get_config")
        return {name: int(getattr(cfg, name)) for name, _ in MrtxConfig._fields_}
