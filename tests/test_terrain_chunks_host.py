"""How the terrain queries of MoonRT split their work into library calls, without a GPU: the point chunks of
illumination_series, horizon, horizon_sun, surface_temperature, view_hits and line_of_sight (an uneven last chunk, N = 0)
and the bands of illumination_map and viewshed, through a fake library that fills every output row of a point with the
point's latitude (the tests use latitude = the point's index) and every map row with its row number."""
import ctypes as C

import numpy as np
import pytest

from moonrtx_amd import _lib
from moonrtx_amd import renderer as rmod
from moonrtx_amd.renderer import MoonRT, MoonRTError

E_INVALID = -1


class FakeBuffer:
    made = []

    def __init__(self, nbytes, device=0):
        self.nbytes, self.ptr, self.data, self.freed = int(nbytes), 0x1000 * (len(FakeBuffer.made) + 1), None, False
        FakeBuffer.made.append(self)

    def download(self, dtype, shape):
        return np.asarray(self.data, dtype).reshape(shape)

    def free(self):
        self.freed = True


def floats(addr, n):
    return np.ctypeslib.as_array((C.c_float * n).from_address(addr)) if n > 0 else np.zeros(0, np.float32)


class FakeLib:
    """The terrain entry points on the host: like the library they refuse n < 1; calls = (name, n, first latitude, ...)."""

    def __init__(self):
        self.calls = []

    def mrtx_last_error(self, ctx):
        return b"n must be >= 1"

    def mrtx_get_config(self, ctx, cfg):
        return 0

    def _points(self, name, pts, n, *more):
        self.calls.append((name, n, float(np.ctypeslib.as_array((C.c_double * 2).from_address(pts))[0]) if n > 0 else None)
                          + more)
        return n >= 1

    def _fill(self, host, n, width, st):
        floats(host, n * width).reshape(n, width)[:] = (self.calls[-1][2] + np.arange(n, dtype=np.float32))[:, None]
        st._obj.launches = 1

    def mrtx_illum_series(self, ctx, pts, n, ep, m, first, count, n_sun, dev, host, st):
        if not self._points("series", pts, n, count):
            return E_INVALID
        self._fill(host, n, 4 * count, st)
        return 0

    def mrtx_horizon_points(self, ctx, pts, n, n_az, n_bis, dev, host, st):
        if not self._points("horizon", pts, n, n_az):
            return E_INVALID
        self._fill(host, n, n_az, st)
        return 0

    def mrtx_horizon_sun(self, ctx, pts, n, n_az, dh, hh, ep, m, mode, dev, host, st):
        if not self._points("horizon_sun", pts, n, float(floats(hh, 1)[0]) if n > 0 else None):
            return E_INVALID
        self._fill(host, n, 4 if mode else m, st)
        return 0

    def mrtx_thermal(self, ctx, pts, n, n_az, dh, hh, ep, fl, m, model, mode, dev, host, st):
        if not self._points("thermal", pts, n, float(floats(hh, 1)[0]) if n > 0 else None):
            return E_INVALID
        self._fill(host, n, {0: m - model._obj.n_spin, 1: 4, 2: m}[mode], st)
        st._obj.reserved = 2
        return 0

    def mrtx_view_hits(self, ctx, pts, n, k, dev, host, st):
        if not self._points("view_hits", pts, n, k):
            return E_INVALID
        first = self.calls[-1][2]
        out = floats(host, n * (2 * k + 1))
        out[:2 * n * k] = np.repeat(first + np.arange(n, dtype=np.float32), 2 * k)
        out[2 * n * k:] = first + np.arange(n, dtype=np.float32)
        st._obj.launches, st._obj.bounce_rays = 1, n * k
        return 0

    def mrtx_sight_points(self, ctx, pts, n, obs, n_obs, th, mm, rm, nb, dev, host, st):
        if not self._points("sight", pts, n, n_obs):
            return E_INVALID
        self._fill(host, n, 1, st)
        return 0

    def _grid(self, name, gref, dev, host, st, width):
        g = gref._obj
        self.calls.append((name, g.row_begin, g.row_end, dev is not None))
        vals = np.repeat(np.arange(g.row_begin, g.row_end, dtype=np.float32), g.w * width)
        if host is not None:
            C.memmove(host, vals.ctypes.data, vals.nbytes)
        else:
            next(b for b in FakeBuffer.made if b.ptr == dev).data = vals.copy()
        st._obj.launches = 1
        return 0

    def mrtx_illum_grid(self, ctx, gref, dev, host, st):
        return self._grid("illum_grid", gref, dev, host, st, 4)

    def mrtx_sight_grid(self, ctx, gref, dev, host, st):
        return self._grid("sight_grid", gref, dev, host, st, 1)


@pytest.fixture
def rt(monkeypatch):
    FakeBuffer.made.clear()
    monkeypatch.setattr(rmod, "DeviceBuffer", FakeBuffer)
    r = MoonRT.__new__(MoonRT)
    r._lib = FakeLib()
    r._ctx = None
    return r


N = 7
LA, LO = np.arange(N, dtype=np.float64), np.zeros(N)
EP = np.zeros((5, 14))
ROWS = np.arange(N, dtype=np.float32)


def model(n_spin=2):
    md = _lib.MrtxThermalModel()
    md.n_spin = n_spin
    return md


def spans(rt, name):
    return [(c[1], c[2]) for c in rt._lib.calls if c[0] == name]


def test_illumination_series_chunks(rt):
    st = {}
    out = rt.illumination_series(LA, LO, EP, count=2, chunk_bytes=3 * 2 * 16, stats=st)     # 3 points of 2 float4 per call
    assert spans(rt, "series") == [(3, 0.0), (3, 3.0), (1, 6.0)] and st["launches"] == 3
    assert out.shape == (N, 2, 4) and np.array_equal(out[:, 0, 0], ROWS)
    rt._lib.calls.clear()
    assert rt.illumination_series([], [], EP, count=2).shape == (0, 2, 4) and not rt._lib.calls     # N = 0: no call


def test_horizon_chunks(rt):
    out = rt.horizon(LA, LO, n_az=4, chunk_bytes=3 * 4 * 4)
    assert spans(rt, "horizon") == [(3, 0.0), (3, 3.0), (1, 6.0)]
    assert np.array_equal(out, np.repeat(ROWS[:, None], 4, 1))
    rt._lib.calls.clear()
    with pytest.raises(MoonRTError):                   # N = 0: one call with no points, which the library refuses
        rt.horizon([], [], n_az=4)
    assert spans(rt, "horizon") == [(0, None)]


def test_horizon_sun_chunks_and_horizon_slices(rt):
    hz = np.repeat(ROWS[:, None], 4, 1)
    st = {}
    out = rt.horizon_sun(LA, LO, hz, EP, chunk_bytes=3 * 5 * 4, stats=st)                  # FULL: 3 points of 5 epochs
    assert [c[1:] for c in rt._lib.calls] == [(3, 0.0, 0.0), (3, 3.0, 3.0), (1, 6.0, 6.0)] and st["launches"] == 3
    assert np.array_equal(out, np.repeat(ROWS[:, None], 5, 1))
    rt._lib.calls.clear()
    assert rt.horizon_sun(LA, LO, hz, EP, summary=True, chunk_bytes=16).shape == (N, 4)       # SUMMARY: one call
    assert spans(rt, "horizon_sun") == [(N, 0.0)]
    rt._lib.calls.clear()
    with pytest.raises(MoonRTError):
        rt.horizon_sun([], [], np.zeros((0, 4), np.float32), EP, summary=True)
    assert spans(rt, "horizon_sun") == [(0, None)]
    with pytest.raises(ValueError):
        rt.horizon_sun(LA, LO, FakeBuffer(N * 16), EP)                                         # n_az missing
    with pytest.raises(ValueError):
        rt.horizon_sun(LA, LO, FakeBuffer(N * 16 - 4), EP, n_az=4)                             # too small
    with pytest.raises(ValueError):
        rt.horizon_sun(LA, LO, hz[1:], EP)


def test_surface_temperature_chunks(rt):
    hz = np.repeat(ROWS[:, None], 4, 1)
    st = {}
    out = rt.surface_temperature(LA, LO, hz, EP, np.ones(5), model(), mode="full", chunk_bytes=3 * 3 * 4, stats=st)
    assert [c[1:] for c in rt._lib.calls] == [(3, 0.0, 0.0), (3, 3.0, 3.0), (1, 6.0, 6.0)]
    assert np.array_equal(out, np.repeat(ROWS[:, None], 3, 1))
    assert st["launches"] == 3 and st["newton_cap_hits"] == 6
    rt._lib.calls.clear()
    out = rt.surface_temperature(LA, LO, hz, EP, np.ones(5), model(), mode="flux", chunk_bytes=2 * 5 * 4)
    assert spans(rt, "thermal") == [(2, 0.0), (2, 2.0), (2, 4.0), (1, 6.0)] and out.shape == (N, 5)
    rt._lib.calls.clear()
    assert rt.surface_temperature(LA, LO, hz, EP, np.ones(5), model(), chunk_bytes=16).shape == (N, 4)    # SUMMARY: one call
    assert spans(rt, "thermal") == [(N, 0.0)]
    rt._lib.calls.clear()
    with pytest.raises(MoonRTError):
        rt.surface_temperature([], [], np.zeros((0, 4), np.float32), EP, np.ones(5), model())
    assert spans(rt, "thermal") == [(0, None)]


def test_view_hits_chunks(rt):
    st = {}
    hits, share = rt.view_hits(LA, LO, k=16, chunk_bytes=3 * 33 * 4, stats=st)
    assert spans(rt, "view_hits") == [(3, 0.0), (3, 3.0), (1, 6.0)]
    assert hits.shape == (N, 16, 2) and np.array_equal(hits[:, :, 0], np.repeat(ROWS[:, None], 16, 1))
    assert np.array_equal(share, ROWS) and st["bounce_rays"] == N * 16 and st["launches"] == 3
    rt._lib.calls.clear()
    with pytest.raises(MoonRTError):
        rt.view_hits([], [], k=16)
    assert spans(rt, "view_hits") == [(0, None)]


def test_line_of_sight_chunks(rt):
    out = rt.line_of_sight(LA, LO, (0.0, 0.0, 0.0), chunk_bytes=12)
    assert spans(rt, "sight") == [(3, 0.0), (3, 3.0), (1, 6.0)] and np.array_equal(out, ROWS)
    rt._lib.calls.clear()
    assert rt.line_of_sight([], [], (0.0, 0.0, 0.0)).shape == (0,) and not rt._lib.calls


@pytest.mark.parametrize("which", ["illum", "sight"])
def test_maps_stream_bands_through_one_buffer(rt, which):
    call = (lambda **kw: rt.illumination_map(lat=(10, -10), lon=(0, 40), shape=(10, 6), **kw)) if which == "illum" else \
        (lambda **kw: rt.viewshed((1.0, 2.0, 3.0), lat=(10, -10), lon=(0, 40), shape=(10, 6), **kw))
    node = 16 if which == "illum" else 4
    st = {}
    whole = call(stats=st)
    assert rt._lib.calls == [(which + "_grid", 0, 10, False)] and st["launches"] == 1 and not FakeBuffer.made
    assert whole.shape[:2] == (10, 6) and np.array_equal(whole.reshape(10, -1)[:, 0], np.arange(10, dtype=np.float32))
    rt._lib.calls.clear()
    st = {}
    band = call(rows=(1, 10), band_bytes=4 * 6 * node, stats=st)           # 4 rows per band, the last one uneven
    assert [c[1:] for c in rt._lib.calls] == [(1, 5, True), (5, 9, True), (9, 10, True)] and st["launches"] == 3
    assert np.array_equal(band, whole[1:10])
    assert len(FakeBuffer.made) == 1 and FakeBuffer.made[0].freed and FakeBuffer.made[0].nbytes == 4 * 6 * node
