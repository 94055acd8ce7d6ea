"""What the host and the GPU tests of mrtx_occultation and mrtx_horizon_passes share: the raw calls and the lists of refusals.
A list is [(a pattern of the refusal's text, whether the case needs a displacement map, keyword arguments of the call)]: a
case that needs none is refused before the call looks for the DEM, so it gives its own text on a machine without a GPU too.
dev is the address of device memory, 16-byte aligned, or any such number where no device is present: no case gets as far as
writing to it."""
import ctypes as C
import re

import numpy as np

from moonrtx_amd import _lib

LAUNCHES = 77                   # what a call's statistics block holds before the call: a refusal leaves it there


def _ptr(a):
    return None if a is None else a.ctypes.data


def refused(lib, ctx, code, st, text):
    """One refusal: the code, the text, and the statistics block as it was."""
    assert code == -1 and st.launches == LAUNCHES, (text, code, st.launches)
    msg = lib.mrtx_last_error(ctx).decode()
    assert re.search(text, msg), (text, msg)


# ---- mrtx_occultation
def occult_call(lib, ctx, p, n, src, body, m, mode, dev_out, host):
    """mrtx_occultation with arrays (or None) for the tables and integers for the outputs: (code, statistics block)."""
    st = _lib.MrtxStats()
    st.launches = LAUNCHES
    rc = lib.mrtx_occultation(ctx, _ptr(p), n, _ptr(src), _ptr(body), m, mode, dev_out, host, C.byref(st))
    return rc, st


def occult_base(pts, far, earth, out):
    """A good FULL call: pts (2, 2) float64, far and earth (m, 14) float64 epoch tables, out (2, m) float32."""
    return dict(p=pts, n=2, src=far, body=earth, m=far.shape[0], mode=0, dev_out=None, host=out.ctypes.data)


def occult_refusals(pts, far, earth, out, radius, dev):
    """radius: the Moon's, in the units of the tables."""
    base = occult_base(pts, far, earth, out)
    m = base["m"]

    def edit(table, col, value, k=5):
        t = table.copy()
        t[k, col] = value
        return t

    def case(text, needs_dem=False, **kw):
        return text, needs_dem, dict(base, **kw)
    cases = [case("null point list or epoch table", src=None), case("null point list or epoch table", body=None),
             case("null point list or epoch table", p=None),
             case("n and m must be >= 1 \\(got 2, 0\\)", m=0), case("n and m must be >= 1 \\(got 2, -3\\)", m=-3),
             case("n and m must be >= 1 \\(got 0, %d\\)" % m, n=0)]
    for col in (0, 3, 4, 6, 9, 12):             # light_pos, light_radius, light_radiance, center, u, v
        text = "epoch 5: bad light" if col < 5 else "epoch 5: bad moon frame"
        for bad in (float("nan"), float("inf")):
            cases += [case(text, True, src=edit(far, col, bad)), case(text, True, body=edit(earth, col, bad))]
    near = earth.copy()                         # the body's centre 1.5 Moon radii from the Moon's, its own radius 3.67
    near[5, 0:3] = near[5, 5:8] + (near[5, 0:3] - near[5, 5:8]) * (1.5 * radius / np.linalg.norm(near[5, 0:3] - near[5, 5:8]))
    cases += [case("epoch 5: bad light", True, src=edit(far, 3, -1.0)),
              case("epoch 5: the body's radius must be > 0", True, body=edit(earth, 3, 0.0)),
              case("epoch 5: bad light", True, body=edit(earth, 3, -2.0)),
              case("epoch 5: the body reaches into the Moon's bounding sphere", True, body=near),
              case("is not nearer than the source", True, src=earth, body=far)]     # the body beyond the source
    cases += [case("mode must be 0 \\(FULL\\) or 1 \\(SUMMARY\\) \\(got %d\\)" % mode, mode=mode) for mode in (-1, 2, 7)]
    cases += [case("give exactly one of dev_out and host_out", host=None),
              case("give exactly one of dev_out and host_out", dev_out=dev),
              case("dev_out must be 16-byte aligned", mode=1, dev_out=dev + 4, host=None),
              case("point 0: latitude must lie in \\[-90, 90\\]", True, p=np.array([[91.0, 0.0], [0.0, 0.0]])),
              case("at most 2\\^24 epochs per call \\(got 16777217\\)", m=(1 << 24) + 1)]
    return cases


# ---- mrtx_horizon_passes
def passes_call(lib, ctx, k, lat, lon, hz, pos, dev_out, host_out, cap, total, st, heights=None, dev_hz=None):
    """mrtx_horizon_passes with arrays for the tables and integers for the outputs; total: a c_uint64 or None."""
    pts = np.ascontiguousarray(np.stack([lat, lon], -1))
    keep = (pts, np.ascontiguousarray(pos, np.float64), np.ascontiguousarray(hz, np.float32))
    return lib.mrtx_horizon_passes(ctx, C.byref(k), pts.ctypes.data, _ptr(heights), lat.size, hz.shape[1], dev_hz,
                                   None if dev_hz else keep[2].ctypes.data, keep[1].ctypes.data, dev_out, host_out, cap,
                                   None if total is None else C.byref(total), C.byref(st))


def passes_block(n_sat=3, m=16, mode=_lib.PASSES_SUMMARY, reserved=0, radius_m=1737400.0, min_elev_deg=0.0):
    return _lib.MrtxPasses(n_sat, m, mode, reserved, radius_m, min_elev_deg)


def passes_refusals(pos, out, dev):
    """pos (3, 16, 3) float64 positions in metres, all outside the bounding sphere; out (4, 8) float32: four points.  The
    keyword arguments are those of passes_call after the horizon table."""
    R_m = passes_block().radius_m
    block = passes_block
    H = out.ctypes.data

    def case(text, needs_dem=False, k=None, pos_=pos, dev_out=None, host_out=H, cap=0, heights=None):
        return text, needs_dem, dict(k=k or block(), pos=pos_, dev_out=dev_out, host_out=host_out, cap=cap, heights=heights)
    inside, near = pos.copy(), pos.copy()
    inside[1, 7] = pos[1, 7] / np.linalg.norm(pos[1, 7]) * (1.0005 * R_m)
    near[1, 7] = pos[1, 7] / np.linalg.norm(pos[1, 7]) * (1.004 * R_m)   # outside the sphere, but not outside it plus 10 km
    cases = [case("satellite 1, epoch 7: the position lies within the Moon's bounding sphere", True, pos_=inside),
             case("satellite 1, epoch 7: the position lies within the Moon's bounding sphere", True, pos_=near,
                  heights=np.full(4, 1e4))]
    for bad in (np.nan, np.inf):
        broken = pos.copy()
        broken[2, 3, 1] = bad
        cases.append(case("satellite 2, epoch 3: the position is not finite", True, pos_=broken))
    FULL, LIST = _lib.PASSES_FULL, _lib.PASSES_LIST
    cases += [
        case("n_sat \\* m at most 2\\^24 \\(got 256 x 65537\\)", k=block(256, (1 << 16) + 1)),    # before the table is read
        case("mode must be 0 \\(FULL\\), 1 \\(SUMMARY\\) or 2 \\(LIST\\) \\(got 3\\)", k=block(mode=3)),
        case("mode must be 0 \\(FULL\\), 1 \\(SUMMARY\\) or 2 \\(LIST\\) \\(got -1\\)", k=block(mode=-1)),
        case("give at most one of dev_out and host_out", dev_out=dev),
        case("give exactly one of dev_out and host_out", host_out=None),
        case("give exactly one of dev_out and host_out", k=block(mode=FULL), host_out=None),
        case("dev_out must be 16-byte aligned", dev_out=dev + 4, host_out=None),
        case("dev_out must be 16-byte aligned", k=block(mode=FULL), dev_out=dev + 8, host_out=None),
        case("dev_out must be 8-byte aligned", k=block(mode=LIST), dev_out=dev + 4, host_out=None, cap=100),
        case("without a table pass_cap must be 0 \\(got 5\\)", k=block(mode=LIST), host_out=None, cap=5),
        case("n_sat must lie in \\[1, 256\\] \\(got 0\\)", k=block(n_sat=0)),
        case("reserved must be 0", k=block(reserved=1)),
        case("radius_m must be finite and > 0", k=block(radius_m=0.0)),
        case("min_elev_deg must lie in \\[-90, 90\\)", k=block(min_elev_deg=90.0)),
        case("point 2: height must lie in \\[0, 1e4\\] m", True, heights=np.array([0.0, 1.0, 2e4, 0.0])),
    ]
    return cases
