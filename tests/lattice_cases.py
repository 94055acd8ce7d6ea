"""What the host and the GPU tests of mrtx_regions_label, mrtx_regions_stats, mrtx_regions_zonal, mrtx_regions_shape,
mrtx_proximity and mrtx_regions_reach share: the raw calls and the lists of refusals.  A list is [(a pattern of the refusal's
text, keyword arguments of the call)]; dev and dev2 are the addresses of 8192 bytes of device memory each, or any two 16-byte
aligned numbers 8192 apart where no device is present: no case gets as far as reading them."""
import ctypes as C
import math
import re

import numpy as np

from moonrtx_amd import _lib

INF = math.inf
CMAX = 2 ** 29


def _ptr(a):
    return None if a is None else a.ctypes.data


def refused(lib, ctx, code, text):
    """One refusal: the code and the text."""
    assert code == -1, text
    msg = lib.mrtx_last_error(ctx).decode()
    assert re.search(text, msg), (text, msg)


# ---- mrtx_regions_label and mrtx_regions_stats
def regions_block(rows=8, cols=9, wrap=0, conn=4, n_ch=1, ch=0, lo=-INF, hi=INF, reserved=0):
    return _lib.MrtxRegions(rows, cols, wrap, conn, n_ch, ch, lo, hi, reserved)


def label_call(lib, ctx, r, dev_field=None, host_field=None, dev_mask=None, host_mask=None, dev_labels=None, host_labels=None,
               n=None, block=True):
    """mrtx_regions_label with integers for every table."""
    st = _lib.MrtxStats()
    return lib.mrtx_regions_label(ctx, C.byref(r) if block else None, dev_field, host_field, dev_mask, host_mask, dev_labels,
                                  host_labels, n, C.byref(st))


def label_refusals(mask, field, labels, n, dev, dev2):
    """mask (8, 9) uint8, field (8, 9) float32, labels (8, 9) int32, n: a c_uint32."""
    block = regions_block
    M, F, L = mask.ctypes.data, field.ctypes.data, labels.ctypes.data
    N = C.byref(n)
    return [
        ("null regions block", dict(r=block(), host_mask=M, host_labels=L, n=N, block=False)),
        ("reserved must be 0", dict(r=block(reserved=1), host_mask=M, host_labels=L, n=N)),
        ("empty lattice", dict(r=block(rows=0), host_mask=M, host_labels=L, n=N)),
        ("empty lattice", dict(r=block(cols=-3), host_mask=M, host_labels=L, n=N)),
        ("at most 2\\^31 nodes", dict(r=block(rows=65536, cols=32769), host_mask=M, host_labels=L, n=N)),
        ("wrap must be 0 or 1", dict(r=block(wrap=2), host_mask=M, host_labels=L, n=N)),
        ("cols >= 3", dict(r=block(cols=2, wrap=1), host_mask=M, host_labels=L, n=N)),
        ("connectivity must be 4 or 8", dict(r=block(conn=6), host_mask=M, host_labels=L, n=N)),
        ("exactly one of a field and a mask", dict(r=block(), host_mask=M, host_field=F, host_labels=L, n=N)),
        ("exactly one of a field and a mask", dict(r=block(), dev_mask=dev, host_field=F, host_labels=L, n=N)),
        ("exactly one of a field and a mask", dict(r=block(), host_labels=L, n=N)),
        ("exactly one of dev_field and host_field", dict(r=block(), dev_field=dev, host_field=F, host_labels=L, n=N)),
        ("exactly one of dev_mask and host_mask", dict(r=block(), dev_mask=dev, host_mask=M, host_labels=L, n=N)),
        ("exactly one of dev_labels and host_labels", dict(r=block(), host_mask=M, n=N)),
        ("exactly one of dev_labels and host_labels", dict(r=block(), host_mask=M, host_labels=L, dev_labels=dev, n=N)),
        ("null n_regions", dict(r=block(), host_mask=M, host_labels=L)),
        ("n_ch must lie in 1 .. 16", dict(r=block(n_ch=0), host_field=F, host_labels=L, n=N)),
        ("n_ch must lie in 1 .. 16", dict(r=block(n_ch=17), host_field=F, host_labels=L, n=N)),
        ("ch must lie in", dict(r=block(n_ch=2, ch=2), host_field=F, host_labels=L, n=N)),
        ("ch must lie in", dict(r=block(ch=-1), host_field=F, host_labels=L, n=N)),
        ("lo must be <= hi", dict(r=block(lo=1.0, hi=0.5), host_field=F, host_labels=L, n=N)),
        ("must not be NaN", dict(r=block(lo=math.nan), host_field=F, host_labels=L, n=N)),
        ("must not be NaN", dict(r=block(hi=math.nan), host_field=F, host_labels=L, n=N)),
        ("dev_field must be 4-byte aligned", dict(r=block(), dev_field=dev + 2, dev_labels=dev2, n=N)),
        ("dev_labels must be 4-byte aligned", dict(r=block(), dev_mask=dev, dev_labels=dev2 + 1, n=N)),
        ("must not overlap", dict(r=block(), dev_mask=dev, dev_labels=dev + 68, n=N)),
        ("must not overlap", dict(r=block(), dev_field=dev + 4, dev_labels=dev, n=N)),
    ]


def stats_call(lib, ctx, rows=8, cols=9, wrap=0, dev_labels=None, host_labels=None, n_regions=4, dev_out=None, host_out=None):
    return lib.mrtx_regions_stats(ctx, rows, cols, wrap, dev_labels, host_labels, n_regions, None, dev_out, host_out, None)


def stats_refusals(labels, table, dev):
    """labels (8, 9) int32, table: four records of REGION_DTYPE."""
    L, T = labels.ctypes.data, table.ctypes.data
    return [
        ("empty lattice", dict(rows=0, host_labels=L, host_out=T)),
        ("cols >= 3", dict(cols=2, wrap=1, host_labels=L, host_out=T)),
        ("wrap must be 0 or 1", dict(wrap=-1, host_labels=L, host_out=T)),
        ("exactly one of dev_labels and host_labels", dict(host_out=T)),
        ("exactly one of dev_labels and host_labels", dict(dev_labels=dev, host_labels=L, host_out=T)),
        ("exactly one of dev_out and host_out", dict(host_labels=L)),
        ("exactly one of dev_out and host_out", dict(host_labels=L, dev_out=dev, host_out=T)),
        ("exceeds the lattice", dict(host_labels=L, host_out=T, n_regions=73)),
        ("dev_labels must be 4-byte aligned", dict(dev_labels=dev + 2, host_out=T)),
        ("dev_out must be 8-byte aligned", dict(host_labels=L, dev_out=dev + 4)),
        ("must not overlap", dict(dev_labels=dev, dev_out=dev + 280)),
    ]


# ---- mrtx_regions_zonal and mrtx_regions_shape
def zonal_spec(rows=8, cols=9, wrap=0, n_ch=1, scale=1.0, hist_ch=0, n_bins=0, lo=0.0, inv_w=1.0, reserved=0):
    return _lib.MrtxZonalSpec(rows, cols, wrap, n_ch, scale, hist_ch, n_bins, lo, inv_w, reserved)


def zonal_call(lib, ctx, z, labels=None, dev_labels=None, n=1, field=None, dev_field=None, weights=None, dev_out=None, out=None,
               dev_hist=None, hist=None, block=True):
    """mrtx_regions_zonal with numpy arrays for the host tables and integers for the device tables."""
    return lib.mrtx_regions_zonal(ctx, C.byref(z) if block else None, dev_labels, _ptr(labels), n, dev_field, _ptr(field),
                                  _ptr(weights), dev_out, _ptr(out), dev_hist, _ptr(hist), None)


def zonal_refusals(labels, field, out, hist, dev, dev2):
    """labels (8, 9) int32, field (8, 9) float32, out: four records of ZONAL_DTYPE, hist: 4 x 6 uint64."""
    spec = zonal_spec
    base = dict(labels=labels, field=field, out=out, n=4)
    H = dict(base, hist=hist)
    return [
        ("null zonal block", dict(base, z=spec(), block=False)),
        ("reserved must be 0", dict(base, z=spec(reserved=1))),
        ("empty lattice", dict(base, z=spec(rows=0))),
        ("empty lattice", dict(base, z=spec(cols=-3))),
        ("at most 2\\^31 nodes", dict(base, z=spec(rows=65536, cols=32769))),
        ("wrap must be 0 or 1", dict(base, z=spec(wrap=2))),
        ("cols >= 3", dict(base, z=spec(cols=2, wrap=1))),
        ("n_ch must lie in 1 .. 16", dict(base, z=spec(n_ch=0))),
        ("n_ch must lie in 1 .. 16", dict(base, z=spec(n_ch=17))),
        ("scale must be finite and > 0", dict(base, z=spec(scale=0.0))),
        ("scale must be finite and > 0", dict(base, z=spec(scale=-1.0))),
        ("scale must be finite and > 0", dict(base, z=spec(scale=INF))),
        ("scale must be finite and > 0", dict(base, z=spec(scale=math.nan))),
        ("n_bins must lie in 0 .. 4096", dict(H, z=spec(n_bins=-1))),
        ("n_bins must lie in 0 .. 4096", dict(H, z=spec(n_bins=4097))),
        ("hist_ch must lie in", dict(H, z=spec(n_bins=4, hist_ch=1))),
        ("hist_ch must lie in", dict(H, z=spec(n_bins=4, hist_ch=-1))),
        ("hist_lo must be finite", dict(H, z=spec(n_bins=4, lo=INF))),
        ("hist_lo must be finite", dict(H, z=spec(n_bins=4, lo=math.nan))),
        ("hist_inv_w finite and > 0", dict(H, z=spec(n_bins=4, inv_w=0.0))),
        ("hist_inv_w finite and > 0", dict(H, z=spec(n_bins=4, inv_w=-2.0))),
        ("hist_inv_w finite and > 0", dict(H, z=spec(n_bins=4, inv_w=INF))),
        ("exactly one of dev_labels and host_labels", dict(base, z=spec(), labels=None)),
        ("exactly one of dev_labels and host_labels", dict(base, z=spec(), dev_labels=dev)),
        ("exactly one of dev_field and host_field", dict(base, z=spec(), field=None)),
        ("exactly one of dev_field and host_field", dict(base, z=spec(), dev_field=dev)),
        ("exactly one of dev_out and host_out", dict(base, z=spec(), out=None)),
        ("exactly one of dev_out and host_out", dict(base, z=spec(), dev_out=dev)),
        ("without bins dev_hist and host_hist must be NULL", dict(H, z=spec())),
        ("without bins dev_hist and host_hist must be NULL", dict(base, z=spec(), dev_hist=dev)),
        ("exactly one of dev_hist and host_hist", dict(base, z=spec(n_bins=4))),
        ("exactly one of dev_hist and host_hist", dict(H, z=spec(n_bins=4), dev_hist=dev)),
        ("exceeds the lattice", dict(base, z=spec(), n=73)),
        ("at most 2\\^28 columns", dict(H, z=spec(rows=32768, cols=32768, n_bins=4094), n=65537)),
        ("dev_labels must be 4-byte aligned", dict(base, z=spec(), labels=None, dev_labels=dev + 2)),
        ("dev_field must be 4-byte aligned", dict(base, z=spec(), field=None, dev_field=dev + 1)),
        ("dev_out must be 8-byte aligned", dict(base, z=spec(), out=None, dev_out=dev + 4)),
        ("dev_hist must be 8-byte aligned", dict(base, z=spec(n_bins=4), dev_hist=dev + 4)),
        ("must not overlap", dict(base, z=spec(), labels=None, dev_labels=dev, out=None, dev_out=dev + 280)),
        ("must not overlap", dict(base, z=spec(), field=None, dev_field=dev + 8, out=None, dev_out=dev)),
        ("must not overlap", dict(base, z=spec(n_bins=4), labels=None, dev_labels=dev, dev_hist=dev + 8)),
        ("must not overlap", dict(base, z=spec(n_bins=4), field=None, dev_field=dev2, dev_hist=dev2 + 8)),
        ("must not overlap", dict(base, z=spec(n_bins=4), out=None, dev_out=dev2, dev_hist=dev2 + 216)),
    ]


def shape_call(lib, ctx, rows=8, cols=9, wrap=0, conn=4, dev_labels=None, host_labels=None, n=4, side_ew=None, side_ns=None,
               dev_out=None, host_out=None):
    return lib.mrtx_regions_shape(ctx, rows, cols, wrap, conn, dev_labels, _ptr(host_labels), n, _ptr(side_ew), _ptr(side_ns),
                                  dev_out, _ptr(host_out), None)


def shape_refusals(labels, shape_out, dev):
    """labels (8, 9) int32, shape_out: four records of SHAPE_DTYPE."""
    ew, ns = np.ones(8, np.uint32), np.ones(9, np.uint32)
    S = dict(host_labels=labels, host_out=shape_out)
    return [
        ("empty lattice", dict(S, rows=0)),
        ("at most 2\\^31 nodes", dict(S, rows=65536, cols=32769)),
        ("wrap must be 0 or 1", dict(S, wrap=-1)),
        ("cols >= 3", dict(S, cols=2, wrap=1)),
        ("connectivity must be 4 or 8", dict(S, conn=6)),
        ("exactly one of dev_labels and host_labels", dict(S, host_labels=None)),
        ("exactly one of dev_labels and host_labels", dict(S, dev_labels=dev)),
        ("exactly one of dev_out and host_out", dict(S, host_out=None)),
        ("exactly one of dev_out and host_out", dict(S, dev_out=dev)),
        ("both of side_ew and side_ns or neither", dict(S, side_ew=ew)),
        ("both of side_ew and side_ns or neither", dict(S, side_ns=ns)),
        ("exceeds the lattice", dict(S, n=73)),
        ("dev_labels must be 4-byte aligned", dict(S, host_labels=None, dev_labels=dev + 2)),
        ("dev_out must be 8-byte aligned", dict(S, host_out=None, dev_out=dev + 4)),
        ("must not overlap", dict(host_labels=None, dev_labels=dev, dev_out=dev + 280)),
    ]


# ---- mrtx_proximity and mrtx_regions_reach
def prox_call(lib, ctx, p="default", pos=None, labels=None, near=None, d2=None, dev_pos=None, dev_labels=None, dev_near=None,
              dev_d2=None, pairs=None, st=None):
    if isinstance(p, str):
        p = _lib.MrtxProximity(8, 9, 0, 0)
    return lib.mrtx_proximity(ctx, None if p is None else C.byref(p), dev_pos, _ptr(pos), dev_labels, _ptr(labels), dev_near,
                              _ptr(near), dev_d2, _ptr(d2), None if pairs is None else C.byref(pairs),
                              None if st is None else C.byref(st))


def prox_device_tables(dev):
    """The four device tables of an 8 x 9 lattice in one block: 864, 288, 288 and 576 bytes."""
    return dict(dev_pos=dev, dev_labels=dev + 1024, dev_near=dev + 2048, dev_d2=dev + 4096)


def prox_off_positions(pos):
    """pos (8, 9, 3) int32 with the last coordinate of the last node one past the bound."""
    off = pos.copy()
    off[7, 8, 2] = CMAX + 1
    return off


def prox_refusals(pos, labels, near, d2, dev):
    """pos (8, 9, 3) int32 within the bound, labels and near (8, 9) int32, d2 (8, 9) uint64."""
    P = _lib.MrtxProximity
    base = dict(pos=pos, labels=labels, near=near, d2=d2)
    D = prox_device_tables(dev)
    off = prox_off_positions(pos)
    low = pos.copy()
    low[0, 0, 0] = -CMAX - 1
    return [
        ("null proximity block", dict(base, p=None)),
        ("empty lattice", dict(base, p=P(0, 9, 0, 0))),
        ("empty lattice", dict(base, p=P(8, -1, 0, 0))),
        ("at most 2\\^31 nodes", dict(base, p=P(65536, 32769, 0, 0))),
        ("mode must be", dict(base, p=P(8, 9, 2, 0))),
        ("mode must be", dict(base, p=P(8, 9, -1, 0))),
        ("reserved must be 0", dict(base, p=P(8, 9, 0, 1))),
        ("exactly one of dev_pos and host_pos", dict(base, pos=None)),
        ("exactly one of dev_pos and host_pos", dict(base, dev_pos=dev)),
        ("exactly one of dev_labels and host_labels", dict(base, labels=None)),
        ("exactly one of dev_labels and host_labels", dict(base, dev_labels=dev)),
        ("exactly one of dev_nearest and host_nearest", dict(base, near=None)),
        ("exactly one of dev_nearest and host_nearest", dict(base, dev_near=dev)),
        ("exactly one of dev_dist2 and host_dist2", dict(base, d2=None)),
        ("exactly one of dev_dist2 and host_dist2", dict(base, dev_d2=dev)),
        ("dev_dist2 must be 8-byte aligned", dict(base, d2=None, dev_d2=dev + 4)),
        ("dev_pos must be 4-byte aligned", dict(base, pos=None, dev_pos=dev + 2)),
        ("dev_labels must be 4-byte aligned", dict(base, labels=None, dev_labels=dev + 1)),
        ("dev_nearest must be 4-byte aligned", dict(base, near=None, dev_near=dev + 2)),
        ("must not overlap", dict(D, dev_labels=dev + 860)),
        ("must not overlap", dict(D, dev_near=dev + 1024 + 284)),
        ("must not overlap", dict(D, dev_d2=dev + 2048 + 280)),
        ("must not overlap", dict(D, dev_d2=dev + 8)),
        ("must not overlap", dict(D, dev_near=dev + 4096 + 572)),
        ("must not overlap", dict(D, dev_labels=dev + 4096)),
        ("coordinate 2 of node 71 must lie in -2\\^29 .. 2\\^29", dict(base, pos=off)),
        ("coordinate 0 of node 0 must lie in -2\\^29 .. 2\\^29", dict(base, pos=low)),
    ]


def reach_call(lib, ctx, rows, cols, labels=None, n=1, d2=None, near=None, out=None, dev_labels=None, dev_d2=None, dev_near=None,
               dev_out=None, st=None):
    return lib.mrtx_regions_reach(ctx, rows, cols, dev_labels, _ptr(labels), n, dev_d2, _ptr(d2), dev_near, _ptr(near), dev_out,
                                  _ptr(out), None if st is None else C.byref(st))


def reach_refusals(labels, d2, near, out, dev):
    """labels and near (8, 9) int32, d2 (8, 9) uint64, out: four records of REACH_DTYPE.  Every case on 8 x 9 nodes unless it
    says otherwise."""
    R = dict(labels=labels, d2=d2, near=near, out=out, n=4)
    cases = [
        ("empty lattice", dict(R, rows=0)),
        ("at most 2\\^31 nodes", dict(R, rows=65536, cols=32769)),
        ("exactly one of dev_labels and host_labels", dict(R, labels=None)),
        ("exactly one of dev_labels and host_labels", dict(R, dev_labels=dev)),
        ("exactly one of dev_dist2 and host_dist2", dict(R, d2=None)),
        ("exactly one of dev_dist2 and host_dist2", dict(R, dev_d2=dev)),
        ("exactly one of dev_nearest and host_nearest", dict(R, near=None)),
        ("exactly one of dev_nearest and host_nearest", dict(R, dev_near=dev)),
        ("exactly one of dev_out and host_out", dict(R, out=None)),
        ("exactly one of dev_out and host_out", dict(R, dev_out=dev)),
        ("exceeds the lattice", dict(R, n=73)),
        ("dev_labels must be 4-byte aligned", dict(R, labels=None, dev_labels=dev + 2)),
        ("dev_dist2 must be 8-byte aligned", dict(R, d2=None, dev_d2=dev + 4)),
        ("dev_nearest must be 4-byte aligned", dict(R, near=None, dev_near=dev + 1)),
        ("dev_out must be 8-byte aligned", dict(R, out=None, dev_out=dev + 4)),
        ("must not overlap", dict(R, labels=None, dev_labels=dev, out=None, dev_out=dev + 280)),
        ("must not overlap", dict(R, d2=None, dev_d2=dev + 64, out=None, dev_out=dev)),
        ("must not overlap", dict(R, near=None, dev_near=dev + 120, out=None, dev_out=dev)),
    ]
    return [(text, dict(dict(rows=8, cols=9), **kw)) for text, kw in cases]
