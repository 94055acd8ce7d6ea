"""What the host and the GPU tests of mrtx_fill and mrtx_fill_basins share: the raw calls, the list of refusals and the built
lattices.  A built case is (z, conn, wrap, edge_outlets, table or None)."""
import ctypes as C
import re

import numpy as np

from moonrtx_amd import _lib
from moonrtx_amd import basins as bs

WALL = 1000


def block(rows=8, cols=9, wrap=0, conn=8, edge=1, reserved=0):
    return _lib.MrtxFill(rows, cols, wrap, conn, edge, reserved)


def _ptr(a):
    return None if a is None else a.ctypes.data


def fill_call(lib, ctx, f, z=None, dev_z=None, outlet=None, dev_outlet=None, fill=None, dev_fill=None, visits=None, st=None,
              block=True):
    """mrtx_fill with numpy arrays for the host tables and integers for the device tables."""
    return lib.mrtx_fill(ctx, C.byref(f) if block else None, dev_z, _ptr(z), dev_outlet, _ptr(outlet), dev_fill, _ptr(fill),
                         C.byref(visits) if visits is not None else None, C.byref(st) if st is not None else None)


def basins_call(lib, ctx, rows=8, cols=9, wrap=0, conn=8, labels=None, dev_labels=None, n=1, z=None, dev_z=None, fill=None,
                dev_fill=None, weights=None, out=None, dev_out=None, st=None):
    return lib.mrtx_fill_basins(ctx, rows, cols, wrap, conn, dev_labels, _ptr(labels), n, dev_z, _ptr(z), dev_fill, _ptr(fill),
                                _ptr(weights), dev_out, _ptr(out), C.byref(st) if st is not None else None)


def refusal_tables():
    """(z (8, 9), outlet (8, 9), fill (8, 9), labels (8, 9), records (4,)): the host tables of the refusal cases, zeroed."""
    return (np.zeros((8, 9), np.int32), np.zeros((8, 9), np.uint8), np.zeros((8, 9), np.int32), np.zeros((8, 9), np.int32),
            np.zeros(4, bs.BASIN_DTYPE))


def fill_refusals(z, outlet, fill, dev):
    """[(a pattern of the refusal's text, keyword arguments of fill_call)]; dev: the address of 8192 bytes of device memory, or
    any 16-byte aligned number where no device is present: no case gets as far as reading it."""
    F = dict(z=z, fill=fill)
    D = dict(dev_z=dev, dev_fill=dev + 512, dev_outlet=dev + 1024)
    hi, lo = z.copy(), z.copy()
    hi[3, 4], lo[7, 8] = 2 ** 30 + 1, -2 ** 30 - 1
    return [
        ("null fill block", dict(F, f=block(), block=False)),
        ("reserved must be 0", dict(F, f=block(reserved=1))),
        ("empty lattice", dict(F, f=block(rows=0))),
        ("empty lattice", dict(F, f=block(cols=-3))),
        ("at most 2\\^31 nodes", dict(F, f=block(rows=65536, cols=32769))),
        ("wrap must be 0 or 1", dict(F, f=block(wrap=2))),
        ("cols >= 3", dict(F, f=block(cols=2, wrap=1))),
        ("connectivity must be 4 or 8", dict(F, f=block(conn=6))),
        ("edge_outlets must be 0 or 1", dict(F, f=block(edge=2))),
        ("edge_outlets must be 0 or 1", dict(F, f=block(edge=-1))),
        ("at most one of dev_outlet and host_outlet", dict(F, f=block(), outlet=outlet, dev_outlet=dev)),
        ("no outlet source", dict(F, f=block(edge=0))),
        ("exactly one of dev_z and host_z", dict(F, f=block(), z=None)),
        ("exactly one of dev_z and host_z", dict(F, f=block(), dev_z=dev)),
        ("exactly one of dev_fill and host_fill", dict(F, f=block(), fill=None)),
        ("exactly one of dev_fill and host_fill", dict(F, f=block(), dev_fill=dev)),
        ("dev_z must be 4-byte aligned", dict(D, f=block(), dev_z=dev + 2)),
        ("dev_fill must be 4-byte aligned", dict(D, f=block(), dev_fill=dev + 513)),
        ("must not overlap", dict(D, f=block(), dev_fill=dev + 284)),
        ("must not overlap", dict(D, f=block(), dev_outlet=dev + 284)),
        ("must not overlap", dict(D, f=block(), dev_outlet=dev + 512 + 284)),
        ("height 31 must lie in -2\\^30 .. 2\\^30 \\(got 1073741825\\)", dict(F, f=block(), z=hi)),
        ("height 71 must lie in -2\\^30 .. 2\\^30 \\(got -1073741825\\)", dict(F, f=block(), z=lo)),
    ]


def basins_refusals(labels, z, fill, out, dev):
    F = dict(labels=labels, z=z, fill=fill, out=out)
    D = dict(dev_labels=dev, dev_z=dev + 512, dev_fill=dev + 1024, dev_out=dev + 1536)
    hi = z.copy()
    hi[0, 2] = 2 ** 30 + 1
    return [
        ("empty lattice", dict(F, rows=0)),
        ("at most 2\\^31 nodes", dict(F, rows=65536, cols=32769)),
        ("wrap must be 0 or 1", dict(F, wrap=-1)),
        ("cols >= 3", dict(F, cols=2, wrap=1)),
        ("connectivity must be 4 or 8", dict(F, conn=0)),
        ("exactly one of dev_labels and host_labels", dict(F, labels=None)),
        ("exactly one of dev_labels and host_labels", dict(F, dev_labels=dev)),
        ("exactly one of dev_z and host_z", dict(F, z=None)),
        ("exactly one of dev_z and host_z", dict(F, dev_z=dev)),
        ("exactly one of dev_fill and host_fill", dict(F, fill=None)),
        ("exactly one of dev_fill and host_fill", dict(F, dev_fill=dev)),
        ("exactly one of dev_out and host_out", dict(F, out=None)),
        ("exactly one of dev_out and host_out", dict(F, dev_out=dev)),
        ("exceeds the lattice", dict(F, n=73)),
        ("dev_labels must be 4-byte aligned", dict(D, dev_labels=dev + 2)),
        ("dev_z must be 4-byte aligned", dict(D, dev_z=dev + 513)),
        ("dev_fill must be 4-byte aligned", dict(D, dev_fill=dev + 1027)),
        ("dev_out must be 8-byte aligned", dict(D, dev_out=dev + 1540)),
        ("must not overlap", dict(D, n=4, dev_out=dev + 280)),
        ("must not overlap", dict(D, n=4, dev_out=dev + 512 + 280)),
        ("must not overlap", dict(D, n=4, dev_out=dev + 1024 + 280)),
        ("height 2 must lie in -2\\^30 .. 2\\^30", dict(F, z=hi)),
    ]


def assert_refused(lib, ctx, call, text, kw, untouched):
    """One refusal: the code, the text, visits and the statistics as they were, the host outputs untouched."""
    st = _lib.MrtxStats()
    st.launches, st.kernel_ms = 0xABCD, -7.0
    kw = dict(kw, st=st)
    visits = None
    if call is fill_call:
        visits = C.c_uint64(5)
        kw["visits"] = visits
    assert call(lib, ctx, **kw) == -1, text
    msg = lib.mrtx_last_error(ctx).decode()
    assert re.search(text, msg), (text, msg)
    assert visits is None or visits.value == 5, text
    assert st.launches == 0xABCD and st.kernel_ms == -7.0, text
    for a in untouched:
        assert (a.view(np.uint8) == 0).all(), text


# ---- built lattices
def one_outlet(shape, at):
    t = np.zeros(shape, np.uint8)
    t[at] = 1
    return t


def serpentine(n, conn, transposed=False):
    """Walls everywhere but a channel one node wide: along the odd rows, joined at alternating ends, from a pit at its head to
    the lattice's only outlet at its far end, of height 5.  The channel crosses every tile border; every node of it fills to 5."""
    z = np.full((n, n), WALL, np.int32)
    rows = list(range(1, n - 1, 2))
    for k, i in enumerate(rows):
        z[i, 1:n - 1] = 0
        if k + 1 < len(rows):
            z[i + 1, n - 2 if k % 2 == 0 else 1] = 0
    z[1, 1] = -10
    last = rows[-1]
    end = (last, 1 if len(rows) % 2 == 0 else n - 2)
    z[end] = 5
    t = one_outlet((n, n), end)
    if transposed:
        z, t = np.ascontiguousarray(z.T), np.ascontiguousarray(t.T)
    return z, conn, False, False, t


def diagonal(n, conn, kind):
    """A channel along the main diagonal, the anti-diagonal or, wrapped, j = (i + n / 2) mod n: its nodes touch at their corners
    only, so it drains at connectivity 8 (through the tiles' corners, across the seam) and not at 4.  The outlet, of height 5,
    is the channel's last node; the table is the only outlet source."""
    z = np.full((n, n), WALL, np.int32)
    i = np.arange(n)
    j = {"main": i, "anti": n - 1 - i, "wrapped": (i + n // 2) % n}[kind]
    z[i, j] = 0
    z[0, j[0]] = -10
    z[n - 1, j[n - 1]] = 5
    return z, conn, kind == "wrapped", False, one_outlet((n, n), (n - 1, int(j[n - 1])))


def flat(rows, cols, conn, wrap=False):
    return np.full((rows, cols), 3, np.int32), conn, wrap, True, None


def flat_basin(n, conn):
    """One flat floor inside a rim of height 100 on the lattice's edge, with a single notch of height 7 in the rim."""
    z = np.zeros((n, n), np.int32)
    z[0, :] = z[-1, :] = z[:, 0] = z[:, -1] = 100
    z[n // 2 + 3, n - 1] = 7
    return z, conn, False, True, None


def checkerboard(rows, cols, conn, wrap=False):
    i, j = np.indices((rows, cols))
    return np.where((i + j) % 2 == 0, 0, 10).astype(np.int32), conn, wrap, True, None


def random_case(seed, rows, cols, conn, wrap, lo, hi, table_share=0.0, edge=True):
    rng = np.random.default_rng(seed)
    z = rng.integers(lo, hi + 1, (rows, cols)).astype(np.int32)
    t = (rng.random((rows, cols)) < table_share).astype(np.uint8) if table_share else None
    return z, conn, wrap, edge, t
