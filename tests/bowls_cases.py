"""What the host and the GPU tests of mrtx_bowls share: the raw call, the list of refusals and the built lattices.  A built case
is (z, conn, wrap, edge_outlets, table or None), as in fill_cases."""
import ctypes as C
import re

import numpy as np

from moonrtx_amd import _lib
from moonrtx_amd import basins as bs

WALL = 5000


def block(rows=8, cols=9, wrap=0, conn=8, edge=1, invert=0, reserved=(0, 0)):
    return _lib.MrtxBowls(rows, cols, wrap, conn, edge, invert, (C.c_int32 * 2)(*reserved))


def _ptr(a):
    return None if a is None else a.ctypes.data


def bowls_call(lib, ctx, b, z=None, dev_z=None, outlet=None, dev_outlet=None, weights=None, bowls=None, dev_bowls=None, cap=0,
               label=None, dev_label=None, n=None, rounds=None, st=None, block=True):
    """mrtx_bowls with numpy arrays for the host tables and integers for the device tables."""
    return lib.mrtx_bowls(ctx, C.byref(b) if block else None, dev_z, _ptr(z), dev_outlet, _ptr(outlet), _ptr(weights), dev_bowls,
                          _ptr(bowls), cap, dev_label, _ptr(label), C.byref(n) if n is not None else None,
                          C.byref(rounds) if rounds is not None else None, C.byref(st) if st is not None else None)


def refusal_tables():
    """(z (8, 9), outlet (8, 9), records (4,), labels (8, 9)): the host tables of the refusal cases, zeroed."""
    return np.zeros((8, 9), np.int32), np.zeros((8, 9), np.uint8), np.zeros(4, bs.BOWL_DTYPE), np.zeros((8, 9), np.int32)


def refusals(z, outlet, bowls, label, dev):
    """[(a pattern of the refusal's text, keyword arguments of bowls_call)]; dev: the address of 16384 bytes of device memory, or
    any 16-byte aligned number where no device is present: no case gets as far as reading it."""
    F = dict(z=z, bowls=bowls, cap=4, label=label)
    D = dict(dev_z=dev, dev_outlet=dev + 512, dev_bowls=dev + 1024, cap=4, dev_label=dev + 2048)
    hi, lo = z.copy(), z.copy()
    hi[3, 4], lo[7, 8] = 2 ** 30 + 1, -2 ** 30 - 1
    return [
        ("null bowls block", dict(F, b=block(), block=False)),
        ("reserved must be 0", dict(F, b=block(reserved=(1, 0)))),
        ("reserved must be 0", dict(F, b=block(reserved=(0, -1)))),
        ("empty lattice", dict(F, b=block(rows=0))),
        ("empty lattice", dict(F, b=block(cols=-3))),
        ("at most 2\\^31 nodes", dict(F, b=block(rows=65536, cols=32769))),
        ("wrap must be 0 or 1", dict(F, b=block(wrap=2))),
        ("cols >= 3", dict(F, b=block(cols=2, wrap=1))),
        ("connectivity must be 4 or 8", dict(F, b=block(conn=6))),
        ("edge_outlets must be 0 or 1", dict(F, b=block(edge=2))),
        ("invert must be 0 or 1 \\(got 2\\)", dict(F, b=block(invert=2))),
        ("invert must be 0 or 1 \\(got -1\\)", dict(F, b=block(invert=-1))),
        ("at most one of dev_outlet and host_outlet", dict(F, b=block(), outlet=outlet, dev_outlet=dev)),
        ("no outlet source", dict(F, b=block(edge=0))),
        ("exactly one of dev_z and host_z", dict(F, b=block(), z=None)),
        ("exactly one of dev_z and host_z", dict(F, b=block(), dev_z=dev)),
        ("null n_bowls", dict(F, b=block(), n=None)),
        ("at most one of dev_bowls and host_bowls", dict(F, b=block(), dev_bowls=dev)),
        ("at most one of dev_label and host_label", dict(F, b=block(), dev_label=dev)),
        ("without a bowl table bowl_cap must be 0 \\(got 4\\)", dict(F, b=block(), bowls=None, label=None)),
        ("a label table needs a bowl table", dict(F, b=block(), bowls=None, cap=0)),
        ("dev_z must be 4-byte aligned", dict(D, b=block(), dev_z=dev + 2)),
        ("dev_bowls must be 8-byte aligned", dict(D, b=block(), dev_bowls=dev + 1028)),
        ("dev_label must be 4-byte aligned", dict(D, b=block(), dev_label=dev + 2049)),
        ("must not overlap", dict(D, b=block(), dev_outlet=dev + 284)),
        ("must not overlap", dict(D, b=block(), dev_bowls=dev + 280)),
        ("must not overlap", dict(D, b=block(), dev_label=dev + 284)),
        ("must not overlap", dict(D, b=block(), dev_bowls=dev + 512 + 64)),
        ("must not overlap", dict(D, b=block(), dev_label=dev + 512 + 68)),
        ("must not overlap", dict(D, b=block(), dev_label=dev + 1024 + 252)),
        ("height 31 must lie in -2\\^30 .. 2\\^30 \\(got 1073741825\\)", dict(F, b=block(), z=hi)),
        ("height 71 must lie in -2\\^30 .. 2\\^30 \\(got -1073741825\\)", dict(F, b=block(), z=lo)),
    ]


def assert_refused(lib, ctx, text, kw, untouched):
    """One refusal: the code, the text, n_bowls, rounds and the statistics as they were, the host outputs untouched."""
    st = _lib.MrtxStats()
    st.launches, st.kernel_ms = 0xABCD, -7.0
    n, rounds = C.c_uint64(5), C.c_uint64(6)
    kw = dict(dict(n=n, rounds=rounds), **kw)
    assert bowls_call(lib, ctx, st=st, **kw) == -1, text
    msg = lib.mrtx_last_error(ctx).decode()
    assert re.search(text, msg), (text, msg)
    assert n.value == 5 and rounds.value == 6, text
    assert st.launches == 0xABCD and st.kernel_ms == -7.0, text
    for a in untouched:
        assert (a.view(np.uint8) == 0).all(), text


# ---- built lattices
def one_outlet(shape, at):
    t = np.zeros(shape, np.uint8)
    t[at] = 1
    return t


def serpentine(n, conn, wrap=False):
    """Walls everywhere but a channel one node wide along the odd rows, joined at alternating ends, whose heights fall by one
    from node to node down to the lattice's only outlet at its far end: one descent path through every tile, wave and row
    border.  Every 37th node of it is a pit 50 deep.  wrap: the columns rolled, so that the channel crosses the seam twice in
    every row."""
    z = np.full((n, n), WALL, np.int32)
    path = []
    rows = list(range(1, n - 1, 2))
    for k, i in enumerate(rows):
        cols = list(range(1, n - 1))
        if k % 2:
            cols.reverse()
        path += [(i, j) for j in cols]
        if k + 1 < len(rows):
            path.append((i + 1, cols[-1]))
    for k, at in enumerate(path):
        z[at] = len(path) - k - (50 if k % 37 == 5 else 0)
    t = one_outlet((n, n), path[-1])
    if wrap:
        z, t = np.roll(z, n // 2 + 5, 1), np.roll(t, n // 2 + 5, 1)
    return np.ascontiguousarray(z), conn, wrap, False, np.ascontiguousarray(t)


def staircase(pits, conn):
    """A row of pits between walls that rise from left to right, inside a lattice of high walls, the only outlet beyond the last
    and highest wall: pit 0 spills into pit 1, the two together into pit 2, and so on.  The chain of parents above the first
    leaf holds every meta bowl, `pits` - 1 of them."""
    cols = 2 * pits + 1
    z = np.full((5, cols), WALL, np.int32)
    for k in range(pits):
        z[2, 2 * k] = -100 - 3 * k
        z[2, 2 * k + 1] = 7 * k
    z[2, cols - 1] = 7 * pits
    return z, conn, False, False, one_outlet(z.shape, (2, cols - 1))


def pit_grid(n, seed):
    """Pits with random floors at every odd (row, column), walls of random height between them: (n / 2)^2 minima inside a ring of
    edge outlets."""
    rng = np.random.default_rng(seed)
    z = rng.integers(100, 200, (n, n)).astype(np.int32)
    z[1::2, 1::2] = rng.integers(0, 50, z[1::2, 1::2].shape)
    return z, 8, False, True, None


def random_case(seed, rows, cols, conn, wrap, lo, hi, table_share=0.0, edge=True):
    rng = np.random.default_rng(seed)
    z = rng.integers(lo, hi + 1, (rows, cols)).astype(np.int32)
    t = (rng.random((rows, cols)) < table_share).astype(np.uint8) if table_share else None
    return z, conn, wrap, edge, t
