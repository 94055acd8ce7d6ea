"""What the host and the GPU tests of mrtx_regions_outline share: the raw call and the list of refusals."""
import ctypes as C

import numpy as np

from moonrtx_amd import _lib
from moonrtx_amd import regions as rg


def block(rows=8, cols=9, wrap=0, conn=4, mode=1, reserved=0):
    return _lib.MrtxOutline(rows, cols, wrap, conn, mode, reserved)


def outline_call(lib, ctx, o, labels=None, dev_labels=None, n=1, weights=None, dev_rings=None, rings=None, ring_cap=0,
                 dev_vertices=None, vertices=None, vertex_cap=0, counts=None, block=True, st=None):
    """mrtx_regions_outline with numpy arrays for the host tables and integers for the device tables."""
    ptr = lambda a: None if a is None else a.ctypes.data
    nr, nv = counts if counts is not None else (C.c_uint64(0), C.c_uint64(0))
    return lib.mrtx_regions_outline(ctx, C.byref(o) if block else None, dev_labels, ptr(labels), n, ptr(weights), dev_rings,
                                    ptr(rings), ring_cap, dev_vertices, ptr(vertices), vertex_cap,
                                    C.byref(nr) if nr is not None else None, C.byref(nv) if nv is not None else None,
                                    C.byref(st) if st is not None else None)


def refusal_tables():
    """(labels (8, 9), rings (4,), vertices (16, 2)): the host tables of the refusal cases, zeroed."""
    return np.zeros((8, 9), np.int32), np.zeros(4, rg.RING_DTYPE), np.zeros((16, 2), np.int32)


def refusal_cases(labels, rings, vertices, dev):
    """[(a pattern of the refusal's text, keyword arguments of outline_call)]; dev: the address of 8192 bytes of device memory, or
    any 16-byte aligned number where no device is present: no case gets as far as reading it."""
    F = dict(labels=labels, rings=rings, ring_cap=4, vertices=vertices, vertex_cap=16)
    D = dict(dev_labels=dev, dev_rings=dev + 512, ring_cap=4, dev_vertices=dev + 1024, vertex_cap=16)
    return [
        ("null outline block", dict(F, o=block(), block=False)),
        ("reserved must be 0", dict(F, o=block(reserved=1))),
        ("empty lattice", dict(F, o=block(rows=0))),
        ("empty lattice", dict(F, o=block(cols=-3))),
        ("at most 2\\^31 nodes", dict(F, o=block(rows=65536, cols=32769))),
        ("at most 2\\^28 nodes", dict(F, o=block(rows=16384, cols=16385))),
        ("wrap must be 0 or 1", dict(F, o=block(wrap=2))),
        ("cols >= 3", dict(F, o=block(cols=2, wrap=1))),
        ("connectivity must be 4 or 8", dict(F, o=block(conn=6))),
        ("mode must be MRTX_OUTLINE_ALL or MRTX_OUTLINE_CORNERS", dict(F, o=block(mode=2))),
        ("mode must be MRTX_OUTLINE_ALL or MRTX_OUTLINE_CORNERS", dict(F, o=block(mode=-1))),
        ("exactly one of dev_labels and host_labels", dict(F, o=block(), labels=None)),
        ("exactly one of dev_labels and host_labels", dict(F, o=block(), dev_labels=dev)),
        ("null n_rings or n_vertices", dict(F, o=block(), counts=(None, C.c_uint64(5)))),
        ("null n_rings or n_vertices", dict(F, o=block(), counts=(C.c_uint64(5), None))),
        ("at most one of dev_rings and host_rings", dict(F, o=block(), dev_rings=dev)),
        ("at most one of dev_vertices and host_vertices", dict(F, o=block(), dev_vertices=dev)),
        ("a ring table and a vertex table, or neither", dict(F, o=block(), rings=None)),
        ("a ring table and a vertex table, or neither", dict(F, o=block(), vertices=None)),
        ("without tables ring_cap and vertex_cap must be 0", dict(labels=labels, o=block(), ring_cap=1)),
        ("without tables ring_cap and vertex_cap must be 0", dict(labels=labels, o=block(), vertex_cap=1)),
        ("exceeds the lattice", dict(F, o=block(), n=73)),
        ("dev_labels must be 4-byte aligned", dict(D, o=block(), dev_labels=dev + 2)),
        ("dev_rings must be 8-byte aligned", dict(D, o=block(), dev_rings=dev + 516)),
        ("dev_vertices must be 4-byte aligned", dict(D, o=block(), dev_vertices=dev + 1026)),
        ("must not overlap", dict(D, o=block(), dev_rings=dev + 280)),
        ("must not overlap", dict(D, o=block(), dev_vertices=dev + 284)),
        ("must not overlap", dict(D, o=block(), dev_vertices=dev + 512 + 184)),
    ]


def assert_refused(lib, ctx, text, kw, rings, vertices):
    """One refusal: the code, the text, the counts and the statistics as they were, the host tables untouched."""
    import re
    kw = dict(kw)
    nr, nv = kw.pop("counts", (C.c_uint64(5), C.c_uint64(5)))
    st = _lib.MrtxStats()
    st.launches, st.kernel_ms = 0xABCD, -7.0
    assert outline_call(lib, ctx, counts=(nr, nv), st=st, **kw) == -1, text
    msg = lib.mrtx_last_error(ctx).decode()
    assert re.search(text, msg), (text, msg)
    assert (nr is None or nr.value == 5) and (nv is None or nv.value == 5), text
    assert st.launches == 0xABCD and st.kernel_ms == -7.0, text
    assert (rings.view(np.uint8) == 0).all() and (vertices == 0).all(), text
