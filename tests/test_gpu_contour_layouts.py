"""The contour kernels on the MI355X against the built tables of tests/contour_layout_cases.py: every
table from a host and from a device height table, equal to tests/contour_model.py in every field and vertex; the number of
launches from B alone; and the large table, whose chunk sums take scan_nodes_kernel and scan_chunks_kernel through a second
and a third pass, against lines composed from its patches', unwrapped and wrapped, into the caller's own device tables.
tests/test_contour_layouts_host.py shows which edge each table holds and which defect of a kernel it would catch."""
import ctypes as C
import functools

import numpy as np
import pytest

import contour_cases as cc
import contour_layout_cases as lc
from moonrtx_amd import _lib
from moonrtx_amd.renderer import DeviceBuffer, MoonRT
from test_gpu_contour import LINE, assert_contours_equal, run

pytestmark = pytest.mark.gpu

NAMES = list(lc.tables())


@pytest.fixture(scope="module")
def rt(native_lib):
    """One context for the module, without a DEM, a light or a Moon frame: the stage needs none of them."""
    r = MoonRT(16, 16)
    yield r
    r.close()


def launches_of(B, fill):
    """3 of the count; then 5 and the rounds of the trace, and 2 more for a fill call."""
    return 3 + (5 + lc.rounds_of(B) + (2 if fill else 0) if B else 0)


@pytest.mark.parametrize("name", NAMES)
def test_every_table_equals_the_model(rt, name):
    z, levels, wrap = lc.tables()[name]
    z = np.ascontiguousarray(z)
    lines, vertices = lc.traced(name)
    B = len(vertices)
    assert B == lc.layout(name)["B"]
    # the count call alone
    nl, nv = C.c_uint64(77), C.c_uint64(77)
    st = _lib.MrtxStats()
    k = cc.block(*z.shape, int(wrap), len(levels))
    assert cc.contour_call(rt._lib, rt._ctx, k, z, levels=np.ascontiguousarray(levels), counts=(nl, nv), st=st) == 0, \
        rt._lib.mrtx_last_error(rt._ctx)
    assert (nl.value, nv.value) == (len(lines), B) and st.launches == launches_of(B, False), name
    # the count call and the fill call, from a host and from a device table
    for device in (False, True):
        stats = {}
        got = run(rt, z, levels, wrap, device, stats=stats)
        assert_contours_equal(got, lines, vertices, (name, device))
        assert stats["launches"] == launches_of(B, False) + launches_of(B, True), (name, device)


# ---- the large table
@pytest.fixture(scope="module")
def large(native_lib):
    """The large table on the device, uploaded once."""
    z = lc.large_z(lc.LARGE_TILING)
    buf = DeviceBuffer(z.size * 4)
    buf.upload(np.ascontiguousarray(z, np.int32))
    yield z.shape, buf
    buf.free()


@functools.lru_cache(maxsize=None)
def composed():
    return lc.compose(lc.LARGE_TILING)


@pytest.mark.parametrize("wrap", [False, True], ids=["unwrapped", "wrapped"])
def test_the_large_table_equals_its_composed_lines(rt, large, wrap):
    """More than 2048 chunks of nodes and of elements: the carries of scan_nodes_kernel and of scan_chunks_kernel link three
    passes and more.  Heights on the device, the caller's own device tables sized exactly; the seam cells are all zero, so the
    wrapped table has the same lines."""
    (rows, cols), buf = large
    c = lc.large_counts(lc.LARGE_TILING)
    assert c["nodes"] == rows * cols and lc.n_chunks(c["nodes"]) > 2 * lc.PASS and lc.n_chunks(c["B"]) > 2 * lc.PASS
    want_l, want_v = composed()
    L, V = len(want_l), len(want_v)
    assert (L, V) == (c["lines"], c["B"]) and int((want_l["closed"] == 0).sum()) == c["open_lines"] > 0
    k = cc.block(rows, cols, int(wrap), len(lc.LARGE_LEVELS))
    nl, nv = C.c_uint64(0), C.c_uint64(0)
    st = _lib.MrtxStats()
    assert cc.contour_call(rt._lib, rt._ctx, k, dev_z=buf.ptr, levels=lc.LARGE_LEVELS, counts=(nl, nv), st=st) == 0, \
        rt._lib.mrtx_last_error(rt._ctx)
    assert (nl.value, nv.value) == (L, V)                                       # the count call returns the composed totals
    assert st.launches == launches_of(V, False) == 3 + 5 + c["rounds"]
    lb, vb = DeviceBuffer(32 * L), DeviceBuffer(4 * V)
    try:
        assert cc.contour_call(rt._lib, rt._ctx, k, dev_z=buf.ptr, levels=lc.LARGE_LEVELS, dev_lines=lb.ptr, line_cap=L,
                               dev_vertices=vb.ptr, vertex_cap=V, counts=(nl, nv), st=st) == 0, rt._lib.mrtx_last_error(rt._ctx)
        assert (nl.value, nv.value) == (L, V) and st.launches == launches_of(V, True)
        got_l, got_v = lb.download(LINE, (L,)), vb.download(np.int32, (V,))
    finally:
        lb.free()
        vb.free()
    for name in LINE.names:
        bad = np.flatnonzero(got_l[name] != want_l[name])
        assert bad.size == 0, (wrap, name, int(bad[0]), got_l[bad[0]], want_l[bad[0]])
    bad = np.flatnonzero(got_v != want_v)
    assert bad.size == 0, (wrap, "vertex", int(bad[0]), int(got_v[bad[0]]), int(want_v[bad[0]]))
