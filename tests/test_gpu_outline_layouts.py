"""The outline kernels on the MI355X against the built tables of tests/outline_layout_cases.py: every
table under contract and jump, at connectivity 4 and 8, in CORNERS and ALL mode, from a host and from a device label table, with
and without row weights, equal to tests/outline_model.py in every field and vertex; the number of launches from B and the variant
alone; the tables that fill the dead jump buffer also into the caller's own device tables, the same bytes; and the large table,
whose chunk sums take scan_chunks through a second and a third pass, against outlines composed from its pattern's.
tests/test_outline_layouts_host.py shows which edge each table holds and which defect of a kernel it would catch."""
import ctypes as C
import functools

import numpy as np
import pytest

import outline_cases as oc
import outline_layout_cases as lc
import outline_model as om
from moonrtx_amd import _lib
from moonrtx_amd import regions as rg
from moonrtx_amd.renderer import DeviceBuffer, MoonRT
from test_gpu_outline import assert_outlines_equal, each_variant, run  # noqa: F401  (each_variant is a fixture)

pytestmark = pytest.mark.gpu

NAMES = list(lc.tables())


@pytest.fixture(scope="module")
def rt(native_lib):
    """One context for the module, without a DEM, a light or a Moon frame: the stage needs none of them."""
    r = MoonRT(16, 16)
    yield r
    r.close()


@functools.lru_cache(maxsize=None)
def traced(name, conn, mode):
    labels, n, wrap = lc.tables()[name]
    return om.trace(labels, conn, wrap, mode, lc.weights_for(labels.shape[0]))


def launches_of(B, contract, fill, weighted):
    """3, then 8 or 4 and the rounds, then 2 or 3 for a fill call."""
    return 3 + (8 if contract else 4) + lc.rounds_of(B) + ((2 if weighted else 3) if fill else 0)


@pytest.mark.parametrize("name", NAMES)
def test_every_table_equals_the_model(rt, each_variant, name):
    labels, n, wrap = lc.tables()[name]
    labels = np.ascontiguousarray(labels)
    w = lc.weights_for(labels.shape[0])
    contract = each_variant == "contract"
    for conn in (4, 8):
        B = lc.layout(name, conn)["B"]
        for corners in (True, False):
            rings, vertices = traced(name, conn, om.CORNERS if corners else om.ALL)
            plain = rings.copy()
            plain["warea"] = plain["area"]
            for device in (False, True):
                for weights, want in ((w, rings), (None, plain)):
                    st = {}
                    got = run(rt, labels, n, conn, wrap, corners, weights, device, stats=st)
                    what = (name, each_variant, conn, corners, device, weights is not None)
                    assert_outlines_equal(got, want, vertices, what)
                    # the count call and the fill call
                    assert st["launches"] == launches_of(B, contract, False, False) + launches_of(B, contract, True, weights is not None), what


@pytest.mark.parametrize("name", lc.DEAD_BUFFER)
def test_the_dead_buffer_tables_into_the_callers_tables(rt, each_variant, name):
    """Rings of three sides in ALL mode: 48 B / 3 + 8 B bytes of host-bound tables in the 32 B bytes of the dead jump buffer, at
    an even and an odd number of rounds.  The caller's own device tables receive the same bytes."""
    labels, n, wrap = lc.tables()[name]
    labels = np.ascontiguousarray(labels)
    w = lc.weights_for(labels.shape[0])
    o = oc.block(*labels.shape, int(wrap), 4, _lib.OUTLINE_ALL)
    want_r, want_v = traced(name, 4, om.ALL)
    R, V = len(want_r), len(want_v)
    assert 48 * R + 8 * V == 24 * lc.layout(name, 4)["B"]
    host_r, host_v = np.zeros(R, rg.RING_DTYPE), np.zeros((V, 2), np.int32)
    nr, nv = C.c_uint64(0), C.c_uint64(0)
    assert oc.outline_call(rt._lib, rt._ctx, o, labels, n=n, weights=w, rings=host_r, ring_cap=R, vertices=host_v, vertex_cap=V,
                           counts=(nr, nv)) == 0, rt._lib.mrtx_last_error(rt._ctx)
    assert (nr.value, nv.value) == (R, V)
    assert_outlines_equal(rg.Outlines(host_r, host_v, *labels.shape, wrap), want_r, want_v, (name, each_variant, "host tables"))
    rb, vb = DeviceBuffer(48 * R), DeviceBuffer(8 * V)
    try:
        assert oc.outline_call(rt._lib, rt._ctx, o, labels, n=n, weights=w, dev_rings=rb.ptr, ring_cap=R, dev_vertices=vb.ptr,
                               vertex_cap=V, counts=(nr, nv)) == 0, rt._lib.mrtx_last_error(rt._ctx)
        assert rb.download(rg.RING_DTYPE, (R,)).tobytes() == host_r.tobytes()
        assert vb.download(np.int32, (V, 2)).tobytes() == host_v.tobytes()
    finally:
        rb.free()
        vb.free()


# ---- the large table
@pytest.fixture(scope="module")
def large(native_lib):
    """The large table on the device, uploaded once."""
    labels = lc.large_labels(lc.LARGE_TILING)
    buf = DeviceBuffer(labels.size * 4)
    buf.upload(np.ascontiguousarray(labels, np.int32))
    yield labels.shape, buf
    buf.free()


@functools.lru_cache(maxsize=None)
def composed(conn, weighted):
    return lc.compose(lc.LARGE_TILING, conn, om.CORNERS, lc.LARGE_WEIGHT if weighted else None)


@pytest.mark.parametrize("weighted", [False, True], ids=["no weights", "one weight"])
@pytest.mark.parametrize("conn", [4, 8])
def test_the_large_table_equals_its_composed_outlines(rt, large, each_variant, conn, weighted):
    """1141 chunks of nodes and 2086 chunks of sides: scan_chunks' carry links two passes over the nodes and three over the
    chains and the heads.  CORNERS mode, labels on the device, 23 rounds."""
    (rows, cols), buf = large
    nodes, B, n_rings = lc.large_counts(lc.LARGE_TILING, conn)
    assert nodes == rows * cols and lc.n_chunks(nodes) > lc.PASS and lc.n_chunks(B) > 2 * lc.PASS
    want_r, want_v = composed(conn, weighted)
    assert len(want_r) == n_rings and int(want_r["n_sides"].astype(np.int64).sum()) == B
    w = np.full(rows, lc.LARGE_WEIGHT, np.uint32) if weighted else None
    contract = each_variant == "contract"
    o = oc.block(rows, cols, 0, conn, _lib.OUTLINE_CORNERS)
    nr, nv = C.c_uint64(0), C.c_uint64(0)
    st = _lib.MrtxStats()
    assert oc.outline_call(rt._lib, rt._ctx, o, dev_labels=buf.ptr, n=7, weights=w, counts=(nr, nv), st=st) == 0, \
        rt._lib.mrtx_last_error(rt._ctx)
    assert (nr.value, nv.value) == (len(want_r), len(want_v))                  # the count call returns the composed totals
    assert st.launches == launches_of(B, contract, False, weighted) == 3 + (8 if contract else 4) + 23
    rb, vb = DeviceBuffer(48 * len(want_r)), DeviceBuffer(8 * len(want_v))
    try:
        assert oc.outline_call(rt._lib, rt._ctx, o, dev_labels=buf.ptr, n=7, weights=w, dev_rings=rb.ptr, ring_cap=len(want_r),
                               dev_vertices=vb.ptr, vertex_cap=len(want_v), counts=(nr, nv), st=st) == 0, rt._lib.mrtx_last_error(rt._ctx)
        assert st.launches == launches_of(B, contract, True, weighted)
        got = rg.Outlines(rb.download(rg.RING_DTYPE, (len(want_r),)), vb.download(np.int32, (len(want_v), 2)), rows, cols, False)
    finally:
        rb.free()
        vb.free()
    assert_outlines_equal(got, want_r, want_v, ("the large table", each_variant, conn, weighted))
