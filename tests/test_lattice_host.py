"""The refusals of the region calls without a GPU (mrtx_regions_label, mrtx_regions_stats, mrtx_regions_zonal, mrtx_regions_shape,
mrtx_proximity, mrtx_regions_reach): every refusal of the GPU tests' lists comes before the first device call, so on a machine
without a GPU each still gives its own text, and so do the unknown values of the three variant switches."""
import ctypes as C

import numpy as np
import pytest

import lattice_cases as lc
from moonrtx_amd import _lib
from moonrtx_amd import regions as rg

BASE = 1 << 40                  # never dereferenced: a device call with it, or without a device, would not give -1
DEV, DEV2 = BASE, BASE + 8192


@pytest.fixture
def ctx(native_lib):
    """A context handle; without a GPU mrtx_create stops at its first HIP call but hands the context out."""
    c = C.c_void_p()
    rc = native_lib.mrtx_create(C.byref(_lib.MrtxConfig(0, 16, 16, 0, 1, 0, 0)), C.byref(c))
    assert rc in (0, -2) and c.value
    yield c
    native_lib.mrtx_destroy(c)


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    for name in ("MOONRT_REGIONS_CATALOGUE", "MOONRT_REGIONS_ZONAL", "MOONRT_PROXIMITY"):
        monkeypatch.delenv(name, raising=False)


def test_a_null_context_is_refused_without_a_text(native_lib):
    assert native_lib.mrtx_regions_label(None, None, None, None, None, None, None, None, None, None) == -1
    assert native_lib.mrtx_regions_stats(None, 8, 9, 0, None, None, 0, None, None, None, None) == -1
    assert native_lib.mrtx_regions_zonal(None, None, None, None, 0, None, None, None, None, None, None, None, None) == -1
    assert native_lib.mrtx_regions_shape(None, 8, 9, 0, 4, None, None, 0, None, None, None, None, None) == -1
    assert native_lib.mrtx_proximity(None, None, None, None, None, None, None, None, None, None, None, None) == -1
    assert native_lib.mrtx_regions_reach(None, 8, 9, None, None, 0, None, None, None, None, None, None, None) == -1


def test_label_and_stats_refusals_come_before_any_device_call(native_lib, ctx, monkeypatch):
    mask = np.ones((8, 9), np.uint8)
    field = np.ones((8, 9), np.float32)
    labels = np.full((8, 9), 7, np.int32)
    n = C.c_uint32(4321)
    for text, kw in lc.label_refusals(mask, field, labels, n, DEV, DEV2):
        lc.refused(native_lib, ctx, lc.label_call(native_lib, ctx, **kw), text)
        assert n.value == 4321 and (labels == 7).all(), text
    table = np.zeros(4, rg.REGION_DTYPE)
    for text, kw in lc.stats_refusals(labels, table, DEV):
        lc.refused(native_lib, ctx, lc.stats_call(native_lib, ctx, **kw), text)
        assert (table.view(np.uint8) == 0).all(), text
    # an unknown value of the variant switch, by name; the two known ones are not refused for it
    L, T = labels.ctypes.data, table.ctypes.data
    for bad in ("fast", "", "Plain"):
        monkeypatch.setenv("MOONRT_REGIONS_CATALOGUE", bad)
        lc.refused(native_lib, ctx, lc.stats_call(native_lib, ctx, host_labels=L, host_out=T),
                   "MOONRT_REGIONS_CATALOGUE must be runs or plain \\(got %s\\)" % bad)
    for good in ("runs", "plain"):
        monkeypatch.setenv("MOONRT_REGIONS_CATALOGUE", good)
        lc.refused(native_lib, ctx, lc.stats_call(native_lib, ctx, host_labels=L, host_out=T, n_regions=73), "exceeds the lattice")
    assert (table.view(np.uint8) == 0).all()


def test_zonal_and_shape_refusals_come_before_any_device_call(native_lib, ctx, monkeypatch):
    labels = np.zeros((8, 9), np.int32)
    field = np.ones((8, 9), np.float32)
    out = np.zeros(4, rg.ZONAL_DTYPE)
    hist = np.zeros(4 * 6, np.uint64)
    for text, kw in lc.zonal_refusals(labels, field, out, hist, DEV, DEV2):
        lc.refused(native_lib, ctx, lc.zonal_call(native_lib, ctx, **kw), text)
        assert (out.view(np.uint8) == 0).all() and (hist == 0).all(), text
    shape_out = np.zeros(4, rg.SHAPE_DTYPE)
    for text, kw in lc.shape_refusals(labels, shape_out, DEV):
        lc.refused(native_lib, ctx, lc.shape_call(native_lib, ctx, **kw), text)
        assert (shape_out.view(np.uint8) == 0).all(), text
    # an unknown value of the switch is refused by name, in both calls; the two known ones are not refused for it
    base = dict(labels=labels, field=field, out=out, n=4)
    S = dict(host_labels=labels, host_out=shape_out)
    for bad in ("fast", "", "Runs"):
        monkeypatch.setenv("MOONRT_REGIONS_ZONAL", bad)
        text = "MOONRT_REGIONS_ZONAL must be runs or plain \\(got %s\\)" % bad
        lc.refused(native_lib, ctx, lc.zonal_call(native_lib, ctx, lc.zonal_spec(), **base), text)
        lc.refused(native_lib, ctx, lc.shape_call(native_lib, ctx, **S), text)
    for good in ("runs", "plain"):
        monkeypatch.setenv("MOONRT_REGIONS_ZONAL", good)
        lc.refused(native_lib, ctx, lc.zonal_call(native_lib, ctx, lc.zonal_spec(reserved=1), **base), "reserved must be 0")
        lc.refused(native_lib, ctx, lc.shape_call(native_lib, ctx, **dict(S, conn=6)), "connectivity must be 4 or 8")
    assert (out.view(np.uint8) == 0).all() and (shape_out.view(np.uint8) == 0).all()


def test_proximity_and_reach_refusals_come_before_any_device_call(native_lib, ctx, monkeypatch):
    i, j = np.mgrid[0:8, 0:9]
    pos = np.ascontiguousarray(np.stack([j * 3, i * 2, np.zeros_like(i)], -1), np.int32)
    labels = np.where((i + 2 * j) % 3 == 0, 0, -1).astype(np.int32)
    near, d2 = np.zeros((8, 9), np.int32), np.zeros((8, 9), np.uint64)
    for text, kw in lc.prox_refusals(pos, labels, near, d2, DEV):
        lc.refused(native_lib, ctx, lc.prox_call(native_lib, ctx, **kw), text)
        assert (near == 0).all() and (d2 == 0).all(), text
    out = np.zeros(4, rg.REACH_DTYPE)
    for text, kw in lc.reach_refusals(labels, d2, near, out, DEV):
        lc.refused(native_lib, ctx, lc.reach_call(native_lib, ctx, **kw), text)
        assert (out.view(np.uint8) == 0).all(), text
    # an unknown value of the variant switch, by name; the two known ones are not refused for it
    base = dict(pos=pos, labels=labels, near=near, d2=d2)
    for bad in ("fast", "", "Brute"):
        monkeypatch.setenv("MOONRT_PROXIMITY", bad)
        lc.refused(native_lib, ctx, lc.prox_call(native_lib, ctx, **base), "MOONRT_PROXIMITY must be prune or brute \\(got %s\\)" % bad)
    for good in ("prune", "brute"):
        monkeypatch.setenv("MOONRT_PROXIMITY", good)
        lc.refused(native_lib, ctx, lc.prox_call(native_lib, ctx, **dict(base, pos=lc.prox_off_positions(pos))),
                   "coordinate 2 of node 71 must lie in")
    assert (near == 0).all() and (d2 == 0).all()
