"""The regions stage on the MI355X (DESIGN.md sections 3.20 and 4.26): labels, region count and every field of the catalogue
equal to the model's (tests/regions_model.py) on every built case (tests/regions_cases.py) at both connectivities, from host
and from device tables, with and without row weights; the launch count independent of the set; every refusal; a bad label
table; a context without a DEM; the largest lattice, 2^31 nodes, against its closed form; the render state left alone; the
catalogue tool; and the illumination statistics of a bowl through MoonRT.regions.  Everything is compared with ==."""
import ctypes as C
import math
from datetime import datetime, timezone

import numpy as np
import pytest

import lattice_cases as lc
import model_cases as mc
import regions_cases as rc
import regions_model as model
from bowl_dem import bowl_dem
from common import assert_bit_equal
from moonrtx_amd import _lib
from moonrtx_amd import regions as rg
from moonrtx_amd.renderer import DeviceBuffer, MoonRT, MoonRTError
from moonrtx_amd.scene import named_scene
from test_gpu_illumination import make

pytestmark = pytest.mark.gpu

INF = math.inf


@pytest.fixture(scope="module")
def rt(native_lib):
    """One context for the module, without a DEM, a light or a Moon frame: the stage needs none of them."""
    r = MoonRT(16, 16)
    yield r
    r.close()


def run(rt, case, conn, device=False, weights=None, stats=None):
    """MoonRT.regions on a case, from host arrays or from DeviceBuffers."""
    kw = dict(connectivity=conn, wrap=case["wrap"], row_weights=weights, stats=stats)
    if "mask" in case:
        src, name = case["mask"], "mask"
    else:
        src, name = case["field"], "field"
        kw.update(channel=case["ch"], lo=case["lo"], hi=case["hi"])
    if not device:
        return rt.regions(**{name: src}, **kw)
    buf = DeviceBuffer(max(src.nbytes, 4))
    try:
        buf.upload(src)
        return rt.regions(**{name: buf}, shape=src.shape, **kw)
    finally:
        buf.free()


def assert_map_equal(got, labels, n, table, what):
    assert got.n == n, f"{what}: {got.n} regions, the model has {n}"
    if not np.array_equal(got.labels, labels):
        bad = np.argwhere(got.labels != labels)
        raise AssertionError(f"{what}: {len(bad)} of {labels.size} labels differ, first at {tuple(bad[0])}: "
                             f"{got.labels[tuple(bad[0])]} vs {labels[tuple(bad[0])]}")
    assert got.table.dtype == rg.REGION_DTYPE and got.table.shape == (n,)
    for name in rg.REGION_DTYPE.names:
        if not np.array_equal(got.table[name], table[name]):
            k = int(np.flatnonzero(got.table[name] != table[name])[0])
            raise AssertionError(f"{what}: {name} differs, first in region {k}: {got.table[k]} vs {table[k]}")


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("name", [c["name"] for c in rc.CASES])
def test_every_case_equals_the_model(rt, name, conn):
    case = rc.BY_NAME[name]
    labels, n = rc.answer(case, conn)
    w = rc.weights_for(case)
    for device in (False, True):
        for weighted in (False, True):
            got = run(rt, case, conn, device, w if weighted else None)
            assert_map_equal(got, labels, n, rc.table(case, conn, weighted),
                             f"{name}, {conn}-connected, {'device' if device else 'host'} tables, "
                             f"{'row weights' if weighted else 'no weights'}")


@pytest.mark.parametrize("catalogue", ["runs", "plain"])
def test_full_set_with_weights_near_2_32(rt, monkeypatch, catalogue):
    """One region, every node adding to one record, weights near 2^32 - 1: the sum needs 64 bits; the run reduction and the
    one-atomic-per-node yardstick give the same record."""
    monkeypatch.setenv("MOONRT_REGIONS_CATALOGUE", catalogue)
    case = rc.BY_NAME["full"]
    w = rc.weights_for(case, heavy=True)
    want = rc.table(case, 4, True, heavy=True)
    assert want[0]["weight"] > 2 ** 47 and want[0]["count"] == 65536
    for device in (False, True):
        assert_map_equal(run(rt, case, 4, device, w), *rc.answer(case, 4), want, f"full set, heavy weights, {catalogue}")
    r59 = rc.BY_NAME["random_0.59_wrapped"]
    assert_map_equal(run(rt, r59, 8, False, rc.weights_for(r59)), *rc.answer(r59, 8), rc.table(r59, 8, True),
                     f"random 0.59, {catalogue}")


def test_catalogue_switch_is_checked(rt, monkeypatch):
    monkeypatch.setenv("MOONRT_REGIONS_CATALOGUE", "fast")
    with pytest.raises(MoonRTError, match="MOONRT_REGIONS_CATALOGUE"):
        run(rt, rc.BY_NAME["1x40"], 4)


def test_launches_do_not_depend_on_the_set(rt):
    masks = [rc.BY_NAME["spiral"]["mask"], np.zeros((96, 96), np.uint8), np.ones((96, 96), np.uint8),
             rc.random_mask(96, 96, 0.59, 5)]
    for conn in (4, 8):
        for wrap in (False, True):
            seen = []
            for m in masks:
                st = {}
                rt.regions(mask=m, connectivity=conn, wrap=wrap, stats=st)
                assert st["label_launches"] > 0 and st["kernel_ms"] > 0.0
                seen.append(st["label_launches"])
            assert len(set(seen)) == 1, seen


# ---- the ABI straight
def label_call(rt, r, **kw):
    return lc.label_call(rt._lib, rt._ctx, r, **kw)


block = lc.regions_block


def test_every_refusal(rt):
    mask = np.ones((8, 9), np.uint8)
    field = np.ones((8, 9), np.float32)
    labels = np.full((8, 9), 7, np.int32)
    dev = DeviceBuffer(4096)
    dev2 = DeviceBuffer(4096)
    n = C.c_uint32(4321)
    try:
        for text, kw in lc.label_refusals(mask, field, labels, n, dev.ptr, dev2.ptr):
            lc.refused(rt._lib, rt._ctx, label_call(rt, **kw), text)
            assert n.value == 4321 and (labels == 7).all(), text
        # the catalogue's own
        table = np.zeros(4, rg.REGION_DTYPE)
        for text, kw in lc.stats_refusals(labels, table, dev.ptr):
            lc.refused(rt._lib, rt._ctx, lc.stats_call(rt._lib, rt._ctx, **kw), text)
            assert (table.view(np.uint8) == 0).all(), text
        # the context still works
        case = rc.BY_NAME["33x65_wrapped"]
        assert_map_equal(run(rt, case, 8), *rc.answer(case, 8), rc.table(case, 8), "after the refusals")
    finally:
        dev.free()
        dev2.free()


def stats_of(rt, labels, n_regions, wrap=False, weights=None, device=False):
    """(return code, table) of mrtx_regions_stats on a caller's label table."""
    labels = np.ascontiguousarray(labels, np.int32)
    rows, cols = labels.shape
    table = np.zeros(max(n_regions, 1), rg.REGION_DTYPE)
    wp = None if weights is None else weights.ctypes.data
    if not device:
        code = rt._lib.mrtx_regions_stats(rt._ctx, rows, cols, int(wrap), None, labels.ctypes.data, n_regions, wp, None,
                                          table.ctypes.data, None)
        return code, table[:n_regions]
    lab, out = DeviceBuffer(labels.nbytes), DeviceBuffer(table.nbytes)
    try:
        lab.upload(labels)
        out.upload(table)
        code = rt._lib.mrtx_regions_stats(rt._ctx, rows, cols, int(wrap), lab.ptr, None, n_regions, wp, out.ptr, None, None)
        return code, out.download(rg.REGION_DTYPE, table.shape)[:n_regions]
    finally:
        lab.free()
        out.free()


def test_a_bad_label_table_is_refused_after_the_launch(rt):
    labels, n = rc.answer(rc.BY_NAME["random_0.59"], 4)
    for bad in (n, n + 1000, 2 ** 31 - 1, -2, -2 ** 31):
        for device in (False, True):
            mine = labels.copy()
            mine[17, 23] = bad
            code, _ = stats_of(rt, mine, n, device=device)
            assert code == -1, bad
            assert "1 entries outside -1" in rt._lib.mrtx_last_error(rt._ctx).decode()
    # and the context goes on
    code, t = stats_of(rt, labels, n)
    assert code == 0 and np.array_equal(t, rc.table(rc.BY_NAME["random_0.59"], 4).astype(rg.REGION_DTYPE))


def test_the_callers_own_labels(rt):
    """A table that is no labelling: numbers scattered over the lattice, one number unused, wrapped and not."""
    rng = np.random.default_rng(9)
    mine = rng.integers(-1, 6, (37, 70)).astype(np.int32)
    mine[mine == 3] = -1                                    # number 3 has no node
    w = (5 + np.arange(37)).astype(np.uint32)
    for wrap in (False, True):
        for device in (False, True):
            code, t = stats_of(rt, mine, 6, wrap, w, device)
            assert code == 0
            want = model.catalogue(mine, 6, wrap, w)
            assert want[3]["count"] == 0 and (want[3]["root_i"], want[3]["root_j"]) == (-1, -1)
            for name in rg.REGION_DTYPE.names:
                assert np.array_equal(t[name], want[name]), (name, wrap, device)
    # no regions: the table is checked, nothing is written
    code, t = stats_of(rt, np.full((5, 5), -1, np.int32), 0)
    assert code == 0 and len(t) == 0
    one = np.full((5, 5), -1, np.int32)
    one[2, 2] = 0
    code, _ = stats_of(rt, one, 0, device=True)
    assert code == -1


def test_device_labels_are_the_host_labels(rt):
    """Straight through the ABI with device tables for input, labels and catalogue."""
    case = rc.BY_NAME["random_0.59_wrapped"]
    labels, n = rc.answer(case, 8)
    m = case["mask"]
    src, lab = DeviceBuffer(m.nbytes), DeviceBuffer(4 * m.size)
    try:
        src.upload(m)
        k = C.c_uint32(0)
        st = _lib.MrtxStats()
        r = block(200, 136, 1, 8)
        assert rt._lib.mrtx_regions_label(rt._ctx, C.byref(r), None, None, src.ptr, None, lab.ptr, None, C.byref(k),
                                          C.byref(st)) == 0
        assert k.value == n and st.launches > 0 and st.kernel_ms > 0.0
        assert np.array_equal(lab.download(np.int32, m.shape), labels)
        assert np.array_equal(src.download(np.uint8, m.shape), m)           # the input is left alone
    finally:
        src.free()
        lab.free()


def test_a_lattice_of_2_31_nodes(native_lib):
    """The largest lattice the stage takes, 32768 x 65536 wrapped, every node in the set but one row: two regions whose
    catalogue is known in closed form.  Node indices reach 2^31 - 1, byte offsets 8 GB, a count 2^30.6 and sum_i 2^45."""
    rows, cols, gap = 32768, 65536, 20000
    r = MoonRT(16, 16)
    src, lab, rec = DeviceBuffer(rows * cols), DeviceBuffer(4 * rows * cols), DeviceBuffer(2 * 56)
    try:
        ones = np.ones((1024, cols), np.uint8)
        for a in range(0, rows, 1024):
            src.upload(ones, a * cols)
        src.upload(np.zeros(cols, np.uint8), gap * cols)
        k = C.c_uint32(0)
        st = _lib.MrtxStats()
        b = block(rows, cols, 1, 4)
        assert r._lib.mrtx_regions_label(r._ctx, C.byref(b), None, None, src.ptr, None, lab.ptr, None, C.byref(k),
                                         C.byref(st)) == 0, r._lib.mrtx_last_error(r._ctx)
        small = {}
        r.regions(mask=np.ones((8, 9), np.uint8), wrap=True, stats=small)
        assert k.value == 2 and st.launches == small["label_launches"]
        w = (1 + np.arange(rows) % 7).astype(np.uint32)
        assert r._lib.mrtx_regions_stats(r._ctx, rows, cols, 1, lab.ptr, None, 2, w.ctypes.data, rec.ptr, None, None) == 0, \
            r._lib.mrtx_last_error(r._ctx)
        t = rec.download(rg.REGION_DTYPE, (2,))

        def row_of_labels(i):
            out = np.empty(cols, np.int32)
            assert r._lib.mrtx_dev_download(lab.device, out.ctypes.data, lab.ptr + 4 * i * cols, out.nbytes) == 0
            return out
        for i, want in ((0, 0), (gap - 1, 0), (gap, -1), (gap + 1, 1), (rows - 1, 1)):
            assert (row_of_labels(i) == want).all(), i
        # dj over a full wrapped row with the root in column 0: -cols / 2 .. cols / 2 - 1, which sums to -cols / 2
        for n, (i0, i1) in enumerate(((0, gap - 1), (gap + 1, rows - 1))):
            ii = np.arange(i0, i1 + 1, dtype=np.int64)
            want = (int(w[i0:i1 + 1].astype(np.int64).sum()) * cols, int(ii.sum()) * cols, -(cols // 2) * len(ii), len(ii) * cols,
                    i0, 0, i0, i1, -(cols // 2), cols // 2 - 1, 0)
            assert tuple(int(v) for v in t[n].tolist()) == want, n
    finally:
        for buf in (src, lab, rec):
            buf.free()
        r.close()


def test_leaves_the_render_state_alone(native_lib):
    s = named_scene("S1", 16, 16).with_size(48, 32, spp_per_launch=16)
    dem = mc.crater_dem()
    case = rc.BY_NAME["random_0.59"]

    def go(with_regions):
        r = make(s, dem, _lib.F_COUNT_STATS)
        st1 = r.render(1)
        if with_regions:
            assert_map_equal(run(r, case, 4, weights=rc.weights_for(case)), *rc.answer(case, 4), rc.table(case, 4, True),
                             "between two renders")
            run(r, case, 8, device=True)
        st2 = r.render(1)
        out = r.read_linear(), r.read_hits(), r.samples_done(), st1, st2
        r.close()
        return out
    a, b = go(False), go(True)
    assert_bit_equal(b[0], a[0], "linear radiance")
    assert_bit_equal(b[1], a[1], "hit buffer")
    assert b[2] == a[2] == 32
    for k in ("primary_hits", "shadow_rays", "height_samples", "bounce_rays"):
        assert b[4][k] == a[4][k], k


def test_the_catalogue_tool_lists_what_it_totals(native_lib, tmp_path):
    """tools/region_catalogue.py on a saved south-polar map: the CSV's areas sum to the printed total, exactly in units and
    as the exactly rounded float sum in km^2, and the labels it writes are the model's with the small regions dropped."""
    import csv
    import os
    import re
    import subprocess
    import sys
    rows, cols = 127, 384
    rng = np.random.default_rng(3)
    lit = rng.random((rows, cols, 2)).astype(np.float32)
    lit[40:60, 370:, 1] = 0.0                                # a shadow across the seam
    lit[40:60, :9, 1] = 0.0
    np.save(tmp_path / "stats.npy", lit)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, os.path.join(root, "tools", "region_catalogue.py"), "--map", str(tmp_path / "stats.npy"),
                        "--channel", "1", "--below", "0.3", "--window", "7800", "0", "127", "384", "120", "1",
                        "--min-area-km2", "2000", "--unit-m2", "100", "--out", str(tmp_path / "labels.npy"),
                        "--csv", str(tmp_path / "regions.csv")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    total = re.search(r"total area (\S+) km\^2 = (\d+) units", p.stdout)
    assert total, p.stdout
    with open(tmp_path / "regions.csv") as f:
        lines = list(csv.DictReader(f))
    assert len(lines) >= 2
    assert math.fsum(float(r["area_km2"]) for r in lines) == float(total.group(1))
    assert sum(int(r["area_units"]) for r in lines) == int(total.group(2))
    areas = [float(r["area_km2"]) for r in lines]
    assert areas == sorted(areas, reverse=True) and min(areas) >= 2000.0 and [int(r["rank"]) for r in lines] == list(range(1, len(lines) + 1))
    labels, n = model.label(model.predicate(lit, 1, -INF, 0.3), 4, True)
    w = rg.row_weights((7800, 0, 127, 384, 120, 1), (23040, 46080), 1737400.0, 100.0)
    t = model.catalogue(labels, n, True, w)
    keep = t["weight"].astype(np.float64) * 100.0 >= 2000e6
    got = np.load(tmp_path / "labels.npy")
    assert len(lines) == keep.sum() and got.max() == keep.sum() - 1
    assert np.array_equal(got >= 0, np.isin(labels, np.flatnonzero(keep)))
    # the shadow across the seam (20 rows x 23 columns near the equator) is in the largest region, which straddles the seam
    assert int(lines[0]["nodes"]) >= 20 * 23 and int(lines[0]["col_west"]) > int(lines[0]["col_east"])


def test_illumination_statistics_of_a_bowl(native_lib):
    """The lit share of a bowl near the south pole over a month, thresholded through MoonRT.regions: the map's regions equal
    the model's on the same map, with the window's row weights."""
    from moonrtx_amd import ephemeris as E
    from moonrtx_amd.sunlight import illumination_statistics
    H, W = 360, 720
    dem = bowl_dem(H, W, lat0_deg=-84.0, lon0_deg=40.0, theta_c_deg=4.0, d_over_D=0.2)
    r = MoonRT(16, 16)
    r.upload_dem(dem)
    r.apply_scene(named_scene("S1", 16, 16))
    r.set_params(flags=0)
    window = (340, 400, 18, 60)                              # rows 340 .. 357: latitudes -80.25 .. -88.75
    la, lo, _ = r.traverse_nodes(window)
    LA, LO = np.meshgrid(la, lo, indexing="ij")
    s = illumination_statistics(r, LA.ravel(), LO.ravel(), datetime(2025, 1, 1, tzinfo=timezone.utc), 30, step_min=360,
                                n_az=64, n_bis=8, observer=E.Observer(52.2, 21.0, 0.0))
    field = np.ascontiguousarray(np.stack([s.mean_fraction, s.lit_fraction, s.full_fraction], -1).reshape(18, 60, 3),
                                 np.float32)
    hi = 0.5 * (float(field[:, :, 1].min()) + float(field[:, :, 1].max()))
    w = rg.row_weights(window, (H, W), 1737400.0, 1e4)
    got = r.regions(field=field, channel=1, hi=hi, connectivity=8, row_weights=w, unit_m2=1e4)
    r.close()
    mask = model.predicate(field, 1, -INF, hi)
    assert 0 < mask.sum() < mask.size
    labels, n = model.label(mask, 8, False)
    assert n >= 1
    assert_map_equal(got, labels, n, model.catalogue(labels, n, False, w), "the bowl's lit share")
    assert abs(got.area_m2().sum() - float((mask * w[:, None].astype(np.float64)).sum()) * 1e4) < 1.0
