"""The region kernels' run reductions on the MI355X against the built tables of tests/run_layout_cases.py (DESIGN.md sections
4.26 and 4.27): the catalogue, the zonal statistics, the shapes and the histograms of every table, on every lattice it is laid
on, wrapped and not, from host and from device tables, in the run-reduced and the plain variant, equal to the models
(tests/regions_model.py, tests/zonal_model.py) field by field with ==.  tests/test_run_layouts_host.py shows what each table
reaches and which defect of a kernel it would catch.  Then the rank of the roots across more than 256 chunks, on sets whose
labelling has a closed form: isolated nodes and stripes on lattices of 256, 257 and 1025 chunks."""
import functools

import numpy as np
import pytest

import regions_model as model
import run_layout_cases as lc
import zonal_model as zm
from moonrtx_amd import regions as rg
from moonrtx_amd.renderer import MoonRT
from test_gpu_regions import stats_of
from test_gpu_zonal import assert_records_equal, hash_field, run_shape, run_zonal

pytestmark = pytest.mark.gpu

SCALE = 8.0
CASES = lc.cases()
HOST_DEVICE = ((False, "host tables"), (True, "device tables"))


@pytest.fixture(scope="module")
def rt(native_lib):
    """One context for the module, without a DEM, a light or a Moon frame: the stage needs none of them."""
    r = MoonRT(16, 16)
    yield r
    r.close()


def table_of(case):
    name, rows, cols, wrap = case
    flat, n, _ = lc.tables()[name]
    return np.ascontiguousarray(flat.reshape(rows, cols)), n, wrap


def where(labels, n, region):
    """The steps in which a region's nodes lie, with what the classifier says of them: where to look when a record differs."""
    c = lc.classify(labels.reshape(-1), n)
    steps = sorted({lc.lane_map(int(k))[:2] for k in np.flatnonzero(labels.reshape(-1) == region)})
    return "; ".join(f"stretch {s} step {t}: catalogue {sorted(c[(s, t)]['catalogue'])}, zonal {sorted(c[(s, t)]['zonal'])}"
                     for s, t in steps[:4]) or "no node carries it"


def assert_catalogue_equal(got, want, labels, n, what):
    assert got.dtype == rg.REGION_DTYPE and got.shape == (n,), what
    for name in rg.REGION_DTYPE.names:
        if not np.array_equal(got[name], want[name]):
            k = int(np.flatnonzero(got[name] != want[name])[0])
            raise AssertionError(f"{what}: {name} differs, first in region {k}: {got[k]} vs {want[k]}; {where(labels, n, k)}")


def assert_layout_records_equal(got, want, labels, n, what):
    try:
        assert_records_equal(got, want, what)
    except AssertionError as e:
        if got.shape != want.shape:
            raise
        # the region of the field the message names: the first field that differs, floats by their bits
        bits = lambda v: np.ascontiguousarray(v, np.float32).view(np.uint32) if v.dtype.kind == "f" else v
        k = next(int(np.argwhere(bits(got[f]) != bits(want[f]))[0][0]) for f in got.dtype.names
                 if not np.array_equal(bits(got[f]), bits(want[f])))
        raise AssertionError(f"{e}; region {k}: {where(labels, n, k)}") from None


@functools.lru_cache(maxsize=None)
def catalogue_of(case, weighted, heavy=False):
    labels, n, wrap = table_of(case)
    return model.catalogue(labels, n, wrap, lc.row_weights(labels.shape[0], heavy) if weighted else None)


@functools.lru_cache(maxsize=None)
def field_of(case):
    """Three channels of the hash field; the first alone is the one-channel field."""
    name, rows, cols, _ = case
    return hash_field(rows, cols, 3, len(name))


@functools.lru_cache(maxsize=None)
def zonal_of(case, weighted):
    name, rows, cols, _ = case
    labels, n, _ = table_of(case)
    return zm.zonal(labels, n, field_of(case), SCALE, lc.row_weights(rows) if weighted else None)


@pytest.mark.parametrize("case", CASES, ids=lc.case_id)
def test_the_catalogue_of_every_table(rt, monkeypatch, case):
    labels, n, wrap = table_of(case)
    w = lc.row_weights(labels.shape[0])
    for variant in ("runs", "plain"):
        monkeypatch.setenv("MOONRT_REGIONS_CATALOGUE", variant)
        for weighted in (False, True):
            for device, side in HOST_DEVICE:
                code, got = stats_of(rt, labels, n, wrap, w if weighted else None, device)
                assert code == 0, rt._lib.mrtx_last_error(rt._ctx)
                assert_catalogue_equal(got, catalogue_of(case, weighted), labels, n,
                                       f"{lc.case_id(case)}, {variant}, {side}, {'row weights' if weighted else 'no weights'}")


@pytest.mark.parametrize("catalogue", ["runs", "plain"])
def test_the_pairs_with_weights_near_2_32(rt, monkeypatch, catalogue):
    monkeypatch.setenv("MOONRT_REGIONS_CATALOGUE", catalogue)
    case = next(c for c in CASES if c[0] == "pairs" and c[3])
    labels, n, wrap = table_of(case)
    want = catalogue_of(case, True, True)
    assert want["weight"].max() > 2 ** 42                    # the fillers: tens of thousands of nodes of weight near 2^32
    for device, side in HOST_DEVICE:
        code, got = stats_of(rt, labels, n, wrap, lc.row_weights(labels.shape[0], heavy=True), device)
        assert code == 0, rt._lib.mrtx_last_error(rt._ctx)
        assert_catalogue_equal(got, want, labels, n, f"pairs, heavy weights, {catalogue}, {side}")


@pytest.mark.parametrize("case", CASES, ids=lc.case_id)
def test_the_zonal_statistics_of_every_table(rt, monkeypatch, case):
    labels, n, wrap = table_of(case)
    field = field_of(case)
    one = np.ascontiguousarray(field[:, :, :1])
    w = lc.row_weights(labels.shape[0])
    for variant in ("runs", "plain"):
        monkeypatch.setenv("MOONRT_REGIONS_ZONAL", variant)
        for weighted in (False, True):
            want = zonal_of(case, weighted)
            for device, side in HOST_DEVICE:
                what = f"{lc.case_id(case)}, {variant}, {side}, {'row weights' if weighted else 'no weights'}"
                got = run_zonal(rt, labels, n, field, w if weighted else None, device, wrap=wrap)
                assert_layout_records_equal(got, want, labels, n, what + ", 3 channels")
                got = run_zonal(rt, labels, n, one, w if weighted else None, device, wrap=wrap)
                assert_layout_records_equal(got, want[:, :1], labels, n, what + ", 1 channel")


@pytest.mark.parametrize("case", CASES, ids=lc.case_id)
def test_the_shapes_of_every_table(rt, monkeypatch, case):
    labels, n, wrap = table_of(case)
    for conn in (4, 8):
        want = zm.shape(labels, n, conn, wrap)
        for variant in ("runs", "plain"):
            monkeypatch.setenv("MOONRT_REGIONS_ZONAL", variant)
            for device, side in HOST_DEVICE:
                got = run_shape(rt, labels, n, conn, wrap, device)
                assert_layout_records_equal(got, want, labels, n, f"{lc.case_id(case)}, {conn}-connected, {variant}, {side}")


@pytest.mark.parametrize("width", lc.HIST_WIDTHS)
def test_the_histograms_of_the_hist_table(rt, monkeypatch, width):
    flat, n, x = lc.hist_table()
    rows, cols = lc.tables()["hist"][2][0]
    labels = np.ascontiguousarray(flat.reshape(rows, cols))
    field = np.ascontiguousarray(x.reshape(rows, cols, 1))
    n_bins = width - 2
    is_open, col = lc.hist_columns(x, n_bins)
    c = lc.classify_hist(flat, n, is_open, col, width)
    for wrap in (False, True):
        for weights in (None, lc.row_weights(rows)):
            want = zm.histogram(labels, n, field[:, :, 0], n_bins, 0.0, 1.0, weights)
            want_z = zm.zonal(labels, n, field, SCALE, weights)
            for variant in ("runs", "plain"):
                monkeypatch.setenv("MOONRT_REGIONS_ZONAL", variant)
                for device, side in HOST_DEVICE:
                    what = f"width {width}, {variant}, {side}, {'row weights' if weights is not None else 'no weights'}"
                    got, h = run_zonal(rt, labels, n, field, weights, device, (0, n_bins, 0.0, float(n_bins)), wrap)
                    assert h.dtype == np.uint64 and h.shape == want.shape
                    if not np.array_equal(h, want):
                        r, k = (int(v) for v in np.argwhere(h != want)[0])
                        steps = sorted({lc.lane_map(int(v))[:2] for v in np.flatnonzero((flat == r) & is_open & (col == k))})
                        raise AssertionError(f"{what}: column {k} of region {r} is {h[r, k]}, the model has {want[r, k]}; its nodes "
                                             f"lie in " + "; ".join(f"stretch {s} step {t}: {sorted(c[(s, t)])}" for s, t in steps[:4]))
                    assert_layout_records_equal(got, want_z, labels, n, what + ", beside the histogram")


# ---- the rank of the roots across more than 256 chunks
def launches_of_a_small_lattice(rt, conn, wrap):
    st = {}
    rt.regions(mask=np.ones((8, 9), np.uint8), connectivity=conn, wrap=wrap, stats=st)
    return st["label_launches"]


def assert_map_is(rt, monkeypatch, mask, conn, wrap, w, labels, K, table_w, table_1, what):
    small = launches_of_a_small_lattice(rt, conn, wrap)
    for variant in ("runs", "plain"):
        monkeypatch.setenv("MOONRT_REGIONS_CATALOGUE", variant)
        for weights, want in ((w, table_w), (None, table_1)):
            st = {}
            got = rt.regions(mask=mask, connectivity=conn, wrap=wrap, row_weights=weights, stats=st)
            tag = f"{what}, {variant}, {'row weights' if weights is not None else 'no weights'}"
            assert got.n == K, f"{tag}: {got.n} regions, the closed form has {K}"
            if not np.array_equal(got.labels, labels):
                bad = np.argwhere(got.labels != labels)
                at = tuple(int(v) for v in bad[0])
                chunk = (at[0] * labels.shape[1] + at[1]) // lc.CHUNK
                raise AssertionError(f"{tag}: {len(bad)} of {labels.size} labels differ, first at {at} (chunk {chunk}, lane "
                                     f"{chunk // lc.scan_split(-(-labels.size // lc.CHUNK))[0]} of the scan): "
                                     f"{got.labels[at]} vs {labels[at]}")
            assert got.table.dtype == rg.REGION_DTYPE and got.table.shape == (K,)
            for name in rg.REGION_DTYPE.names:
                if not np.array_equal(got.table[name], want[name]):
                    k = int(np.flatnonzero(got.table[name] != want[name])[0])
                    raise AssertionError(f"{tag}: {name} differs, first in region {k}: {got.table[k]} vs {want[k]}")
            assert st["label_launches"] == small, tag


@pytest.mark.parametrize("wrap", [False, True], ids=["open", "wrapped"])
@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("rows,cols", lc.RANK_LATTICES)
def test_ranks_of_isolated_nodes(rt, monkeypatch, rows, cols, conn, wrap):
    """10^5 .. 3 x 10^5 one-node regions: every root's rank is its place among the set nodes in row-major order."""
    w = lc.row_weights(rows)
    mask = lc.isolated_mask(rows, cols, wrap, rows + wrap)
    labels, K, table_w = lc.isolated_answer(mask, w)
    assert 100000 <= K <= 300000
    assert_map_is(rt, monkeypatch, mask, conn, wrap, w, labels, K, table_w, lc.isolated_answer(mask)[2],
                  f"isolated nodes, {rows} x {cols}, {conn}-connected{', wrapped' if wrap else ''}")


@pytest.mark.parametrize("wrap", [False, True], ids=["open", "wrapped"])
@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("rows,cols", lc.RANK_LATTICES)
def test_ranks_of_stripes(rt, monkeypatch, rows, cols, conn, wrap):
    w = lc.row_weights(rows)
    labels, K, table_w = lc.stripes_answer(rows, cols, wrap, w)
    assert_map_is(rt, monkeypatch, lc.stripes_mask(rows, cols), conn, wrap, w, labels, K, table_w,
                  lc.stripes_answer(rows, cols, wrap)[2], f"stripes, {rows} x {cols}, {conn}-connected{', wrapped' if wrap else ''}")
