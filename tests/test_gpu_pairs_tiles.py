"""pairs_kernel's walk over several tiles of B on the MI355X: the cases of pairs_tile_cases.py at full
size, every record, every TABLE cell and the pair count equal to the pool reference (pairs_model.pool_pairs), which knows nothing
of tiles, lanes, shares or chunks.  Case A: a share of two tiles among shares of one, at one chunk's tail, exactly one chunk and
two chunks.  Case B: B is A itself, shares of 3 and 4 tiles.  Case C: two shares, of 2 and 3 tiles.  Case D: 2 048 tiles of A, so
one workgroup walks all 65 tiles of B in two rounds and writes its records itself.  Case E: 2 047 and 2 048 tiles of A, where
the combine launch goes.  In none of them splits == tiles_b, the only scheme test_gpu_pairs.py's shapes run."""
import numpy as np
import pytest

import pairs_model as pm
import pairs_tile_cases as tc
from moonrtx_amd import _lib
from moonrtx_amd.renderer import DeviceBuffer, MoonRT

pytestmark = pytest.mark.gpu

OPS, RANKS = ("any", "both"), ("count", "gap")
BEST = [(op, "best", rank) for op in OPS for rank in RANKS]
BUILD = {"A, m = 70": lambda: tc.case_a(tc.FULL, 0), "A, m = 2048": lambda: tc.case_a(tc.FULL, 1),
         "A, m = 2118": lambda: tc.case_a(tc.FULL, 2), "B": lambda: tc.case_b(tc.FULL), "C": lambda: tc.case_c(tc.FULL),
         "D": lambda: tc.case_d(tc.FULL)}
TABLED = [n for n in BUILD if n != "D"]                     # D's table is 541 MB: once, below


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if not np.array_equal(got, want):
        at = np.argwhere(got != want)[:8]
        raise AssertionError(f"{what}: " + "; ".join(f"{tuple(i)}: got {got[tuple(i)]}, want {want[tuple(i)]}" for i in at))


@pytest.fixture(scope="module")
def rt(native_lib):
    """One context for the module, without a DEM, a light or a Moon frame: the stage needs none of them."""
    r = MoonRT(16, 16)
    yield r
    r.close()


@pytest.fixture(scope="module")
def cases():
    """name -> the case and its references so far: built once, shared and left unchanged."""
    built = {}

    def get(name):
        if name not in built:
            built[name] = (BUILD[name](), {})
        return built[name]
    return get


def refs(cases, name, calls, bounds=None):
    """The references of `calls` = (op, mode, rank)s and the pair count, one pass over the pairs for those not yet there."""
    c, have = cases(name)
    missing = [k for k in calls if (k, bounds) not in have]
    if missing:
        st = {}
        for k, r in zip(missing, c.references(missing, bounds, st)):
            r.setflags(write=False)
            have[(k, bounds)] = r
        have[("pairs", bounds)] = st["pairs"]
    return [have[(k, bounds)] for k in calls], have[("pairs", bounds)]


def call(rt, c, op, mode, rank, bounds=None, stats=None, **kw):
    return rt.mask_pairs(c.mask_a, c.m, mask_b=c.mask_b, op=op, mode=mode, rank=rank, base=c.base, stats=stats,
                         **(c.pos(bounds) if bounds else {}), **kw)


def reduces(table, best, rank, m, what):
    red = pm.reduce_table_fast(table, rank, m)
    for field in ("partner", "count", "gap"):
        assert np.array_equal(red[field], best[field]), f"{what}: BEST is not the reduction of TABLE in {field}"


@pytest.mark.parametrize("name", list(BUILD))
def test_best_over_several_tiles_of_a_share(rt, cases, name):
    c, _ = cases(name)
    want, pairs = refs(cases, name, BEST)
    assert pairs == c.n_a * c.cols - (0 if c.n_b else c.n_a)
    for (op, _, rank), w in zip(BEST, want):
        st = {}
        got = call(rt, c, op, "best", rank, stats=st)
        same(got, w, f"{name}: {op} best by {rank}")       # all four fields, gap_first among them
        assert st["pairs"] == pairs and st["launches"] == 1 + (c.layout.splits > 1), name


@pytest.mark.parametrize("name", TABLED)
def test_table_over_several_tiles_of_a_share(rt, cases, name):
    c, _ = cases(name)
    calls = [(op, "table", "count") for op in OPS]
    want, pairs = refs(cases, name, calls + BEST)
    for (op, _, _), w in zip(calls, want):
        st = {}
        table = call(rt, c, op, "table", "count", stats=st)
        same(table, w, f"{name}: {op} table")
        assert st["pairs"] == pairs and st["launches"] == 1
        for rank in RANKS:
            reduces(table, refs(cases, name, [(op, "best", rank)])[0][0], rank, c.m, f"{name}: {op} by {rank}")


@pytest.mark.parametrize("name", list(BUILD))
def test_positions_prune_against_brute(rt, cases, monkeypatch, name):
    c, _ = cases(name)
    with_table = name in TABLED
    for bounds in tc.BOUNDS:
        calls = [("any", "best", "count")] + ([("both", "table", "gap")] if with_table else [])
        want, pairs = refs(cases, name, calls, bounds)
        got = {}
        for variant in ("prune", "brute"):
            monkeypatch.setenv("MOONRT_PAIRS", variant)
            out = []
            for (op, mode, rank), w in zip(calls, want):
                st = {}
                r = call(rt, c, op, mode, rank, bounds, stats=st)
                same(r, w, f"{name}: {variant}, d2 in {bounds}: {op} {mode}")
                assert st["pairs"] == pairs, (variant, bounds)
                out += [r.tobytes(), st["pairs"], st["launches"]]
            assert out[2] == 3 + (c.layout.splits > 1) and (not with_table or out[5] == 3)
            got[variant] = out
        assert got["prune"] == got["brute"], bounds
    everything = refs(cases, name, BEST)[1]
    assert refs(cases, name, BEST[:1], tc.BOUNDS[1])[1] == 0 and refs(cases, name, BEST[:1], tc.BOUNDS[2])[1] == everything


@pytest.mark.parametrize("name", list(BUILD))
def test_best_with_positions_by_every_op_and_rank(rt, cases, monkeypatch, name):
    monkeypatch.setenv("MOONRT_PAIRS", "prune")
    c, _ = cases(name)
    want, pairs = refs(cases, name, BEST, tc.BOUNDS[0])
    for (op, _, rank), w in zip(BEST, want):
        st = {}
        same(call(rt, c, op, "best", rank, tc.BOUNDS[0], stats=st), w, f"{name}: {op} best by {rank}, d2 in {tc.BOUNDS[0]}")
        assert st["pairs"] == pairs


def test_case_d_s_table_on_the_device(rt, cases, monkeypatch):
    """16 380 x 4 130 cells, 541 MB, within the ABI's 2^28 pairs: written into a device buffer by workgroups that prune whole
    rounds, compared as raw bytes."""
    monkeypatch.setenv("MOONRT_PAIRS", "prune")
    c, _ = cases("D")
    bounds = tc.BOUNDS[0]
    (want,), pairs = refs(cases, "D", [("any", "table", "count")], bounds)
    assert c.n_a * c.cols <= 1 << 28
    out = DeviceBuffer(want.nbytes)
    try:
        st = {}
        assert call(rt, c, "any", "table", "count", bounds, stats=st, out=out) is out
        got = out.download(np.uint64, (want.size,))
    finally:
        out.free()
    assert st["pairs"] == pairs and st["launches"] == 3
    assert np.array_equal(got, want.reshape(-1).view(np.uint64))
    table = got.view(_lib.PAIR_TABLE_DTYPE).reshape(want.shape)
    for rank in RANKS:
        reduces(table, call(rt, c, "any", "best", rank, bounds), rank, c.m, f"D by {rank}")


@pytest.mark.parametrize("name", ["B", "A, m = 2118"])
def test_device_and_host_tables_agree_over_several_tiles(rt, cases, monkeypatch, name):
    """Device-resident tables, an out_offset into a buffer prefilled with 0xA5, the same call twice: the same bytes as from host
    tables and nothing written outside the records.  In TABLE a pruned tile left unblanked would keep its 0xA5."""
    monkeypatch.setenv("MOONRT_PAIRS", "prune")
    c, _ = cases(name)
    bounds = tc.BOUNDS[0]
    arrays = [c.mask_a, c.mask_b, c.base, c.pos_a, c.pos_b]
    bufs = [None if a is None else DeviceBuffer(a.nbytes) for a in arrays]
    out = DeviceBuffer(8 * c.n_a * c.cols + 1024)
    try:
        for b, a in zip(bufs, arrays):
            if b is not None:
                b.upload(a)
        for op, mode, rank in (("both", "best", "gap"), ("any", "table", "count")):
            (want,), pairs = refs(cases, name, [(op, mode, rank)], bounds)
            host = call(rt, c, op, mode, rank, bounds)
            same(host, want, f"{name}: {mode} from host tables")
            for _ in range(2):
                out.upload(np.full(out.nbytes // 8, 0xA5A5A5A5A5A5A5A5, np.uint64))
                st = {}
                got = rt.mask_pairs(bufs[0], c.m, mask_b=bufs[1], op=op, mode=mode, rank=rank, base=bufs[2], n_rows=c.n_a,
                                    n_rows_b=c.n_b if c.n_b else None, positions_a=bufs[3], positions_b=bufs[4], d2_min=bounds[0],
                                    d2_max=bounds[1], out=out, out_offset=40, stats=st)
                assert got is out and st["pairs"] == pairs
                raw = out.download(np.uint8, (out.nbytes,))
                assert raw[40:40 + host.nbytes].tobytes() == host.tobytes(), (name, mode)
                assert (raw[:40] == 0xA5).all() and (raw[40 + host.nbytes:] == 0xA5).all()      # nothing else was written
    finally:
        for b in bufs + [out]:
            if b is not None:
                b.free()


def test_the_edge_where_b_stops_being_shared_out(rt, monkeypatch):
    """2 047 tiles of A: two shares and a combine launch; 2 048: one share that writes its records itself.  The same rows give
    the same records."""
    monkeypatch.setenv("MOONRT_PAIRS", "prune")
    narrow, wide = tc.case_e(tc.FULL, False), tc.case_e(tc.FULL, True)
    for bounds in (None, tc.BOUNDS[0]):
        for op, _, rank in BEST:
            got = []
            for c in (narrow, wide):
                st, stm = {}, {}
                got.append(call(rt, c, op, "best", rank, bounds, stats=st))
                same(got[-1], c.reference(op=op, rank=rank, bounds=bounds, stats=stm), f"{c.name}: {op} by {rank}, {bounds}")
                assert st["pairs"] == stm["pairs"]
                assert st["launches"] == (2 if bounds else 0) + 1 + (c is narrow), c.name
            same(got[0], got[1][:narrow.n_a], f"E: {op} by {rank}: the rows both calls share")
    for c in (narrow, wide):
        for op in OPS:
            same(call(rt, c, op, "table", "count", tc.BOUNDS[0]), c.reference(op=op, mode="table", bounds=tc.BOUNDS[0]), c.name)
