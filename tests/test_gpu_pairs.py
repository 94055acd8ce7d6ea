"""Joint availability of mask rows on the MI355X (DESIGN.md sections 3.28 and 4.37): every record equal to the model
(tests/pairs_model.py) on the designed patterns at every word and chunk edge, on row counts around the tile sizes with partners
that tie, with positions whose d2 meet the bounds exactly, in the prune and brute variants, from device and host tables, after a
bad device coordinate, and end to end from horizon_mask to site_pairs and greedy_sites on the crater DEM."""
from datetime import datetime, timedelta, timezone

import numpy as np
import pytest

import model_cases as mc
import pairs_model as pm
from moonrtx_amd import _lib
from moonrtx_amd import networks as nw
from moonrtx_amd import traverse as tv
from moonrtx_amd._calls import MoonRTError
from moonrtx_amd.renderer import DeviceBuffer, MoonRT
from test_gpu_horizon import OBS, scene
from test_gpu_illumination import make
from test_pairs_host import M_VALUES, night_rows

pytestmark = pytest.mark.gpu

OPS, RANKS = ("any", "both"), ("count", "gap")


@pytest.fixture(scope="module")
def rt(native_lib):
    """One context for the module, without a DEM, a light or a Moon frame: the stage needs none of them."""
    r = MoonRT(16, 16)
    yield r
    r.close()


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if not np.array_equal(got, want):
        at = np.argwhere(got != want)[:8]
        raise AssertionError(f"{what}: " + "; ".join(f"{tuple(i)}: got {got[tuple(i)]}, want {want[tuple(i)]}" for i in at))


def check_all(rt, A, m, B=None, base=None, what="", **pos):
    """ROWS, and BEST and TABLE for both ops and ranks, against the model; BEST against the reduction of the device's TABLE."""
    if not pos:
        same(rt.mask_pairs(A, m, mode="rows", base=base), pm.mask_pairs(A, m, mode="rows", base=base), f"{what}: rows")
    for op in OPS:
        st, stm = {}, {}
        table = rt.mask_pairs(A, m, mask_b=B, op=op, mode="table", base=base, stats=st, **pos)
        same(table, pm.mask_pairs(A, m, mask_b=B, op=op, mode="table", base=base, stats=stm, **pos), f"{what}: {op} table")
        assert st["pairs"] == stm["pairs"], what
        for rank in RANKS:
            st = {}
            best = rt.mask_pairs(A, m, mask_b=B, op=op, rank=rank, base=base, stats=st, **pos)
            want = pm.mask_pairs(A, m, mask_b=B, op=op, rank=rank, base=base, **pos)
            same(best, want, f"{what}: {op} best by {rank}")
            assert st["pairs"] == stm["pairs"], what
            red = pm.reduce_table(table, np.zeros(table.shape, np.int32), rank)
            for field in ("partner", "count", "gap"):
                assert np.array_equal(red[field], best[field]), f"{what}: {op} by {rank}: BEST is not the reduction of TABLE"


@pytest.mark.parametrize("m", M_VALUES)
def test_designed_patterns(rt, m):
    rng = np.random.default_rng(m)
    P = pm.patterns(m)
    words = pm.pack(P)
    junk = pm.with_garbage(words, m, rng)
    base = pm.pack(pm.row(m, [(0, m // 3), (m - 3, m)]))
    for base_words in (None, base, pm.with_garbage(base, m, rng)):
        check_all(rt, words, m, base=base_words, what=f"m = {m}")
        for mode in ("rows", "best", "table"):
            same(rt.mask_pairs(junk, m, mode=mode, base=base_words), rt.mask_pairs(words, m, mode=mode, base=base_words),
                 f"m = {m}, {mode}: garbage past m")
    rows = rt.mask_pairs(junk, m, mode="rows")
    assert [tuple(r)[1:] for r in rows] == [pm.stats_loop(r) for r in P]
    best = rt.mask_pairs(words, m)                          # complementary rows find each other: a full union
    assert best["count"][-1] == m and best["gap"][-1] == 0 and best["gap_first"][-1] == -1


def tie_rows(rng, n, m):
    """n rows drawn from a small pool, so that several partners tie in count and gap; the pool holds rows of equal count and
    different gaps, and rows that share neither."""
    pool = [pm.row(m, [(10, 40)]), pm.row(m, [(10, 25), (100, 115)]), pm.row(m, [(150, 180)]), pm.row(m, [(60, 70)]),
            pm.row(m, [(0, 90)]), pm.row(m, [(120, m)])] + list(night_rows(rng, 4, m))
    return np.array([pool[int(k)] for k in rng.integers(0, len(pool), n)], bool)


@pytest.mark.parametrize("n_a,n_b", [(1, 0), (1, 130), (63, 0), (64, 65), (65, 0), (130, 0), (130, 63), (9, 200)])
def test_row_counts_and_ties(rt, n_a, n_b):
    m = 200
    rng = np.random.default_rng(1000 * n_a + n_b)
    A = pm.pack(tie_rows(rng, n_a, m))
    B = pm.pack(tie_rows(rng, n_b, m)) if n_b else None
    base = pm.pack(pm.row(m, [(0, 150)]))
    check_all(rt, A, m, B=B, what=f"{n_a} x {n_b or 'self'}")
    check_all(rt, A, m, B=B, base=base, what=f"{n_a} x {n_b or 'self'} with base")
    if n_a > 1 or n_b:
        best = rt.mask_pairs(A, m, mask_b=B)
        t = pm.mask_pairs(A, m, mask_b=B, mode="table")
        ties = [(t["count"][a] == best["count"][a]).sum() for a in range(n_a)]
        assert max(ties) > 1 or (n_b or n_a) < 8            # the least b among equal partners was on trial


def lattice(n, far):
    """n sites on a 10-unit lattice of 13 columns (so d2 = 100, 200, 400, 500, ... exactly), row after row, so that a tile of
    consecutive sites is compact; the last `far` sites lie alone, far from everything."""
    k = np.arange(n)
    pos = np.stack([10 * (k % 13), 10 * (k // 13), np.zeros(n, int)], -1)
    for j in range(far):
        pos[n - far + j] = (10 ** 6 * (j + 1), -10 ** 6, 7)
    return pos


@pytest.mark.parametrize("n_a,n_b", [(130, 0), (65, 200), (200, 9)])
def test_positions_bounds_and_variants(rt, monkeypatch, n_a, n_b):
    m = 129
    rng = np.random.default_rng(n_a)
    A = pm.pack(tie_rows(rng, n_a, m))
    B = pm.pack(tie_rows(rng, n_b, m)) if n_b else None
    pa = lattice(n_a, 3)
    pb = lattice(n_b, 2)[::-1].copy() if n_b else None
    for lo, hi in ((100, 400), (0, 100), (200, 200), (0, 2 ** 64 - 1), (500, 10 ** 5), (10 ** 12, 2 ** 64 - 1)):
        pos = dict(positions_a=pa, positions_b=pb, d2_min=lo, d2_max=hi)
        ok = pm.eligible(n_a, n_b or n_a, B is None, pa, pb, lo, hi)
        d2 = pm.d2_table(pa, pa if pb is None else pb)
        if (lo, hi) == (100, 400):
            assert (d2 == lo).any() and (d2 == hi).any() and not ok.all(axis=1).any() and (~ok.any(axis=1)).sum() >= 3
            assert B is not None or not ok.diagonal().any()
        got = {}
        for variant in ("prune", "brute"):
            monkeypatch.setenv("MOONRT_PAIRS", variant)
            st, st2 = {}, {}
            got[variant] = (rt.mask_pairs(A, m, mask_b=B, stats=st, **pos).tobytes(),
                            rt.mask_pairs(A, m, mask_b=B, mode="table", rank="gap", stats=st2, **pos).tobytes(),
                            st["pairs"], st2["pairs"], st["launches"], st2["launches"])
            assert st["pairs"] == st2["pairs"] == int(ok.sum()), (variant, lo, hi)
        assert got["prune"] == got["brute"], (lo, hi)
        monkeypatch.setenv("MOONRT_PAIRS", "prune")
        check_all(rt, A, m, B=B, what=f"{n_a} x {n_b or 'self'}, d2 in [{lo}, {hi}]", **pos)
    best = rt.mask_pairs(A, m, mask_b=B, positions_a=pa, positions_b=pb, d2_min=100, d2_max=400)
    assert (best[-3:]["partner"] == -1).all() and [tuple(r) for r in best[-3:]] == [(-1, 0, 0, -1)] * 3


def test_device_and_host_tables_agree(rt):
    m, n_a, n_b = 64 * _lib.PAIRS_CHUNK_WORDS + 70, 70, 66
    rng = np.random.default_rng(4)
    A, B = pm.with_garbage(pm.pack(night_rows(rng, n_a, m)), m, rng), pm.pack(night_rows(rng, n_b, m))
    base = pm.pack(pm.row(m, [(5, m - 9)]))
    pa, pb = lattice(n_a, 1).astype(np.int32), lattice(n_b, 0).astype(np.int32)
    bufs = [DeviceBuffer(a.nbytes) for a in (A, B, base, pa, pb)]
    out = DeviceBuffer(8 * n_a * n_b + 1024)
    try:
        for b, a in zip(bufs, (A, B, base, pa, pb)):
            b.upload(a)
        for mode, dtype, shape in (("best", _lib.PAIR_DTYPE, (n_a,)), ("table", _lib.PAIR_TABLE_DTYPE, (n_a, n_b)),
                                   ("rows", _lib.PAIR_DTYPE, (n_a,))):
            rows = mode == "rows"
            kw = dict(mode=mode, op="both", rank="gap", d2_min=0 if rows else 100, d2_max=2 ** 64 - 1 if rows else 90000)
            host = rt.mask_pairs(A, m, mask_b=None if rows else B, base=base, positions_a=None if rows else pa,
                                 positions_b=None if rows else pb, **kw)
            same(host, pm.mask_pairs(A, m, mask_b=None if rows else B, base=base, positions_a=None if rows else pa,
                                     positions_b=None if rows else pb, **kw), mode)
            for _ in range(2):                              # the same call twice: the same bytes
                out.upload(np.full(out.nbytes // 8, 0xA5A5A5A5A5A5A5A5, np.uint64))
                got = rt.mask_pairs(bufs[0], m, mask_b=None if rows else bufs[1], base=bufs[2], n_rows=n_a, n_rows_b=n_b,
                                    positions_a=None if rows else bufs[3], positions_b=None if rows else bufs[4], out=out,
                                    out_offset=40, **kw)
                assert got is out
                raw = out.download(np.uint8, (out.nbytes,))
                nbytes = host.nbytes
                assert raw[40:40 + nbytes].tobytes() == host.tobytes(), mode
                assert (raw[:40] == 0xA5).all() and (raw[40 + nbytes:] == 0xA5).all()       # nothing else was written
                same(rt.mask_pairs(A, m, mask_b=None if rows else B, base=base, positions_a=None if rows else pa,
                                   positions_b=None if rows else pb, **kw), host, mode)
    finally:
        for b in bufs + [out]:
            b.free()


def test_a_bad_device_coordinate_is_refused_after_the_launch(rt, monkeypatch):
    m, n = 100, 70
    rng = np.random.default_rng(9)
    A = pm.pack(night_rows(rng, n, m))
    pos = lattice(n, 0).astype(np.int32)
    bad = pos.copy()
    bad[66, 1] = 2 ** 29 + 1
    bad[3, 2] = -2 ** 31
    buf = DeviceBuffer(pos.nbytes)
    try:
        for variant in ("prune", "brute"):
            monkeypatch.setenv("MOONRT_PAIRS", variant)
            buf.upload(bad)
            with pytest.raises(MoonRTError, match=r"\(-1\).*2 coordinates of the device position tables lie outside"):
                rt.mask_pairs(A, m, positions_a=buf, d2_min=0, d2_max=500)
            with pytest.raises(ValueError, match="larger unit"):            # the facade checks a host table itself
                rt.mask_pairs(A, m, positions_a=bad.astype(np.int64))
            buf.upload(pos)                                                 # and nothing else went wrong
            same(rt.mask_pairs(A, m, positions_a=buf, d2_min=0, d2_max=500),
                 pm.mask_pairs(A, m, positions_a=pos, d2_min=0, d2_max=500), variant)
    finally:
        buf.free()


def test_horizon_mask_to_site_pairs_and_greedy_sites(native_lib):
    """24 x 24 points of the crater DEM over 300 hourly epochs: horizon -> horizon_mask into one device buffer (traverse.
    drive_mask) -> site_pairs and greedy_sites on the buffer, against the model on the downloaded mask."""
    s, dem = scene(), mc.crater_dem()
    r = make(s, dem, 0)
    window = (40, 100, 24, 24, 4)
    t0 = datetime(2025, 3, 12, tzinfo=timezone.utc)         # sunrise crosses the window in epochs 49 to 140
    times = [t0 + timedelta(hours=k) for k in range(300)]
    buf = tv.drive_mask(r, window, times, height_m=2.0, min_sun=0.5, n_az=64, n_bis=10, observer=OBS, chunk=200)
    try:
        m, n = 300, 576
        words = buf.download(np.uint64, (n, tv.mask_words(m)))
        bits = tv.unpack_mask(words, m)
        assert 0.05 < bits.mean() < 0.95
        lat, lon, _ = r.traverse_nodes(window)
        la, lo = (a.ravel() for a in np.meshgrid(lat, lon, indexing="ij"))
        pos = nw.point_positions(la, lo, 1737400.0, 1.0)
        stub = type("Model", (), {"mask_pairs": staticmethod(pm.mask_pairs)})
        for rank in RANKS:
            kw = dict(positions=pos, unit_m=1.0, min_dist_m=1000.0, max_dist_m=400000.0, rank=rank)
            got = nw.site_pairs(r, buf, m, n_rows=n, **kw)
            want = nw.site_pairs(stub, words, m, **kw)
            same(got.best, want.best, f"best by {rank}")
            same(got.own, want.own, "own")
            # one sunrise sweeps the window, so the sites' lit spans nest and a union need not beat its better site: >= only
            assert np.array_equal(got.gain, want.gain) and (got.gain >= 0).all()
            same(got.top(5), want.top(5), "top")
            g = nw.greedy_sites(r, buf, m, 3, rank=rank, n_rows=n)
            gm = nw.greedy_sites(stub, words, m, 3, rank=rank)
            assert np.array_equal(g.sites, gm.sites)
            same(g.records, gm.records, "greedy records")
            assert (np.diff(g.records["count"].astype(np.int64)) >= 0).all()
            union = np.bitwise_or.reduce(bits[g.sites], axis=0)
            assert tuple(g.records[-1])[1:] == pm.stats_loop(union)
    finally:
        buf.free()
        r.close()
