"""Joint availability of mask rows without a GPU: the model against an independent brute force, the
designed patterns against every named defect of the kernel's word walk, the ABI, every refusal of mrtx_mask_pairs through a
context without a device, mask_pairs' own argument checks, and networks.py on a stub renderer whose mask_pairs is the model."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pairs_model as pm
from moonrtx_amd import _lib
from moonrtx_amd import networks as nw
from moonrtx_amd import regions as rg
from moonrtx_amd import traverse as tv
from moonrtx_amd.terrain_calls import TerrainCalls

E_INVALID, E_DEVICE = -1, -2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CH = _lib.PAIRS_CHUNK_WORDS     # mrtx_pairs.h's MRTX_PAIRS_CHUNK (held equal, with the model's, by the first test below)
# m: the word edges, and one word below / at / above the kernel's LDS chunk
M_VALUES = (1, 63, 64, 65, 127, 128, 129, 200, 64 * (CH - 1), 64 * CH, 64 * CH + 1, 64 * (CH + 1))


@pytest.fixture
def ctx(native_lib):
    """A context handle; without a GPU mrtx_create stops at its first HIP call but hands the context out."""
    c = C.c_void_p()
    rc = native_lib.mrtx_create(C.byref(_lib.MrtxConfig(0, 16, 16, 0, 1, 0, 0)), C.byref(c))
    assert rc in (0, -2) and c.value
    c.has_device = rc == 0
    yield c
    native_lib.mrtx_destroy(c)


class StubRT:
    """A renderer whose mask_pairs is the model."""
    mask_pairs = staticmethod(pm.mask_pairs)


def night_rows(rng, n, m, nights=3):
    """Rows with a few long nights each, as real masks have."""
    bits = np.ones((n, m), bool)
    for r in range(n):
        for _ in range(int(rng.integers(0, nights + 1))):
            s = int(rng.integers(0, m))
            bits[r, s:s + int(rng.integers(1, max(m // 3, 2)))] = False
    return bits


# ---- the model ---------------------------------------------------------------------------------------------------------------
def test_the_chunk_constant_is_the_header_s():
    text = open(os.path.join(ROOT, "moonrtx_amd", "csrc", "mrtx_pairs.h")).read()
    assert int(re.search(r"#define\s+MRTX_PAIRS_CHUNK\s+(\d+)", text).group(1)) == _lib.PAIRS_CHUNK_WORDS == pm.CHUNK


def test_row_stats_agree_with_the_plain_loop_and_the_word_walk():
    rng = np.random.default_rng(5)
    seen = dict(full=0, gap_at_end=0, several_words=0)
    for _ in range(400):
        m = int(rng.choice([1, 2, 63, 64, 65, 130, 200, int(rng.integers(1, 300))]))
        bits = night_rows(rng, 1, m)[0] if rng.random() < 0.5 else rng.random(m) < rng.choice([0.1, 0.5, 0.9])
        want = pm.stats_loop(bits)
        c, g, f = pm.row_stats(bits[None, :])
        assert (int(c[0]), int(g[0]), int(f[0])) == want
        for chunk in (1, 2, CH):
            assert pm.word_walk(pm.with_garbage(pm.pack(bits), m, rng), m, chunk) == want, (m, chunk)
        seen["full"] += want[0] == m
        seen["gap_at_end"] += want[1] > 0 and want[2] + want[1] == m
        seen["several_words"] += want[1] > 64
    assert min(seen.values()) > 5, seen
    assert pm.stats_loop([True] * 5) == (5, 0, -1) and pm.stats_loop([False, True, False]) == (1, 1, 0)


def brute_pairs(A, B, same, op, rank, base, pos_a, pos_b, lo, hi):
    """BEST, TABLE and pairs straight from the issue's sentences, one pair at a time."""
    n_a, n_b = len(A), len(B)
    rec, table, pairs = [], np.zeros((n_a, n_b), pm.PAIR_TABLE_DTYPE), 0
    for a in range(n_a):
        cands = []
        for b in range(n_b):
            ok = not (same and a == b)
            if ok and pos_a is not None:
                d2 = sum((int(x) - int(y)) ** 2 for x, y in zip(pos_a[a], (pos_a if same else pos_b)[b]))
                ok = lo <= d2 <= hi
            if not ok:
                table[a, b] = (pm.NONE, pm.NONE)
                continue
            pairs += 1
            J = [bool((x or y) if op == "any" else (x and y)) or bool(s) for x, y, s in zip(A[a], B[b], base)]
            c, g, f = pm.stats_loop(J)
            table[a, b] = (c, g)
            cands.append(((-c, g, b) if rank == "count" else (g, -c, b), (b, c, g, f)))
        rec.append(min(cands)[1] if cands else (-1, 0, 0, -1))
    return np.array(rec, pm.PAIR_DTYPE), table, pairs


def test_the_model_agrees_with_a_brute_force():
    rng = np.random.default_rng(11)
    for trial in range(40):
        m = int(rng.choice([1, 7, 64, 65, 100]))
        n_a, n_b = int(rng.integers(1, 7)), int(rng.integers(1, 7))
        same = trial % 2 == 0
        A = night_rows(rng, n_a, m) & (rng.random((n_a, m)) < 0.9)
        if trial % 5 == 0:
            A[1:] = A[0]                                   # every partner ties
        B = A if same else night_rows(rng, n_b, m)
        if trial % 5 == 1:
            B[:] = B[0]
        base = rng.random(m) < 0.2 if trial % 3 == 0 else np.zeros(m, bool)
        pos = trial % 4 < 2
        pa = rng.integers(-3, 4, (n_a, 3)) if pos else None
        pb = None if same or not pos else rng.integers(-3, 4, (len(B), 3))
        lo, hi = (int(rng.integers(0, 6)), int(rng.integers(4, 30))) if pos else (0, pm.M64)
        for op in ("any", "both"):
            for rank in ("count", "gap"):
                want = brute_pairs(A, B, same, op, rank, base, pa, pb, lo, hi)
                kw = dict(mask_b=None if same else pm.pack(B), op=op, rank=rank, base=pm.pack(base) if trial % 3 == 0 else None,
                          positions_a=pa, positions_b=pb, d2_min=lo, d2_max=hi)
                st = {}
                assert np.array_equal(pm.mask_pairs(pm.pack(A), m, mode="best", stats=st, **kw), want[0])
                assert np.array_equal(pm.mask_pairs(pm.pack(A), m, mode="table", **kw), want[1])
                assert st["pairs"] == want[2]
                rec, table, pairs = pm.walk_pairs(pm.with_garbage(pm.pack(A), m, rng), m, **{k: v for k, v in kw.items()})
                assert np.array_equal(rec, want[0]) and np.array_equal(table, want[1]) and pairs == want[2]
    rows = pm.mask_pairs(pm.pack(A), m, mode="rows", base=pm.pack(base))
    assert [tuple(r) for r in rows] == [(-1,) + pm.stats_loop(a | base) for a in A]


def lattice_case(m):
    """Rows and positions for the pair-level defects: sites on a line at unit spacing, d2 bounds that some pairs meet exactly,
    one site too far for any partner, and partners that tie in count and gap."""
    P = pm.patterns(m)
    rows = np.array([P[2], P[3], P[3], P[3], P[9 % len(P)], P[2], P[0]], bool)
    pos = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0], [4, 0, 0], [5, 0, 0], [100, 0, 0]])
    return pm.pack(rows), pos, 1, 4


def test_every_named_defect_is_told_apart_by_the_designed_patterns():
    rng = np.random.default_rng(3)
    told = {mu: 0 for mu in pm.MUTANTS}
    for m in M_VALUES:
        P = pm.patterns(m)
        words = pm.pack(P)
        junk = pm.with_garbage(words, m, rng)
        want = [pm.stats_loop(r) for r in P]
        assert [pm.word_walk(w, m) for w in words] == want and [pm.word_walk(w, m) for w in junk] == want
        for mu in pm.MUTANTS[:6]:
            told[mu] += sum(pm.word_walk(w, m, mutant=mu) != t for tbl in (words, junk) for w, t in zip(tbl, want))
        rows, pos, lo, hi = lattice_case(m)
        good = pm.walk_pairs(rows, m, positions_a=pos, d2_min=lo, d2_max=hi)
        assert np.array_equal(good[0], pm.mask_pairs(rows, m, positions_a=pos, d2_min=lo, d2_max=hi))
        assert good[0]["partner"][-1] == -1                 # the far site has no partner
        for mu in pm.MUTANTS[6:]:
            bad = pm.walk_pairs(rows, m, positions_a=pos, d2_min=lo, d2_max=hi, mutant=mu)
            told[mu] += not (np.array_equal(bad[0], good[0]) and np.array_equal(bad[1], good[1]) and bad[2] == good[2])
    assert all(told.values()), told
    # per m: the word-level defects that m can show at all are shown there
    for m, mutants in ((200, ("no_carry", "later_of_equals", "garbage_counted", "last_word_open", "interior_missed")),
                       (64 * CH + 1, ("chunk_carry_lost",))):
        P = pm.patterns(m)
        for mu in mutants:
            assert any(pm.word_walk(w, m, mutant=mu) != pm.stats_loop(r)
                       for tbl in (pm.pack(P), pm.with_garbage(pm.pack(P), m, rng)) for w, r in zip(tbl, P)), (m, mu)


def test_the_patterns_hold_what_they_are_designed_to_hold():
    m = 200
    P = pm.patterns(m)
    c, g, f = pm.row_stats(P)
    assert (c[0], g[0], f[0]) == (m, 0, -1) and (c[1], g[1], f[1]) == (0, m, 0)
    assert f[2] == 0 and f[3] + g[3] == m                              # gaps touching epoch 0 and m - 1
    assert f[6] + g[6] == 64 and f[7] == 64                           # ending at and starting at a word edge
    assert f[8] // 64 + 2 == (f[8] + g[8] - 1) // 64                  # spanning three words
    assert g[9] == 7 and f[9] == 3                                    # two equal gaps: the earlier one
    assert (g[11], f[11]) == (10, 10)                                 # the interior gap beats the word's end runs
    assert (P[-1] | P[-2]).all() and (P[-3] | P[-4]).all()            # complementary rows


# ---- the ABI -----------------------------------------------------------------------------------------------------------------
def test_the_abi_holds_the_call(native_lib):
    text = open(os.path.join(ROOT, "include", "moonrt.h")).read()
    assert re.search(r"\bint\s+mrtx_mask_pairs\s*\(", text) and "typedef struct MrtxMaskPairs" in text
    assert "mrtx_mask_pairs" in _lib.SIGNATURES and getattr(native_lib, "mrtx_mask_pairs") is not None
    assert native_lib.mrtx_abi_version() == 7 == _lib.ABI_VERSION
    assert C.sizeof(_lib.MrtxMaskPairs) == 48
    for name, value in (("ANY", 0), ("BOTH", 1), ("ROWS", 0), ("BEST", 1), ("TABLE", 2), ("BY_COUNT", 0), ("BY_GAP", 1)):
        assert getattr(_lib, "PAIRS_" + name) == value
        assert re.search(r"#define\s+MRTX_PAIRS_" + name + r"\s+" + str(value) + r"\b", text), name
    assert _lib.PAIR_DTYPE == pm.PAIR_DTYPE and _lib.PAIR_TABLE_DTYPE == pm.PAIR_TABLE_DTYPE


def test_mask_pairs_arguments_are_checked_before_any_device_call(native_lib, ctx, monkeypatch):
    monkeypatch.delenv("MOONRT_PAIRS", raising=False)
    f = native_lib.mrtx_mask_pairs
    m = 130
    A = pm.pack(np.ones((4, m), bool))
    B = pm.pack(np.ones((3, m), bool))
    base = pm.pack(np.ones(m, bool))
    pa = np.zeros((4, 3), np.int32)
    pb = np.zeros((3, 3), np.int32)
    out = np.zeros(64, np.uint64)
    P = lambda a: None if a is None else a.ctypes.data

    def call(c=ctx, blk=True, n_a=4, n_b=0, m=m, op=0, mode=1, rank=0, res=(0, 0), lo=0, hi=2 ** 64 - 1, da=None, ha=A, db=None,
             hb=None, dbase=None, hbase=None, dpa=None, hpa=None, dpb=None, hpb=None, dout=None, hout=out):
        p = _lib.MrtxMaskPairs(n_a, n_b, m, op, mode, rank, (C.c_int32 * 2)(*res), lo, hi)
        hx = lambda v: P(v) if isinstance(v, np.ndarray) else v
        return f(c, C.byref(p) if blk else None, da, hx(ha), db, hx(hb), dbase, hx(hbase), dpa, hx(hpa), dpb, hx(hpb), dout,
                 hx(hout), None, None)
    assert call(c=None) == E_INVALID
    bad = (dict(blk=False), dict(res=(1, 0)), dict(res=(0, 1)), dict(m=0), dict(m=(1 << 24) + 1), dict(n_a=0),
           dict(n_a=(1 << 24) + 1), dict(n_b=-1), dict(n_b=(1 << 24) + 1, hb=B), dict(mode=3), dict(mode=-1), dict(op=2),
           dict(rank=2), dict(ha=None), dict(da=8), dict(db=8, hb=B, n_b=3), dict(dbase=8, hbase=base),
           dict(dpa=8, hpa=pa), dict(dpb=8, hpb=pb, hpa=pa, hb=B, n_b=3), dict(hout=None), dict(dout=8),
           dict(hb=B), dict(n_b=3),                                         # a B table iff n_b > 0
           dict(mode=0, hb=B, n_b=3), dict(mode=0, hpa=pa),                 # ROWS takes neither
           dict(hpb=pb), dict(hpa=pa, hpb=pb), dict(hpa=pa, hb=B, n_b=3), dict(hb=B, n_b=3, hpb=pb),      # pos_b iff pos_a and B
           dict(n_a=1 << 24, m=64 * 128), dict(hb=B, n_b=1 << 24, m=64 * 128),                           # 2^31 words
           dict(mode=2, n_a=1 << 15), dict(mode=2, n_a=1 << 14, hb=B, n_b=(1 << 14) + 1),                # 2^28 pairs
           dict(ha=None, da=4), dict(hb=None, db=12, n_b=3), dict(dbase=4), dict(hout=None, dout=4),     # 8-byte alignment
           dict(hpa=None, dpa=2), dict(hpa=pa, hb=B, n_b=3, dpb=6),                                      # 4-byte alignment
           dict(ha=None, da=4096, hout=None, dout=4096 + 8 * 4 * 3 - 8), dict(dbase=4096, hout=None, dout=4096 + 16),
           dict(dpa=4096, hout=None, dout=4096 + 40), dict(hb=None, db=8192, n_b=3, hout=None, dout=8192 - 8))
    for kw in bad:
        assert call(**kw) == E_INVALID, kw
        assert native_lib.mrtx_last_error(ctx)
    for k in (0, 5, 11):                                                    # a host coordinate outside +-2^29
        for v in (2 ** 29 + 1, -2 ** 29 - 1):
            q = pa.copy()
            q.flat[k] = v
            assert call(hpa=q) == E_INVALID
            q = pb.copy()
            q.flat[min(k, 8)] = v
            assert call(hpa=pa, hb=B, n_b=3, hpb=q) == E_INVALID
    monkeypatch.setenv("MOONRT_PAIRS", "fast")
    assert call() == E_INVALID and b"MOONRT_PAIRS" in native_lib.mrtx_last_error(ctx)
    # good arguments get past every check: what stops them is the device
    edge = pa.copy()
    edge[0], edge[1] = 2 ** 29, -2 ** 29
    for env in (None, "prune", "brute"):
        monkeypatch.delenv("MOONRT_PAIRS", raising=False) if env is None else monkeypatch.setenv("MOONRT_PAIRS", env)
        good = [dict(), dict(op=1, rank=1), dict(mode=2), dict(mode=0), dict(mode=0, op=7, rank=9), dict(mode=2, rank=5),
                dict(hbase=base), dict(hb=B, n_b=3), dict(hpa=edge), dict(hpa=pa, hb=B, n_b=3, hpb=pb, lo=5, hi=2),
                dict(m=1, ha=np.ascontiguousarray(A[:, :1]))]
        if not ctx.has_device:          # made-up device addresses are only ever looked at, never followed, without a device
            good += [dict(hout=None, dout=8), dict(ha=None, da=4096, hout=None, dout=4096 + 8 * 4 * 3),
                     dict(mode=2, n_a=1 << 14, hb=B, n_b=1 << 14, m=1)]
        for kw in good:
            # with a GPU the call simply runs; without one the device is what stops it
            assert call(**kw) == (0 if ctx.has_device else E_DEVICE), (kw, native_lib.mrtx_last_error(ctx))


class _NoDevice(TerrainCalls):
    """mask_pairs' own checks come before the library is touched."""
    _lib = None
    _ctx = None


def test_mask_pairs_checks_its_own_arguments():
    rt = _NoDevice()
    A = pm.pack(np.ones((4, 130), bool))
    pos = np.zeros((4, 3), np.int64)
    for kw in (dict(op="either"), dict(mode="all"), dict(rank="best"), dict(n_epochs=0), dict(n_epochs=(1 << 24) + 1),
               dict(n_epochs=64), dict(mask_a=A.reshape(2, 2, 3)), dict(n_rows=5), dict(mask_b=A[:, :2]), dict(base=A[0, :2]),
               dict(mode="rows", mask_b=A), dict(mode="rows", positions_a=pos), dict(positions_b=pos),
               dict(positions_a=pos, mask_b=A), dict(positions_a=pos[:3]), dict(positions_a=pos.astype(np.float64)),
               dict(positions_a=pos + 2 ** 29 + 1), dict(d2_min=-1), dict(d2_max=2 ** 64)):
        args = dict(mask_a=A, n_epochs=130)
        args.update(kw)
        with pytest.raises(ValueError):
            rt.mask_pairs(**args)


# ---- networks.py -------------------------------------------------------------------------------------------------------------
def test_point_positions_are_node_positions():
    H, W = 180, 360
    for window, unit in (((10, 300, 24, 24, 4), 0.01), ((0, 0, 5, 360, 1, 1), 1.0), ((170, 10, 10, 7, 1), 0.5)):
        w = tv.window_dict(window)
        heights = np.random.default_rng(2).uniform(-3000, 3000, (w["rows"], w["cols"]))
        want = rg.node_positions(window, (H, W), unit_m=unit, heights_m=heights)
        row = w["row0"] + np.arange(w["rows"]) * w["stride"]
        col = (w["col0"] + np.arange(w["cols"]) * w["stride"]) % W
        lat = np.degrees(0.5 * np.pi - (row + 0.5) * (np.pi / H))
        lon = np.degrees(-np.pi + (col + 0.5) * (2.0 * np.pi / W))
        la, lo = (a.ravel() for a in np.meshgrid(lat, lon, indexing="ij"))
        got = nw.point_positions(la, lo, 1737400.0, unit, heights.ravel())
        assert got.dtype == np.int32 and np.array_equal(got, want.reshape(-1, 3))
    with pytest.raises(ValueError):
        nw.point_positions([0.0], [0.0], 1737400.0, 1e-3)              # 1.7e9 units leave +-2^29
    with pytest.raises(ValueError):
        nw.point_positions([0.0, 1.0], [0.0], 1737400.0, 1.0)


def test_distances_round_inward():
    assert nw.distance_d2(5.0, 1.0, True) == 25 == nw.distance_d2(5.0, 1.0, False)
    assert nw.distance_d2(2.5, 1.0, True) == 7 and nw.distance_d2(2.5, 1.0, False) == 6
    assert nw.distance_d2(5000.0, 0.01, True) == nw.distance_d2(5000.0, 0.01, False) + 1        # 0.01 is no binary fraction
    assert nw.distance_d2(1e30, 1.0, False) == 2 ** 64 - 1 and nw.distance_d2(0.0, 1.0, True) == 0
    for bad in ((-1.0, 1.0), (float("nan"), 1.0), (1.0, 0.0)):
        with pytest.raises(ValueError):
            nw.distance_d2(*bad, True)
    # what site_pairs hands to the device
    seen = {}

    class Spy:
        @staticmethod
        def mask_pairs(mask, n, **kw):
            seen.update(kw)
            return pm.mask_pairs(mask, n, **kw)
    A = pm.pack(np.ones((3, 10), bool))
    nw.site_pairs(Spy, A, 10, positions=np.zeros((3, 3), np.int32), unit_m=1.0, min_dist_m=1.5, max_dist_m=2.5)
    with pytest.raises(ValueError):
        nw.site_pairs(Spy, A, 10, max_dist_m=3.0)
    # the band reached the BEST call (the ROWS call after it carries none)
    assert nw.distance_d2(1.5, 1.0, True) == 3 and nw.distance_d2(2.5, 1.0, False) == 6


def test_site_pairs_and_top_on_the_model():
    rng = np.random.default_rng(8)
    m, n = 150, 12
    bits = night_rows(rng, n, m)
    bits[5] = bits[2]                                       # equal sites: pairs that tie
    pos = np.stack([np.arange(n) * 10, np.zeros(n, int), np.zeros(n, int)], -1)
    for rank in ("count", "gap"):
        sp = nw.site_pairs(StubRT, pm.pack(bits), m, positions=pos, unit_m=1.0, min_dist_m=10.0, max_dist_m=30.0, rank=rank)
        assert np.array_equal(sp.best, pm.mask_pairs(pm.pack(bits), m, rank=rank, positions_a=pos, d2_min=100, d2_max=900))
        assert np.array_equal(sp.own, pm.mask_pairs(pm.pack(bits), m, mode="rows"))
        for a in range(n):
            b = int(sp.best["partner"][a])
            assert 1 <= abs(a - b) <= 3
            assert sp.gain[a] == int((bits[a] | bits[b]).sum()) - max(int(bits[a].sum()), int(bits[b].sum())) >= 0
        top = sp.top(4)
        assert len(top) == 4 and len({(int(r["a"]), int(r["b"])) for r in top}) == 4 and (top["a"] < top["b"]).all()
        every = sp.top(10 ** 6)
        key = [((-int(r["count"]), int(r["gap"])) if rank == "count" else (int(r["gap"]), -int(r["count"])), int(r["a"]), int(r["b"]))
               for r in every]
        assert key == sorted(key) and np.array_equal(every[:4], top)
        assert {(int(r["a"]), int(r["b"])) for r in every} == {(min(a, int(b)), max(a, int(b))) for a, b in enumerate(sp.best["partner"])}
    alone = nw.site_pairs(StubRT, pm.pack(bits[:1]), m)
    assert alone.best["partner"][0] == -1 and alone.gain[0] == 0 and len(alone.top(3)) == 0


def test_greedy_sites_on_the_model():
    rng = np.random.default_rng(21)
    m, n = 200, 10
    bits = night_rows(rng, n, m, nights=4) & (rng.random((n, m)) < 0.97)
    words = pm.pack(bits)
    for rank in ("count", "gap"):
        g = nw.greedy_sites(StubRT, words, m, 4, rank=rank)
        union = np.zeros(m, bool)
        for step, (site, rec) in enumerate(zip(g.sites, g.records)):
            cands = [(((-c, q) if rank == "count" else (q, -c)), i) for i in range(n) if i not in g.sites[:step]
                     for c, q, _ in [pm.stats_loop(bits[i] | union)]]
            assert min(cands)[1] == site
            union |= bits[site]
            assert tuple(rec) == (-1,) + pm.stats_loop(union)
        assert len(set(g.sites.tolist())) == len(g.sites) and (np.diff(g.records["count"].astype(np.int64)) >= 0).all()
    # complementary rows: complete after two steps, and no third
    halves = pm.pack(np.array([np.arange(m) < 120, np.arange(m) >= 120, np.ones(m, bool) & (np.arange(m) % 2 == 0)]))
    g = nw.greedy_sites(StubRT, halves, m, 3)
    assert g.sites.tolist() == [0, 1] and g.complete and g.records["gap"][-1] == 0 and g.records["gap_first"][-1] == -1
    # within_m: from the second site on only neighbours of a chosen site, compared in integers (inclusive)
    pos = np.array([[0, 0, 0], [100, 0, 0], [3, 4, 0]])
    g = nw.greedy_sites(StubRT, halves, m, 3, positions=pos, within_m=5.0)
    assert g.sites.tolist() == [0, 2] and not g.complete
    assert nw.greedy_sites(StubRT, halves, m, 3, positions=pos, within_m=4.99).sites.tolist() == [0]
    for kw in (dict(k=0), dict(k=65), dict(rank="best"), dict(within_m=5.0)):
        args = dict(k=2)
        args.update(kw)
        with pytest.raises(ValueError):
            nw.greedy_sites(StubRT, halves, m, **args)
