"""The built cases of tests/traverse_edge_cases.py without a GPU: the model's start() against the tick-by-tick
search on tables that cross 64-epoch words; from start_trace alone, how many pairs of each pair lattice run each path of the
timed edge rule; mutants of start() and a small emulator of the tile scheme with switchable defects, which show that the cases
tell a wrong kernel from a right one; the grade limit at equality; and the builders' own invariants."""
import collections

import numpy as np
import pytest

import timed_traverse_model as ttm
import traverse_edge_cases as ec
import traverse_model as tm
from traverse_model import DI, DJ

NEVER = ttm.NEVER
# name: (n_epochs, ticks_per_epoch, origin, direction shift, seed): n_epochs & 63 = 0, 1 and 63
TABLES = {"n320": (320, 7, (0, 0), 0, 1), "n321": (321, 2, (1, 1), 3, 2), "n319": (319, 1, (2, 0), 6, 3)}
_LAT = {}


def lattice(name):
    if name not in _LAT:
        n, tpe, origin, shift, seed = TABLES[name]
        _LAT[name] = ec.timed_lattice(n, tpe, origin, shift, seed)
    return _LAT[name]


def both_of(lat, p):
    return [a and b for a, b in zip(lat.ok_u[p], lat.ok_v[p])]


# ---- (a) start() on tables that cross words ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [63, 64, 65, 127, 128, 129, 191, 193, 300])
def test_start_agrees_with_the_tick_by_tick_search_across_words(n):
    rng = np.random.default_rng(1000 + n)
    seen = collections.Counter()
    for tpe in (1, 2, 7):
        for _ in range(150):
            style = rng.integers(0, 3)
            if style == 0:
                ok = ec._runs(n, rng, on=float(rng.choice([20, 80, 300])), off=float(rng.choice([1, 3, 70])))
            elif style == 1:
                ok = (rng.random(n) < 0.97).tolist()
            else:                                       # open but for the epochs around the word boundaries
                ok = [True] * n
                for b in range(63, n, 64):
                    for e in (b, b + 1):
                        if e < n and rng.random() < 0.4:
                            ok[e] = False
            q = int(np.exp(rng.uniform(0.0, np.log(200 * tpe)))) if rng.random() < 0.7 else int(rng.integers(1, 200 * tpe + 1))
            a = int(rng.integers(0, n)) * tpe if rng.random() < 0.4 else int(rng.integers(0, n * tpe))
            want = ttm.start_brute(ok, a, q, tpe)
            tr = ttm.start_trace(ok, a, q, tpe)
            assert ttm.start(ok, a, q, tpe) == want == tr.t, (ok, a, q, tpe)
            seen["on" if a % tpe == 0 else "off"] += 1
            seen["none"] += want is None
            seen["crossed"] += tr.boundaries >= 1
            seen["restarted"] += tr.restarts >= 1
            seen["long"] += q >= 64 * tpe
    assert seen["on"] >= 40 and seen["off"] >= 40 and seen["none"] >= 10 and seen["restarted"] >= 5, seen
    if n >= 127:
        assert seen["crossed"] >= 10 and seen["long"] >= 10, seen


def test_start_trace_is_start():
    assert ttm.start_trace(None, 17, 5, 3) == ttm.Trace(17, 0, 0, False, False, [])
    tr = ttm.start_trace([False, True, True, False, True, True, True], 0, 9, 4)
    assert tr.t == 16 and tr.restarts == 1 and tr.attempts == [(1, 3, 3), (4, 6, None)] and not tr.past_table
    assert ttm.start_trace([True, True], 1, 8, 4) == ttm.Trace(None, 0, 0, False, True, [(0, 2, None)])
    ok = [True] + [False] * 200 + [True] * 100
    tr = ttm.start_trace(ok, 3, 500, 7)
    assert tr.t == 201 * 7 and tr.skipped_zero_word and tr.boundaries == (201 + 71) // 64 - 201 // 64


# ---- (b) class counts, from the model alone -----------------------------------------------------------------------------------
def classes_of(lat, p):
    """The paths of the timed edge rule that pair p runs, from start_trace and the pair's rows."""
    u, v, both = lat.ok_u[p], lat.ok_v[p], both_of(lat, p)
    a, q, tpe, n = int(lat.start[p]), lat.q[p], lat.tpe, lat.n_epochs
    tr = ttm.start_trace(both, a, q, tpe)
    assert tr.t == ttm.start(both, a, q, tpe)
    ea = a // tpe
    out = set()
    first = tr.attempts[0] if tr.attempts else None
    if first is not None and first[0] > ea:
        out.add("wait_same_word" if first[0] // 64 == ea // 64 else "wait_later_word")
    if tr.skipped_zero_word and tr.t is not None:
        out.add("wait_skips_zero_word")
    if tr.t == a and q <= tpe and (a + q) % tpe == 0 and ea + 1 < n and not both[ea + 1]:
        out.add("ends_on_last_tick")
    if first is not None and first == (ea, ea + 1, ea + 1) and a + q - 1 == (ea + 1) * tpe and q <= tpe + 1 and tr.t is not None:
        out.add("one_tick_more_restarts")
    if tr.t is not None and tr.boundaries == 1:
        out.add("crosses_one_word")
    if tr.t is not None and tr.boundaries >= 3:
        out.add("spans_two_words")
    for e0, last, z in tr.attempts:
        if z is None:
            continue
        if last // 64 == e0 // 64 + 1 and z == 64 * (last // 64) - 1:
            out.add("blocked_at_bit_63")
        if last // 64 == e0 // 64 + 1 and z == 64 * (last // 64):
            out.add("blocked_at_bit_0")
        if last // 64 >= e0 // 64 + 3 and z // 64 == e0 // 64 + 2:
            out.add("spans_two_words_blocked_in_third")
    if tr.t is not None and (tr.t + q - 1) // tpe == n - 1:
        out.add("last_tick_in_last_epoch")
    if tr.past_table and tr.attempts[-1][1] == n:
        out.add("last_tick_past_table")
    if tr.t is None and any(u) and any(v) and not any(both):
        out.add("never_jointly")
    if not u[ea]:
        out.add("source_closed_at_start")
    if q == 1:
        out.add("q_is_1")
    return out


ALL_CLASSES = ("wait_same_word", "wait_later_word", "wait_skips_zero_word", "ends_on_last_tick", "one_tick_more_restarts",
               "crosses_one_word", "blocked_at_bit_63", "blocked_at_bit_0", "spans_two_words", "spans_two_words_blocked_in_third",
               "last_tick_in_last_epoch", "last_tick_past_table", "never_jointly", "source_closed_at_start", "q_is_1")


@pytest.mark.parametrize("name", list(TABLES))
def test_every_class_holds_at_least_8_pairs(native_lib, name):
    lat = lattice(name)
    assert lat.n_epochs & 63 == {"n320": 0, "n321": 1, "n319": 63}[name] and lat.n >= 480
    count = collections.Counter(c for p in range(lat.n) for c in classes_of(lat, p))
    print(name, dict(count))
    assert all(count[c] >= 8 for c in ALL_CLASSES), {c: count[c] for c in ALL_CLASSES}
    # A[v] of every pair is g_uv(start_u), and v's code is the pair's direction
    A, pred = ttm.field(lat.dem, lat.t, lat.src, lat.start, lat.P, lat.avail, lat.tpc, lat.tpe)
    s = lat.sites
    for p in range(lat.n):
        t = ttm.start(both_of(lat, p), int(lat.start[p]), lat.q[p], lat.tpe)
        assert int(A[s["vi"][p], s["vj"][p]]) == (NEVER if t is None else t + lat.q[p])
        assert pred[s["vi"][p], s["vj"][p]] == (255 if t is None else s["k"][p]) and pred[s["ui"][p], s["uj"][p]] == 8
    # the garbage past the table is there, in both rows of some pairs at once
    if lat.n_epochs & 63:
        ext = ec.unpacked_all(ec.packed(lat.avail, seed=5))
        assert ext[..., lat.n_epochs:].mean() > 0.4
        assert np.array_equal(ext[..., :lat.n_epochs], lat.avail)


def test_big_ticks_cross_2_to_the_32(native_lib):
    lat = ec.big_tick_lattice()
    assert lat.tpe == (1 << 31) - 1 and lat.tpc == 1.0
    x = lat.pair_weights().astype(np.float64) * lat.tpc
    assert ((x > 2.0 ** 30) & (x <= 2.0 ** 31)).sum() >= 1 and (x > 2.0 ** 31).sum() >= 1
    assert all((q is None) == (xx > 2.0 ** 31) for q, xx in zip(lat.q, x))
    crossing = above = 0
    for p in range(lat.n):
        if lat.q[p] is None:
            continue
        t = ttm.start(both_of(lat, p), int(lat.start[p]), lat.q[p], lat.tpe)
        if t is not None:
            crossing += t < 1 << 32 <= t + lat.q[p] - 1
            above += t > 1 << 32 and int(lat.start[p]) > 1 << 32
    assert crossing >= 8 and above >= 8, (crossing, above)
    A, pred = ttm.field(lat.dem, lat.t, lat.src, lat.start, lat.P, lat.avail, lat.tpc, lat.tpe)
    s = lat.sites
    dead = np.array([q is None for q in lat.q])
    assert (A[s["vi"][dead], s["vj"][dead]] == NEVER).all() and (pred[s["vi"][dead], s["vj"][dead]] == 255).all()
    assert (A[s["vi"][~dead], s["vj"][~dead]] != NEVER).sum() >= 100


# ---- (c) the cases tell a wrong rule from a right one -------------------------------------------------------------------------
def start_mutant(ok, a, q, tpe, kind):
    """start() with one defect: `last_from_t_plus_q`, `no_restart` (gives up at the first blocking epoch) or
    `zero_scan_two_words` (looks for a blocking epoch in the word of the drive's first epoch and the next one only)."""
    n = len(ok)
    t = a
    while True:
        e = t // tpe
        while e < n and not ok[e]:
            e += 1
        if e >= n:
            return None
        if e > t // tpe:
            t = e * tpe
        last = (t + q) // tpe if kind == "last_from_t_plus_q" else (t + q - 1) // tpe
        lim = min(last, 64 * (e // 64 + 2) - 1) if kind == "zero_scan_two_words" else last
        z = e
        while z < n and z <= lim and ok[z]:
            z += 1
        if z > lim:
            return t
        if kind == "no_restart":
            return None
        t = (z + 1) * tpe


@pytest.mark.parametrize("name", list(TABLES))
def test_mutants_of_start_change_a_pair(native_lib, name):
    lat = lattice(name)
    true = [ttm.start(both_of(lat, p), int(lat.start[p]), lat.q[p], lat.tpe) for p in range(lat.n)]
    for kind in ("last_from_t_plus_q", "no_restart", "zero_scan_two_words"):
        got = [start_mutant(both_of(lat, p), int(lat.start[p]), lat.q[p], lat.tpe, kind) for p in range(lat.n)]
        changed = sum(g != t for g, t in zip(got, true))
        print(name, kind, changed)
        assert changed >= 1, kind
    if lat.n_epochs & 63:
        # the tail mask ignored: the garbage bits past the table count as epochs
        ext = ec.unpacked_all(ec.packed(lat.avail, seed=5))
        s = lat.sites
        got = [ttm.start((ext[s["ui"][p], s["uj"][p]] & ext[s["vi"][p], s["vj"][p]]).tolist(), int(lat.start[p]), lat.q[p], lat.tpe)
               for p in range(lat.n)]
        changed = sum(g != t for g, t in zip(got, true))
        print(name, "tail mask ignored", changed)
        assert changed >= 1


def halo_mask(a, b, th, tw):
    n_, s_, w_, e_ = a == 0, a == th - 1, b == 0, b == tw - 1
    return (n_ * 1 | (n_ and e_) * 2 | e_ * 4 | (s_ and e_) * 8 | s_ * 16 | (s_ and w_) * 32 | w_ * 64 | (n_ and w_) * 128)


def emulate(rows, cols, wrap, ts, sources, edge, never, defects=()):
    """The tile scheme of DESIGN.md section 4.14 over any monotone edge rule edge(k, vi, vj, ui, uj, xu) -> value or None:
    seeds and their 3 x 3 tiles, launches over the flagged tiles, each tile relaxed to its fixed point against a halo read
    at the start of the launch (the stalest view the memory rule allows), its lowered nodes written back and the neighbour
    tiles that hold one in their halo flagged.  defects: `no_diagonal_flags`, `no_flag_wrap`, `seed_own_tile_only`.
    Returns (values as nested lists, launches)."""
    ty_n, tx_n = -(-rows // ts), -(-cols // ts)
    x = [[never] * cols for _ in range(rows)]

    def flag(flags, y, xx):
        if y < 0 or y >= ty_n:
            return
        if xx < 0 or xx >= tx_n:
            if not wrap or "no_flag_wrap" in defects:
                return
            xx %= tx_n
        flags.add((y, xx))

    flags = set()
    for (i, j), c in sources.items():
        x[i][j] = min(x[i][j], c)
        r = (0,) if "seed_own_tile_only" in defects else (-1, 0, 1)
        for a in r:
            for b in r:
                flag(flags, i // ts + a, j // ts + b)
    launches = 0
    while flags:
        snap = [row[:] for row in x]
        out = set()
        for ty, tx in sorted(flags):
            i0, j0 = ty * ts, tx * ts
            th, tw = min(ts, rows - i0), min(ts, cols - j0)
            val = {}
            for a in range(-1, th + 1):
                for b in range(-1, tw + 1):
                    gi, gj = i0 + a, j0 + b
                    if wrap:
                        gj %= cols
                    if 0 <= gi < rows and 0 <= gj < cols:
                        val[a, b] = snap[gi][gj]
            work = collections.deque(ab for ab, xv in val.items() if xv != never)
            while work:
                a, b = work.popleft()
                xu = val[a, b]
                for k in range(8):
                    va, vb = a - DI[k], b - DJ[k]
                    if not (0 <= va < th and 0 <= vb < tw):
                        continue
                    c = edge(k, i0 + va, j0 + vb, i0 + a, (j0 + b) % cols, xu)
                    if c is not None and c < val[va, vb]:
                        val[va, vb] = c
                        work.append((va, vb))
            mask = 0
            for a in range(th):
                for b in range(tw):
                    if val[a, b] < x[i0 + a][j0 + b]:
                        x[i0 + a][j0 + b] = val[a, b]
                        mask |= halo_mask(a, b, th, tw)
            for k in range(8):
                if mask >> k & 1 and not (k & 1 and "no_diagonal_flags" in defects):
                    flag(out, ty + DI[k], tx + DJ[k])
        flags = out
        launches += 1
    return x, launches


def cost_rule(dem, t, P):
    wl = tm.weights(tm.window_D(dem, t), P, tm.lengths(t, dem.shape), t).astype(np.float64).tolist()
    return lambda k, vi, vj, ui, uj, xu: None if wl[k][vi][vj] == np.inf else xu + wl[k][vi][vj]


def timed_rule(dem, t, P, avail, tpc, tpe):
    ql = ttm.durations(tm.weights(tm.window_D(dem, t), P, tm.lengths(t, dem.shape), t), tpc)
    rows_of = ttm.both_rows(avail)
    return lambda k, vi, vj, ui, uj, xu: ttm.arrive(rows_of, ql, tpe, k, vi, vj, ui, uj, xu)


DEFECTS = ("no_diagonal_flags", "no_flag_wrap", "seed_own_tile_only")


def test_the_emulator_is_the_model_and_every_defect_shows_on_a_corridor(native_lib):
    caught = {(d, ts): [] for d in DEFECTS for ts in (8, 16, 32)}
    for name in ec.CORRIDORS:
        dem, t, src, P, on = ec.corridor(name)
        c = ec.CORRIDOR_TIMED
        av = ec.corridor_mask(name)
        d_want = tm.field(dem, t, src, None, P)[0]
        A_want = ttm.field(dem, t, src, c["ticks"], P, av, c["tpc"], c["tpe"])[0]
        rule_d, rule_A = cost_rule(dem, t, P), timed_rule(dem, t, P, av, c["tpc"], c["tpe"])
        src_d, src_A = tm.reduce_sources(src), ttm.reduce_sources(src, c["ticks"])
        for ts in (8, 16, 32):
            d, launches = emulate(64, 64, t.wrap, ts, src_d, rule_d, np.inf)
            assert np.array_equal(np.array(d), d_want) and launches >= 32 // ts, (name, ts)         # tile by tile, from the source
            A, _ = emulate(64, 64, t.wrap, ts, src_A, rule_A, NEVER)
            assert np.array_equal(np.array(A, np.uint64), A_want), (name, ts)
            for defect in DEFECTS:
                bad, _ = emulate(64, 64, t.wrap, ts, src_d, rule_d, np.inf, (defect,))
                badA, _ = emulate(64, 64, t.wrap, ts, src_A, rule_A, NEVER, (defect,))
                differs = not np.array_equal(np.array(bad), d_want)
                assert differs == (not np.array_equal(np.array(badA, np.uint64), A_want))
                if differs:
                    caught[defect, ts].append(name)
    print(caught)
    assert all(caught.values()), caught


@pytest.mark.parametrize("name", list(ec.THIN))
def test_the_emulator_is_the_model_on_thin_windows(native_lib, name):
    dem, t, src, c0, ticks, av = ec.thin(name)
    c = ec.THIN_TIMED
    d_want = tm.field(dem, t, src, c0)[0]
    A_want = ttm.field(dem, t, src, ticks, None, av, c["tpc"], c["tpe"])[0]
    if t.rows * t.cols > 1:
        assert np.isfinite(d_want).mean() > 0.5 and (A_want != NEVER).mean() > 0.5          # the relief is driven, not walled
    for ts in (8, 16, 32):
        d, _ = emulate(t.rows, t.cols, t.wrap, ts, tm.reduce_sources(src, c0), cost_rule(dem, t, None), np.inf)
        assert np.array_equal(np.array(d), d_want), ts
        A, _ = emulate(t.rows, t.cols, t.wrap, ts, ttm.reduce_sources(src, ticks), timed_rule(dem, t, None, av, c["tpc"], c["tpe"]), NEVER)
        assert np.array_equal(np.array(A, np.uint64), A_want), ts


def test_corridors_are_reached_along_their_diagonal(native_lib):
    for name in ec.CORRIDORS:
        dem, t, src, P, on = ec.corridor(name)
        c = ec.CORRIDOR_TIMED
        for want in (tm.field(dem, t, src, None, P), ttm.field(dem, t, src, c["ticks"], P, ec.corridor_mask(name), c["tpc"], c["tpe"]),
                     ttm.field(dem, t, src, c["ticks"], P, None, c["tpc"], c["tpe"])):
            check_corridor(name, want, src, on)


def check_corridor(name, want, src, on):
    """Every corridor node is reached, by the corridor's diagonal; everything off the corridor is 255."""
    val, pred = want
    reached = np.isfinite(val) if val.dtype == np.float64 else val != np.uint64(NEVER)
    assert np.array_equal(reached, on), name
    assert (pred[~on] == 255).all(), name
    before, after = ec.corridor_codes(name)
    si = src[0][0]
    for i, j in np.argwhere(on):
        assert pred[i, j] == (8 if i == si else before if i > si else after), (name, i, j)


# ---- (d) the grade limit at equality --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(ec.GRADE_KINDS))
def test_the_grade_limit_counts_equality_as_driven(native_lib, kind):
    lat, tight = ec.grade_lattice(kind), ec.grade_lattice(kind, tight=True)
    assert np.float32(lat.max_grade) == lat.g32 and np.float32(tight.max_grade) == np.nextafter(lat.g32, np.float32(0))
    assert 0.03 < lat.g32 < 0.08
    s = lat.sites
    L = ec.edge_lengths(s)
    d, pred = tm.field(lat.dem, lat.t, lat.src, None, lat.P)
    dt, _ = tm.field(tight.dem, tight.t, tight.src, None, tight.P)
    seen = collections.Counter()
    for p in range(lat.n):
        var = lat.variant[p]
        if var is None:
            continue
        Du, Dv = lat.dem[ec.ROW0 + s["ui"][p], ec.COL0 + s["uj"][p]], lat.dem[ec.ROW0 + s["vi"][p], ec.COL0 + s["vj"][p]]
        g = ec.grade32(Du, Dv, L[p])
        reach, reach_tight = np.isfinite(d[s["vi"][p], s["vj"][p]]), np.isfinite(dt[s["vi"][p], s["vj"][p]])
        if var in ("climb", "descend"):             # g == gmax is driven; under the next float32 below it is not
            assert abs(g) == lat.g32 and (g > 0) == (var == "climb") and reach and not reach_tight, (p, var)
            assert pred[s["vi"][p], s["vj"][p]] == s["k"][p]
        elif var in ("climb_above", "descend_below"):   # v one float32 further from u's height: steeper, not driven
            assert abs(g) > lat.g32 and not reach and not reach_tight, (p, var)
        else:                                       # v one float32 nearer: driven
            assert abs(g) < lat.g32 and reach, (p, var)
        seen[var] += 1
    assert all(seen[v] >= 2 for v in ec.GRADE_VARIANTS), seen
    rest = np.array([v is None for v in lat.variant])
    share = np.isfinite(d[s["vi"][rest], s["vj"][rest]]).mean()
    assert 0.25 < share < 0.75, share                   # the other pairs fall on both sides of the limit


# ---- (e) the builders' invariants -----------------------------------------------------------------------------------------------
def test_walled_nodes_are_unreachable_and_pairs_are_independent(native_lib):
    lat = lattice("n320")
    run_t = lambda l: ttm.field(l.dem, l.t, l.src, l.start, l.P, l.avail, l.tpc, l.tpe)
    cl = ec.cost_lattice()
    run_c = lambda l: tm.field(l.dem, l.t, l.src, l.start, l.P)
    for l, run, never in ((lat, run_t, np.uint64(NEVER)), (cl, run_c, np.inf)):
        val, pred = run(l)
        assert (pred[l.walled()] == 255).all() and (val[l.walled()] == never).all()
        assert l.walled().sum() == l.P.size - 2 * l.n
        s = l.sites
        assert (pred[s["ui"], s["uj"]] == 8).all()
        for p in (0, 7, l.n // 2, l.n - 1):
            v2, p2 = run(l.without(p))
            keep = np.ones(l.P.shape, bool)
            keep[[s["ui"][p], s["vi"][p]], [s["uj"][p], s["vj"][p]]] = False
            assert np.array_equal(val[keep], v2[keep]) and np.array_equal(pred[keep], p2[keep])
            assert (p2[~keep] == 255).all()
    # the cost lattice: d[v] = c0 + (double)w exactly, at 2^52 a rounded sum
    d, pred = run_c(cl)
    w = cl.pair_weights().astype(np.float64)
    s = cl.sites
    assert np.array_equal(d[s["vi"], s["vj"]], cl.start + w) and np.array_equal(pred[s["vi"], s["vj"]], s["k"])
    big = cl.start == 2.0 ** 52
    assert big.sum() >= 100 and (w[big] != np.round(w[big])).sum() >= 8       # sums that are not exact
    P = cl.P[np.isfinite(cl.P)]
    assert (P == np.float32(1e-3)).sum() >= 100 and (P == np.float32(1e6)).sum() >= 100 and P.min() >= np.float32(1e-3)
