"""The built tables of the region kernels' run reductions without a GPU (tests/run_layout_cases.py; DESIGN.md sections 4.26 and
4.27): the classifier finds every named event in the table built for it; host simulators of the two carry rules and of the
histogram's carried columns, written from the design text, give the models' records (tests/regions_model.py,
tests/zonal_model.py) on every table; every named defect, a switch on a simulator, makes the tables listed in CAUGHT_BY differ
from the model, so a kernel with that defect would fail tests/test_gpu_run_layouts.py; and the closed forms of the rank tests
equal the model on small instances.

A simulator works on node values of three kinds: sums modulo 2^64, minima and maxima.  An emission is (label, value): what one
atomic add of the kernel carries.  The fixed point and the order key of a node's value are the model's own (zonal_model.fixed,
order_key): what is under test here is the bookkeeping of runs and carries, not the arithmetic of one node."""
import collections

import numpy as np
import pytest

import regions_model as model
import run_layout_cases as lc
import zonal_model as zm

U64, I64 = np.uint64, np.int64
TOP, BOTTOM = np.iinfo(I64).max, np.iinfo(I64).min
M31 = 2 ** 31 - 1
SCALE = 8.0


# ---- node values
class Vals:
    """Per node: add (M, a) uint64 summed modulo 2^64, lo (M, b) int64 under min, hi (M, c) int64 under max; M is the node
    count rounded up to whole steps.  Column 0 of add counts the nodes.  A node outside every region holds the identities."""

    def __init__(self, inside, add, lo=(), hi=()):
        n = len(inside)
        m = -(-n // lc.WAVE) * lc.WAVE
        self.add = np.zeros((m, len(add)), U64)
        self.lo = np.full((m, len(lo)), TOP, I64)
        self.hi = np.full((m, len(hi)), BOTTOM, I64)
        for k, col in enumerate(add):
            self.add[:n, k] = np.where(inside, np.asarray(col, U64), U64(0))
        for k, col in enumerate(lo):
            self.lo[:n, k] = np.where(inside, col, TOP)
        for k, col in enumerate(hi):
            self.hi[:n, k] = np.where(inside, col, BOTTOM)

    def none(self):
        return self.span(0, 0)

    def span(self, a, b):
        return [self.add[a:b].sum(0, dtype=U64), self.lo[a:b].min(0, initial=TOP), self.hi[a:b].max(0, initial=BOTTOM)]


def join(x, y):
    return [x[0] + y[0], np.minimum(x[1], y[1]), np.maximum(x[2], y[2])]


def total(emissions, vals, n):
    """Per label the emissions joined: add (n, a), lo (n, b), hi (n, c)."""
    out = [vals.none() for _ in range(n)]
    for l, v in emissions:
        out[l] = join(out[l], v)
    return [np.array([o[k] for o in out]).reshape(n, -1) for k in range(3)]


def as_u64(ints):
    return np.array([int(v) % 2 ** 64 for v in ints], U64)


# ---- the catalogue: stats_root_kernel's head filter and stats_sum_kernel<true>'s carry rule
def sim_roots(flat, n, drop_lane0=False):
    """The least node index among a label's candidates: a node whose lane is 0 or whose label differs from the node before."""
    flat = np.asarray(flat, I64)
    idx = np.arange(flat.size)
    lane0 = idx % lc.WAVE == 0
    differs = np.concatenate([[True], flat[1:] != flat[:-1]])
    cand = (flat >= 0) & (flat < n) & ((differs & ~lane0) if drop_lane0 else (differs | lane0))
    roots = np.full(n, M31, I64)                            # the record's identity
    np.minimum.at(roots, flat[cand], idx[cand])
    return roots


def catalogue_vals(flat, n, cols, wrap, weights, roots, past_as_label0=False):
    flat = np.asarray(flat, I64)
    inside = (flat >= 0) & (flat < n)
    idx = np.arange(flat.size)
    i, j = idx // cols, idx % cols
    dj = j - roots[np.where(inside, flat, 0)] % cols
    if wrap:
        dj = (dj + cols // 2) % cols - cols // 2
    w = np.ones(flat.size, U64) if weights is None else np.asarray(weights, U64)[i]
    v = Vals(inside, [np.ones(flat.size, U64), w, i.astype(U64), dj.astype(I64).view(U64)], [i, dj], [i, dj])
    if past_as_label0:                                       # what a lane past the last node adds once it is counted
        v.add[flat.size:, 0] = 1
    return v


def sim_catalogue(flat, n, vals, defects=frozenset()):
    N, out = len(flat), []
    past = 0 if "lanes_past_n_read_label_0" in defects else -1
    for s in range(lc.n_stretches(N)):
        carry_l, carry = -1, vals.none()
        for t in range(lc.steps_in(N, s)):
            base = s * lc.STRETCH + t * lc.WAVE
            runs = lc.step_runs(lc.step_labels(flat, n, s, t, past), carry_l, "run_cut_at_a_hole" not in defects)
            recs = [vals.span(base + a, base + (lc.WAVE if "joins_past_the_run_end" in defects else b)) for _, a, b in runs]
            heads = [k for k, (l, _, _) in enumerate(runs) if l >= 0 and recs[k][0][0]]
            mine = [k for k in heads if runs[k][0] == carry_l]
            if mine:
                # every run of the carried label goes on the carried run; the other heads add to their records
                for k in mine[:1] if "several_matches_taken_as_one" in defects else mine:
                    carry = join(carry, recs[k])
                out += [(runs[k][0], recs[k]) for k in heads if k not in mine]
            else:
                # the carried run is over; the run that reaches lane 63 is carried instead
                if carry_l >= 0 and carry[0][0]:
                    out.append((carry_l, carry))
                last = len(runs) - 1
                out += [(runs[k][0], recs[k]) for k in heads if k != last or "carried_run_also_emitted" in defects]
                carry_l, carry = runs[last][0], recs[last]
        if carry_l >= 0 and carry[0][0] and "no_emit_after_the_stretch" not in defects:
            out.append((carry_l, carry))
    return out


def catalogue_records(flat, n, cols, wrap, weights, defects=frozenset()):
    """The catalogue as the kernels would leave it, and the number of emissions."""
    roots = sim_roots(flat, n, "root_filter_drops_lane_0" in defects)
    vals = catalogue_vals(flat, n, cols, wrap, weights, roots, "lanes_past_n_read_label_0" in defects)
    em = sim_catalogue(flat, n, vals, defects)
    add, lo, hi = total(em, vals, n)
    t = np.zeros(n, model.RECORD)
    some = add[:, 0] > 0
    t["count"], t["weight"], t["sum_i"], t["sum_dj"] = add[:, 0], add[:, 1], add[:, 2].view(I64), add[:, 3].view(I64)
    t["root_i"], t["root_j"] = np.where(some, roots // cols, -1), np.where(some, roots % cols, -1)
    t["i_min"], t["dj_min"] = np.where(some, lo[:, 0], 0), np.where(some, lo[:, 1], 0)
    t["i_max"], t["dj_max"] = np.where(some, hi[:, 0], 0), np.where(some, hi[:, 1], 0)
    return t, len(em)


# ---- zonal statistics and shapes: wave_runs' carry rule
def sim_wave_runs(flat, n, vals, defects=frozenset()):
    N, out = len(flat), []
    past = 0 if "lanes_past_n_read_label_0" in defects else -1
    for s in range(lc.n_stretches(N)):
        carry_l, carry = -1, vals.none()
        for t in range(lc.steps_in(N, s)):
            base = s * lc.STRETCH + t * lc.WAVE
            runs = lc.step_runs(lc.step_labels(flat, n, s, t, past), carry_l, "run_cut_at_a_hole" not in defects)
            recs = [vals.span(base + a, base + (lc.WAVE if "joins_past_the_run_end" in defects else b)) for _, a, b in runs]
            # lane 0's run goes on the carried run when it has its label, else lane 0 adds the carried run to its record
            pending = carry_l >= 0 and carry[0][0]
            if runs[0][0] == carry_l or "lane0_joins_any_label" in defects:
                recs[0] = join(recs[0], carry)
                if pending and "lane0_emits_and_joins" in defects:
                    out.append((carry_l, carry))
            elif pending:
                out.append((carry_l, carry))
            last = len(runs) - 1
            out += [(runs[k][0], recs[k]) for k in range(len(runs))
                    if (k != last or "carried_run_also_emitted" in defects) and runs[k][0] >= 0 and recs[k][0][0]]
            carry_l, carry = runs[last][0], recs[last]
        if carry_l >= 0 and carry[0][0] and "no_emit_after_the_stretch" not in defects:
            out.append((carry_l, carry))
    return out


def zonal_vals(flat, n, x, cols, weights, scale, past_as_label0=False):
    flat = np.asarray(flat, I64)
    inside = (flat >= 0) & (flat < n)
    idx = np.arange(flat.size)
    nan = np.isnan(x)
    q, clipped = zm.fixed(np.where(nan, np.float32(0), x), scale)
    w = [1] * flat.size if weights is None else [int(weights[i]) for i in idx // cols]
    ok = (~nan).astype(U64)
    key = zm.order_key(x).astype(I64)
    v = Vals(inside, [np.ones(flat.size, U64), ok, nan.astype(U64), (clipped & ~nan).astype(U64), as_u64(w) * ok, as_u64(q) * ok,
                      as_u64([a * b for a, b in zip(w, q)]) * ok],
             [np.where(nan, TOP, key << 31 | idx)], [np.where(nan, BOTTOM, key << 31 | (M31 - idx))])
    if past_as_label0:
        v.add[flat.size:, 0] = 1
        v.add[flat.size:, 2] = 1                             # a value nobody wrote: counted as something, here as a NaN
    return v


def zonal_records(flat, n, x, cols, weights, scale=SCALE, defects=frozenset()):
    vals = zonal_vals(flat, n, x, cols, weights, scale, "lanes_past_n_read_label_0" in defects)
    em = sim_wave_runs(flat, n, vals, defects)
    add, lo, hi = total(em, vals, n)
    z = np.zeros(n, zm.ZONAL)
    z["count"], z["n_nan"], z["n_clipped"], z["wcount"] = add[:, 1], add[:, 2], add[:, 3], add[:, 4]
    z["sum"], z["wsum"] = add[:, 5].view(I64), add[:, 6].view(I64)
    z["min"], z["max"], z["min_at"], z["max_at"] = np.inf, -np.inf, -1, -1
    for r in np.flatnonzero(add[:, 1]):
        a, b = int(lo[r, 0]) & M31, M31 - (int(hi[r, 0]) & M31)
        z[r]["min"], z[r]["min_at"], z[r]["max"], z[r]["max_at"] = x[a], a, x[b], b
    return z, len(em)


def shape_vals(labels, n, wrap, side_ew=None, side_ns=None):
    """What a node adds to its own region: its boundary sides, and of the four 2 x 2 windows it lies in those in which no node
    before it (in the order NW, NE, SW, SE) carries its label."""
    L = np.asarray(labels, I64)
    rows, cols = L.shape
    P = np.full((rows + 2, cols + 2), -1, I64)
    P[1:-1, 1:-1] = L
    if wrap:
        P[1:-1, 0], P[1:-1, -1] = L[:, -1], L[:, 0]
    m = [[(a == 1 and b == 1) | (P[a:a + rows, b:b + cols] == L) for b in range(3)] for a in range(3)]
    ew = np.broadcast_to((np.ones(rows, U64) if side_ew is None else np.asarray(side_ew, U64))[:, None], L.shape)
    ns = np.ones(rows + 1, U64) if side_ns is None else np.asarray(side_ns, U64)
    north, south = np.broadcast_to(ns[:-1, None], L.shape), np.broadcast_to(ns[1:, None], L.shape)
    sides_ns = (~m[0][1]).astype(U64) + (~m[2][1]).astype(U64)
    sides_ew = (~m[1][0]).astype(U64) + (~m[1][2]).astype(U64)
    perimeter = ~m[0][1] * north + ~m[2][1] * south + (~m[1][0] * ew + ~m[1][2] * ew)
    q1, q3, qd = (np.zeros(L.shape, U64) for _ in range(3))
    for a in range(2):
        for b in range(2):
            w = [m[a][b], m[a][b + 1], m[a + 1][b], m[a + 1][b + 1]]        # NW, NE, SW, SE of the window
            me = (1 - a) * 2 + (1 - b)
            first = ~np.any(w[:me], axis=0) if me else np.ones(L.shape, bool)
            k = sum(v.astype(int) for v in w)
            q1 += first & (k == 1)
            q3 += first & (k == 3)
            qd += first & (k == 2) & ((w[0] & w[3]) | (w[1] & w[2]))
    inside = ((L >= 0) & (L < n)).reshape(-1)
    return Vals(inside, [np.ones(L.size, U64)] + [v.reshape(-1) for v in (perimeter, sides_ns, sides_ew, q1, q3, qd)])


def shape_records(labels, n, conn, wrap, defects=frozenset()):
    vals = shape_vals(labels, n, wrap)
    em = sim_wave_runs(np.asarray(labels).reshape(-1), n, vals, defects)
    add = total(em, vals, n)[0].astype(I64)
    s = np.zeros(n, zm.SHAPE)
    for k, name in enumerate(("perimeter", "sides_ns", "sides_ew", "q1", "q3", "qd")):
        s[name] = add[:, k + 1]
    s["euler"] = (add[:, 4] - add[:, 5] + (2 if conn == 4 else -2) * add[:, 6]) // 4
    return s, len(em)


# ---- the histogram's carried columns
def sim_hist(flat, n, is_open, col, w, width, defects=frozenset()):
    """(flat index into the n x width histogram, amount) per atomic add."""
    N, out = len(flat), []
    carrying = width <= lc.HCOLS
    for s in range(lc.n_stretches(N)):
        carried, acc = -1, collections.Counter()

        def flush():
            for c, v in acc.items():
                if "accumulators_swapped" in defects:
                    c ^= lc.WAVE
                out.append((carried * width + c, v))
            acc.clear()
        for t in range(lc.steps_in(N, s)):
            base = s * lc.STRETCH + t * lc.WAVE
            labs = lc.step_labels(flat, n, s, t)
            lanes = [k for k in range(min(lc.WAVE, N - base)) if labs[k] >= 0 and is_open[base + k]]
            if carrying and lanes:
                if labs[lanes[0]] != carried:               # the first open lane decides
                    if "no_flush_at_a_change" in defects:
                        acc.clear()
                    flush()
                    carried = labs[lanes[0]]
                for k in lanes:
                    if labs[k] == carried:
                        acc[int(col[base + k])] += int(w[base + k])
                lanes = [k for k in lanes if labs[k] != carried]
            keys = collections.OrderedDict()
            for k in lanes:
                keys.setdefault(labs[k] * width + int(col[base + k]), []).append(int(w[base + k]))
            for rank, (key, ws) in enumerate(keys.items()):
                if rank < lc.PEEL:
                    out.append((key, sum(ws)))
                elif "lanes_left_after_the_peels_dropped" not in defects:
                    out += [(key, v) for v in ws]
        if carrying:
            flush()
    return out


def hist_records(flat, n, x, cols, weights, n_bins, defects=frozenset()):
    is_open, col = lc.hist_columns(x, n_bins)
    w = np.ones(len(flat), I64) if weights is None else np.asarray(weights, I64)[np.arange(len(flat)) // cols]
    em = sim_hist(flat, n, is_open, col, w, n_bins + 2, defects)
    h = [0] * (n * (n_bins + 2))
    for k, v in em:
        if 0 <= k < len(h):                                 # a defect may add past the table's end: nothing to compare there
            h[k] += v
    return np.array([v % 2 ** 64 for v in h], U64).reshape(n, n_bins + 2), len(em)


# ---- fields and the models' answers
def field_for(N, seed):
    """(N,) float32: coarse values with NaN, infinities, both zeros and values that clip at SCALE sprinkled in."""
    k = np.arange(N, dtype=np.uint64)
    h = (k * 2654435761 + seed * 40503 + 977) % 4294967296
    h = ((h ^ (h >> 15)) * 2246822519) % 4294967296
    h ^= h >> 13
    x = ((h % 61).astype(np.float64) * 0.25 - 7.5).astype(np.float32)
    for mod, val in ((23, np.nan), (29, np.inf), (31, -np.inf), (37, -0.0), (41, 0.0), (43, 3.0e8), (47, -2.9e8)):
        x[h % mod == 0] = np.float32(val)
    return x


def first_difference(got, want):
    for name in got.dtype.names:
        a, b = got[name], want[name]
        if a.dtype.kind == "f":
            a, b = a.view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32)
        if not np.array_equal(a, b):
            k = int(np.flatnonzero(a != b)[0])
            return f"{name} differs, first in region {k}: {got[k]} vs {want[k]}"
    return None


CASES = lc.cases()


@pytest.mark.parametrize("case", CASES, ids=lc.case_id)
def test_the_simulators_equal_the_models(case):
    name, rows, cols, wrap = case
    flat, n, _ = lc.tables()[name]
    labels = flat.reshape(rows, cols)
    for weights in (None, lc.row_weights(rows)):
        got, _ = catalogue_records(flat, n, cols, wrap, weights)
        assert first_difference(got, model.catalogue(labels, n, wrap, weights)) is None
    if wrap and name != "carry":
        return                                              # what follows does not depend on wrap but for the shapes
    x = lc.hist_table()[2] if name == "hist" else field_for(flat.size, len(name))
    if not wrap:
        for weights in (None, lc.row_weights(rows)):
            got, _ = zonal_records(flat, n, x, cols, weights)
            assert first_difference(got, zm.zonal(labels, n, x.reshape(rows, cols, 1), SCALE, weights)[:, 0]) is None
    if flat.size <= 3000:
        for conn in (4, 8):
            got, _ = shape_records(labels, n, conn, wrap)
            assert first_difference(got, zm.shape(labels, n, conn, wrap)) is None


def test_the_shape_simulator_on_the_pairs():
    flat, n, shapes = lc.tables()["pairs"]
    labels = flat.reshape(shapes[0])
    got, _ = shape_records(labels, n, 8, True)
    assert first_difference(got, zm.shape(labels, n, 8, True)) is None


@pytest.mark.parametrize("n_bins", [w - 2 for w in lc.HIST_WIDTHS])
def test_the_histogram_simulator_equals_the_model(n_bins):
    flat, n, x = lc.hist_table()
    rows, cols = lc.tables()["hist"][2][0]
    for weights in (None, lc.row_weights(rows)):
        got, _ = hist_records(flat, n, x, cols, weights, n_bins)
        want = zm.histogram(flat.reshape(rows, cols), n, x.reshape(rows, cols), n_bins, 0.0, 1.0, weights)
        assert np.array_equal(got, want), n_bins


# ---- what the tables reach
def test_the_pairs_table_holds_every_pair_once():
    flat, n, _ = lc.tables()["pairs"]
    assert flat.size == 2080 * 64 == 130 * lc.STRETCH and n == 2082
    seen = collections.Counter()
    for k in range(2080):
        step = flat[k * 64:(k + 1) * 64]
        lanes = np.flatnonzero(step == k)
        assert lanes.size and (np.diff(lanes) == 1).all() and not (flat == k)[:k * 64].any() and not (flat == k)[(k + 1) * 64:].any()
        seen[(int(lanes[0]), int(lanes[-1]))] += 1
    assert sorted(seen) == lc.PAIRS and set(seen.values()) == {1}
    # both kinds of neighbour occur at both ends of a run
    before = {int(flat[k * 64 + a - 1]) >= 0 for k, (a, b) in enumerate(lc.PAIRS) if a > 0}
    after = {int(flat[k * 64 + b + 1]) >= 0 for k, (a, b) in enumerate(lc.PAIRS) if b < 63}
    assert before == after == {False, True}
    assert lc.lane_map(1024 * 5 + 64 * 3 + 17) == (5, 3, 17)


# the events a table is built for: it must show each of them at least once
BUILT_FOR = {
    "pairs": {"catalogue": {"single_match", "flush_no_match", "lane0_hole_takes_carry", "run_reaches_lane_63",
                            "carry_emitted_after_last_step"},
              "zonal": {"lane0_joins", "lane0_emits", "one_run_spans_step", "carry_emitted_after_last_step"}},
    "carry": {"catalogue": set(lc.CATALOGUE_EVENTS), "zonal": set(lc.ZONAL_EVENTS)},
    "tails": {"catalogue": {"partial_last_step", "carry_emitted_after_last_step", "run_reaches_lane_63"},
              "zonal": {"partial_last_step", "carry_emitted_after_last_step"}},
}


def test_every_named_event_occurs_in_the_table_built_for_it(capsys):
    seen = {}
    for name, (flat, n, _) in lc.tables().items():
        c = lc.classify(flat, n)
        assert sorted(c) == [(s, t) for s in range(lc.n_stretches(flat.size)) for t in range(lc.steps_in(flat.size, s))]
        group = "tails" if name.startswith("tails") else name
        for rule in ("catalogue", "zonal"):
            for e, at in lc.events_of(c, rule).items():
                seen.setdefault((group, rule), {}).setdefault(e, (name, at))
    with capsys.disabled():
        print()
        for (group, rule), ev in sorted(seen.items()):
            print(f"  {group:6s} {rule:9s} " + ", ".join(f"{e} {at[0] if group == 'tails' else ''}{at[1]}" for e, at in sorted(ev.items())))
    for group, rules in BUILT_FOR.items():
        for rule, events in rules.items():
            assert events <= set(seen[(group, rule)]), (group, rule, events - set(seen[(group, rule)]))
    # every tail with a ragged end has a partial last step, and a region reaches its last node
    for N in lc.TAIL_SIZES:
        flat, n, _ = lc.tables()[f"tails_{N}"]
        c = lc.classify(flat, n)
        last = max(c)
        assert last == ((N - 1) // lc.STRETCH, ((N - 1) % lc.STRETCH) // lc.WAVE) and flat[-1] == n - 1
        assert ("partial_last_step" in c[last]["catalogue"]) == (N % 64 != 0)
        assert "carry_emitted_after_last_step" in c[last]["catalogue"] and "carry_emitted_after_last_step" in c[last]["zonal"]
    # the carry table, step by step: what each step was built for
    flat, n, _ = lc.tables()["carry"]
    c = lc.classify(flat, n)
    want = {(0, 0): "no_match_nothing_carried", (0, 1): "single_match", (0, 2): "flush_no_match", (0, 3): "lane0_hole_takes_carry",
            (0, 4): "flush_no_match", (0, 6): "step_entirely_outside", (0, 7): "single_match", (0, 8): "single_match",
            (0, 9): "several_matches", (0, 10): "several_matches", (0, 11): "several_matches", (0, 12): "flush_no_match",
            (0, 13): "several_matches", (0, 14): "flush_no_match", (0, 15): "carry_emitted_after_last_step",
            (1, 0): "no_match_nothing_carried", (1, 4): "no_match_nothing_carried", (1, 6): "lane0_hole_takes_carry"}
    for at, e in want.items():
        assert e in c[at]["catalogue"], (at, e, c[at])
    assert "single_match" in c[(0, 3)]["catalogue"] and "flush_no_match" in c[(0, 6)]["catalogue"]
    assert {"lane0_hole_takes_carry", "flush_no_match"} <= c[(0, 4)]["catalogue"]
    for at, e in {(0, 1): "lane0_joins", (0, 2): "lane0_emits", (0, 5): "one_run_spans_step", (0, 7): "lane0_joins",
                  (0, 15): "carry_emitted_after_last_step", (1, 0): "one_run_spans_step"}.items():
        assert e in c[at]["zonal"], (at, e, c[at])
    assert "lane0_joins" not in c[(1, 0)]["zonal"] and "lane0_emits" not in c[(1, 0)]["zonal"]      # a new wave carries nothing
    assert not (flat == lc.CARRY_UNUSED).any()
    roots = sim_roots(flat, n)
    assert roots[lc.C_] % 64 == 0 and roots[lc.I_] % 64 == 63 and roots[lc.CARRY_UNUSED] == M31


def test_the_histogram_table_reaches_every_named_event(capsys):
    flat, n, x = lc.hist_table()
    for width in lc.HIST_WIDTHS:
        is_open, col = lc.hist_columns(x, width - 2)
        c = lc.classify_hist(flat, n, is_open, col, width)
        ev = lc.events_of(c)
        with capsys.disabled():
            print(f"\n  hist, width {width}: " + ", ".join(f"{e} {at}" for e, at in sorted(ev.items())), end="")
        inside = flat >= 0
        hit = set(col[is_open & inside].tolist())
        assert {0, 63, width - 1} <= hit and (width < 128 or {64, 127} <= hit)
        assert {"first_open_lane_not_lane0", "keys_left_after_8_peels"} <= set(ev)
        if width <= lc.HCOLS:
            assert "carried_region_changes" in c[(0, 2)] and "carried_region_changes" in c[(0, 3)]
            # step 4: lane 0 is NaN, lane 1 belongs to B while A is carried, and A's lanes come later
            assert {"carried_region_changes", "first_open_lane_not_lane0"} <= c[(0, 4)] and np.isnan(x[4 * 64])
            assert flat[4 * 64] == lc.A and flat[4 * 64 + 1] == lc.B and (flat[4 * 64 + 11:5 * 64] == lc.A).all()
            assert ("second_accumulator_used" in ev) == (width > 64)
        else:
            assert "carried_region_changes" not in ev and "second_accumulator_used" not in ev
        # step 5 holds at least 12 keys outside the carried region
        keys = {(int(l), int(k)) for l, k, o in zip(flat[320:384], col[320:384], is_open[320:384]) if o and l != lc.B}
        assert len(keys) >= 12 and "keys_left_after_8_peels" in c[(0, 5)]
        # the carried region's columns 0, 63, 64 and 127 of step 0 at width 128
        if width == 128:
            assert col[0:4].tolist() == [0, 63, 64, 127] and (flat[0:4] == lc.A).all()


# ---- named defects
GROUPS = ("pairs", "carry", "tails", "hist")
CATALOGUE_DEFECTS = ("no_emit_after_the_stretch", "several_matches_taken_as_one", "carried_run_also_emitted", "joins_past_the_run_end",
                     "lanes_past_n_read_label_0", "root_filter_drops_lane_0", "run_cut_at_a_hole")
ZONAL_DEFECTS = ("no_emit_after_the_stretch", "carried_run_also_emitted", "joins_past_the_run_end", "lanes_past_n_read_label_0",
                 "lane0_joins_any_label", "lane0_emits_and_joins", "run_cut_at_a_hole")
HIST_DEFECTS = ("no_flush_at_a_change", "accumulators_swapped", "lanes_left_after_the_peels_dropped")

# Which table (tails: any of them) differs from the model under which defect.  Identities:
#   run_cut_at_a_hole: a lane outside every region adds nothing, so cutting a run there changes how many atomics are issued
#       and no sum; asserted below by the emission counts.
#   several_matches_taken_as_one on pairs: no step of it holds two runs of the carried label (the fillers round a run are
#       two different labels or outside, and a filler outside takes the run's own label).
#   lanes_past_n_read_label_0 on pairs: its size is a multiple of 64, so no lane is past the last node.
#   the histogram's two carrying defects at width 129: rows of 129 columns are not carried.
CAUGHT_BY = {
    ("catalogue", "no_emit_after_the_stretch"): {"pairs", "carry", "tails", "hist"},
    ("catalogue", "several_matches_taken_as_one"): {"carry", "tails", "hist"},
    ("catalogue", "carried_run_also_emitted"): {"pairs", "carry", "tails", "hist"},
    ("catalogue", "joins_past_the_run_end"): {"pairs", "carry", "tails", "hist"},
    ("catalogue", "lanes_past_n_read_label_0"): {"carry", "tails", "hist"},
    ("catalogue", "root_filter_drops_lane_0"): {"pairs", "carry", "tails", "hist"},
    ("catalogue", "run_cut_at_a_hole"): set(),
    ("zonal", "no_emit_after_the_stretch"): {"pairs", "carry", "tails", "hist"},
    ("zonal", "carried_run_also_emitted"): {"pairs", "carry", "tails", "hist"},
    ("zonal", "joins_past_the_run_end"): {"pairs", "carry", "tails", "hist"},
    ("zonal", "lanes_past_n_read_label_0"): {"carry", "tails", "hist"},
    ("zonal", "lane0_joins_any_label"): {"pairs", "carry", "tails", "hist"},
    ("zonal", "lane0_emits_and_joins"): {"pairs", "carry", "tails", "hist"},
    ("zonal", "run_cut_at_a_hole"): set(),
}
HIST_CAUGHT_AT = {
    "no_flush_at_a_change": {64, 65, 128},
    "accumulators_swapped": {64, 65, 128},
    "lanes_left_after_the_peels_dropped": {64, 65, 128, 129},
}


def group_tables(group):
    return [(k, v) for k, v in lc.tables().items() if k == group or (group == "tails" and k.startswith("tails"))]


def test_every_named_defect_is_caught_by_the_tables_listed(capsys):
    matrix, counts = {}, {}
    for group in GROUPS:
        for name, (flat, n, shapes) in group_tables(group):
            rows, cols = shapes[0]
            labels = flat.reshape(rows, cols)
            w = lc.row_weights(rows)
            x = lc.hist_table()[2] if name == "hist" else field_for(flat.size, len(name))
            want_c = model.catalogue(labels, n, False, w)
            want_z = zm.zonal(labels, n, x.reshape(rows, cols, 1), SCALE, w)[:, 0]
            clean = {"catalogue": catalogue_records(flat, n, cols, False, w)[1], "zonal": zonal_records(flat, n, x, cols, w)[1]}
            for rule, defects in (("catalogue", CATALOGUE_DEFECTS), ("zonal", ZONAL_DEFECTS)):
                for d in defects:
                    if rule == "catalogue":
                        got, k = catalogue_records(flat, n, cols, False, w, frozenset([d]))
                        differs = first_difference(got, want_c) is not None
                    else:
                        got, k = zonal_records(flat, n, x, cols, w, defects=frozenset([d]))
                        differs = first_difference(got, want_z) is not None
                    if differs:
                        matrix.setdefault((rule, d), set()).add(group)
                    else:
                        matrix.setdefault((rule, d), set())
                    counts.setdefault((rule, d), []).append(k - clean[rule])
    with capsys.disabled():
        print()
        for (rule, d), groups in matrix.items():
            print(f"  {rule:9s} {d:30s} " + " ".join(f"{g if g in groups else '-':6s}" for g in GROUPS))
    assert matrix == CAUGHT_BY
    # the identity changes the number of emissions, and nothing else
    for rule in ("catalogue", "zonal"):
        assert any(k > 0 for k in counts[(rule, "run_cut_at_a_hole")]) and all(k >= 0 for k in counts[(rule, "run_cut_at_a_hole")])
    # every defect but the identity is caught somewhere
    assert all(groups for key, groups in matrix.items() if key[1] != "run_cut_at_a_hole")


def test_every_histogram_defect_is_caught_at_the_widths_listed(capsys):
    flat, n, x = lc.hist_table()
    rows, cols = lc.tables()["hist"][2][0]
    w = lc.row_weights(rows)
    matrix = {}
    for width in lc.HIST_WIDTHS:
        want = zm.histogram(flat.reshape(rows, cols), n, x.reshape(rows, cols), width - 2, 0.0, 1.0, w)
        for d in HIST_DEFECTS:
            got, _ = hist_records(flat, n, x, cols, w, width - 2, frozenset([d]))
            matrix.setdefault(d, set())
            if not np.array_equal(got, want):
                matrix[d].add(width)
    with capsys.disabled():
        print()
        for d, widths in matrix.items():
            print(f"  histogram {d:36s} " + " ".join(f"{v if v in widths else '-':>4}" for v in lc.HIST_WIDTHS))
    assert matrix == HIST_CAUGHT_AT
    # the second accumulator's columns are what the swap moves at width 128: without them it would be an identity there
    is_open, col = lc.hist_columns(x, 126)
    assert "second_accumulator_used" in lc.events_of(lc.classify_hist(flat, n, is_open, col, 128))


# ---- the closed forms of the rank tests
@pytest.mark.parametrize("wrap", [False, True])
@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("rows,cols", [(40, 70), (41, 71)])
def test_the_closed_forms_equal_the_model(rows, cols, conn, wrap):
    w = lc.row_weights(rows)
    mask = lc.isolated_mask(rows, cols, wrap, 7, target=300, band=4)
    labels, K, table = lc.isolated_answer(mask, w)
    even = lc.even_nodes(rows, cols, wrap)
    assert 100 < K < 600 and not mask[0:4].any() and np.array_equal(mask[4:8] != 0, even[4:8]) and not (mask != 0)[~even].any()
    got, n = model.label(mask, conn, wrap)
    assert n == K and np.array_equal(got, labels)
    assert first_difference(table, model.catalogue(labels, K, wrap, w)) is None
    assert first_difference(lc.isolated_answer(mask)[2], model.catalogue(labels, K, wrap)) is None
    labels, K, table = lc.stripes_answer(rows, cols, wrap, w)
    got, n = model.label(lc.stripes_mask(rows, cols), conn, wrap)
    assert n == K and np.array_equal(got, labels)
    assert first_difference(table, model.catalogue(labels, K, wrap, w)) is None
    assert first_difference(lc.stripes_answer(rows, cols, wrap)[2], model.catalogue(labels, K, wrap)) is None


def test_the_rank_lattices_split_as_the_scan_splits_them():
    chunks = [-(-r * c // lc.CHUNK) for r, c in lc.RANK_LATTICES]
    assert chunks == [256, 257, 1025]
    assert [lc.scan_split(k) for k in chunks] == [(1, 256, 0), (2, 129, 127), (5, 205, 51)]
    # the isolated sets keep K within 10^5 .. 3 x 10^5 and have chunks without a root and chunks with every root they can hold
    for rows, cols in lc.RANK_LATTICES:
        for wrap in (False, True):
            m = lc.isolated_mask(rows, cols, wrap, rows + wrap)
            K = int(m.sum())
            assert 100000 <= K <= 300000, (rows, cols, K)
            flat = np.concatenate([m.reshape(-1), np.zeros(-m.size % lc.CHUNK, np.uint8)]).reshape(-1, lc.CHUNK)
            full = lc.even_nodes(rows, cols, wrap).astype(np.uint8)
            most = np.concatenate([full.reshape(-1), np.zeros(-m.size % lc.CHUNK, np.uint8)]).reshape(-1, lc.CHUNK).sum(1)
            per = flat.sum(1)
            assert (per == 0).any() and ((per == most) & (most > 0)).any(), (rows, cols)
