"""The built tables of the contour kernels without a GPU (tests/contour_layout_cases.py): every named
edge is held by some table; a host simulator of the pipeline, written from the kernels block by block, gives the model's lines
(tests/contour_model.py) on every table, every field and vertex; the composer of the large table equals the model on a small
tiling; and every named defect, a switch on the simulator, changes the lines of exactly the tables listed in CATCHES, so a
kernel with that defect would fail tests/test_gpu_contour_layouts.py on them.  Where a defect cannot show, the identity that
says so is asserted.

The simulator keeps what the kernels keep: count's strided node order and per-wave sums, the binary search slot by slot over a
level table that is staged 256 slots a trip up to 4096 levels, the two one-block scans in passes with a carry, block_scan's
wave ladder and four per-wave sums, eight items in a row in base, heads_sum and heads_write, the expansion from base[], the
successor and predecessor rule with its checks, the int4 windows with their unsigned adds over two buffers and the parity of
the one that holds the result, tails, and vertices.  A slot that no thread wrote is UNWRITTEN; a simulation that reads one,
indexes outside a table or fails one of the kernels' or the driver's own checks raises Broken: on the device the call fails or
the bytes are anyone's, and either way the lines differ."""
import numpy as np
import pytest

import contour_layout_cases as lc
import contour_model as cm

UNWRITTEN = -(10 ** 15)
U32 = 0xFFFFFFFF
NORANK = -1

DEFECTS = ("scan_nodes_drops_the_carry", "scan_chunks_assigns_the_carry", "scan_chunks_drops_the_vertex_carry",
           "wave_offset_takes_k_le_w", "heads_run_cut_by_the_end_counted_full", "rank_with_lt_for_le", "search_upper_bound_one_short",
           "staging_stops_at_the_last_full_256", "seam_edge_left_out_of_the_count", "base_pair_swapped",
           "level_index_from_the_greater_rank", "rounds_one_short", "jump_tie_taken_by_the_farther_window",
           "jump_ignores_a_start_in_the_earlier_window", "tails_without_the_successor_that_is_the_head",
           "heads_write_without_the_vertex_offset", "fin_from_the_other_buffer")
CARRY_DEFECTS = DEFECTS[:3]


class Broken(Exception):
    """The kernels would have read a slot nobody wrote, left a table, or failed the call."""


# ---- the scans
def ladder(inc):
    """The shuffle ladder of a wave over axis 1: lane l adds lane l - d for d = 1, 2, 4, ..."""
    d = 1
    while d < inc.shape[1]:
        inc[:, d:] = inc[:, d:] + inc[:, :-d]
        d <<= 1
    return inc


def block_scan(v, defects):
    """(chunks, 256, k) per thread -> the exclusive scan over each block's threads and each block's total."""
    chunks, _, k = v.shape
    per = v.reshape(chunks * lc.WAVES, 64, k)
    inc = ladder(per.copy())
    sh = inc[:, 63].reshape(chunks, lc.WAVES, k)
    off = np.zeros((chunks, lc.WAVES, k), np.int64)
    for w in range(lc.WAVES):
        for j in range(lc.WAVES):
            if j <= w if "wave_offset_takes_k_le_w" in defects else j < w:
                off[:, w] += sh[:, j]
    return (off.reshape(chunks * lc.WAVES, 1, k) + inc - per).reshape(chunks, 256, k), sh.sum(1)


def scan_passes(sums, pass_len, drop_carry=False, assign_carry=False, drop_columns=()):
    """scan_nodes_kernel and scan_chunks_kernel: (n, k) chunk sums -> their exclusive prefix sums and the grand totals, in
    passes of pass_len chunks."""
    n, k = sums.shape
    out = np.empty_like(sums)
    wave = min(64, pass_len)
    carry = np.zeros(k, np.int64)
    for at in range(0, n, pass_len):
        m = min(pass_len, n - at)
        v = np.zeros((pass_len, k), np.int64)
        v[:m] = sums[at:at + m]
        per = v.reshape(-1, wave, k)
        inc = ladder(per.copy())
        sh = inc[:, -1]
        off = np.zeros(k, np.int64) if drop_carry else carry.copy()
        for c in drop_columns:
            off[c] = 0
        offs = off + np.cumsum(sh, axis=0) - sh
        out[at:at + m] = (offs[:, None, :] + inc - per).reshape(-1, k)[:m]
        carry = sh.sum(0) if assign_carry else carry + sh.sum(0)
    return out, carry


def eight_in_a_row(vals, repeat_the_last=False):
    """(n, k) per item -> (chunks, 256, 8, k): thread t of a chunk holds items 8 t .. 8 t + 7; an item past the end is nothing
    (or, under the defect, the run that the end cuts reads the last item again)."""
    n, k = vals.shape
    chunks = lc.n_chunks(n)
    pad = np.zeros((chunks * lc.CHUNK, k), np.int64)
    pad[:n] = vals
    if repeat_the_last:
        pad[n:-(-n // lc.RUN) * lc.RUN] = vals[n - 1]
    return pad.reshape(chunks, 256, lc.RUN, k)


# ---- the count
def ranks_of(z, levels, defects):
    """rank_of for every node: the binary search slot by slot, over the staged table."""
    n = len(levels)
    tab = np.asarray(levels, np.int64)
    staged = n
    if n <= lc.LDS_LEVELS and "staging_stops_at_the_last_full_256" in defects:
        staged = n // lc.STRIDE * lc.STRIDE
    valid = (z >= -lc.ZMAX) & (z <= lc.ZMAX)
    if (~valid & (z != lc.VOID)).any():
        raise Broken("heights outside the range: the call is refused")
    lo = np.zeros(len(z), np.int64)
    hi = np.full(len(z), n - 1 if "search_upper_bound_one_short" in defects else n, np.int64)
    while True:
        m = valid & (lo < hi)
        if not m.any():
            break
        mid = (lo + hi) >> 1
        if (mid[m] >= staged).any():
            raise Broken("a level slot nobody staged")
        at = tab[np.minimum(mid, n - 1)]
        le = at < z if "rank_with_lt_for_le" in defects else at <= z
        lo = np.where(m & le, mid + 1, lo)
        hi = np.where(m & ~le, mid, hi)
    return np.where(valid, lo, NORANK)


def crossings(ra, rb):
    return np.where((ra == NORANK) | (rb == NORANK), 0, np.abs(ra - rb))


FFS = np.array([-1, 0, 1, 0, 2, 0, 1, 0, 3, 0, 1, 0, 2, 0, 1, 0])
POPC = np.array([0, 1, 1, 2, 1, 2, 2, 3, 1, 2, 2, 3, 2, 3, 3, 4])


def partner(T, ci, cj, s, l, entering):
    """partner() for every element at once: the compact index of the paired side's element, or -1."""
    rows, cols, wrap, rank, base, eid, B = T["rows"], T["cols"], T["wrap"], T["rank"], T["base"], T["eid"], T["B"]
    out = np.full(len(ci), -1, np.int64)
    ok = (ci >= 0) & (ci < rows - 1)
    neg = cj < 0
    if not wrap:
        ok &= ~neg
    cj = np.where(neg, cols - 1, cj)
    cj1 = cj + 1
    over = cj1 >= cols
    if not wrap:
        ok &= ~over
    cj1 = np.where(over, 0, cj1)
    at = np.flatnonzero(ok)
    v0, v1 = ci[at] * cols + cj[at], ci[at] * cols + cj1[at]
    v2, v3 = v1 + cols, v0 + cols
    r = np.stack([rank[v0], rank[v1], rank[v2], rank[v3]])
    full = (r != NORANK).all(0)
    at, v0, v1, v2, v3, r = at[full], v0[full], v1[full], v2[full], v3[full], r[:, full]
    s, l = s[at], l[at]
    ab = sum((l < r[k]).astype(np.int64) << k for k in range(4))
    rot = ((ab >> 1) | (ab << 3)) & 15
    ent, ext = ab & ~rot & 15, ~ab & rot & 15
    if not (((ent if entering else ext) >> s) & 1).all():
        raise Broken("never: the element does not cross its side the way it was said to")
    total = T["z"][v0] + T["z"][v1] + T["z"][v2] + T["z"][v3]
    centre = total >= 4 * T["levels"][np.minimum(l, len(T["levels"]) - 1)] - 2
    t = np.where(POPC[ent] == 2, np.where(centre == entering, (s + 1) & 3, (s + 3) & 3), FFS[ext if entering else ent])
    e = np.choose(t, [2 * v0, 2 * v1 + 1, 2 * v3, 2 * v0 + 1])
    lo = np.minimum(np.choose(t, [r[0], r[1], r[2], r[3]]), np.choose(t, [r[1], r[2], r[3], r[0]]))
    where = base[e] + (l - lo)
    if (l < lo).any() or (where >= B).any() or (where < 0).any() or (eid[where] != e).any():
        raise Broken("never: the partner is no crossed edge")
    out[at] = where
    return out


def simulate(z, levels, wrap, defects=frozenset(), pass_len=lc.PASS):
    """(lines, vertices) as the kernels and the driver leave them, or Broken."""
    defects = frozenset(defects)
    assert defects <= set(DEFECTS)
    rows, cols = z.shape
    N, L = rows * cols, len(levels)
    flat = np.asarray(z, np.int64).reshape(-1)
    lv = np.asarray(levels, np.int64)
    empty = np.zeros(0, cm.LINE), np.zeros(0, np.int32)
    # count_kernel: node e * 256 + t of the chunk; the three ranks are one function of the height
    rank = ranks_of(flat, lv, defects)
    east, south = lc.other_ends(rows, cols, wrap)
    east_counted = east
    if "seam_edge_left_out_of_the_count" in defects:
        east_counted = np.where(np.arange(N) % cols == cols - 1, -1, east)
    cnt = np.stack([crossings(rank, np.where(o >= 0, rank[np.maximum(o, 0)], NORANK)) for o in (east_counted, south)], axis=1)
    chunks = lc.n_chunks(N)
    pad = np.zeros((chunks * lc.CHUNK, 2), np.int64)
    pad[:N] = cnt
    per_thread = pad.reshape(chunks, lc.RUN, lc.STRIDE, 2).sum((1, 3))                   # (chunks, 256): the strided nodes
    node_sums = per_thread.reshape(chunks, lc.WAVES, 64).sum(2).sum(1)
    # scan_nodes_kernel
    node_offs, total = scan_passes(node_sums[:, None], pass_len, drop_carry="scan_nodes_drops_the_carry" in defects)
    B = int(total[0])
    if B >= 2 ** 31:
        raise Broken("the call is refused")
    if B == 0:
        return empty
    # base_kernel: eight nodes in a row
    runs = eight_in_a_row(cnt)                                                          # (chunks, 256, 8, 2)
    excl, _ = block_scan(runs.sum((2, 3))[:, :, None], defects)
    inner = runs.reshape(chunks, 256, 2 * lc.RUN)
    inner = np.cumsum(inner, axis=2) - inner
    base = (node_offs[:, 0][:, None, None] + excl + inner).reshape(-1, 2)[:N]
    if "base_pair_swapped" in defects:
        base = base[:, ::-1]
    base = np.ascontiguousarray(base).reshape(-1)
    # expand_kernel
    ends = np.concatenate([base[1:], [B]])
    if (base > ends).any() or (ends > B).any() or (ends - base > L).any() or base.min() < 0:
        raise Broken("never: the prefix sums ascend to B")
    n_el = ends - base
    eid = np.full(B, UNWRITTEN, np.int64)
    eid[np.repeat(base, n_el) + np.arange(int(n_el.sum())) - np.repeat(np.cumsum(n_el) - n_el, n_el)] = np.repeat(np.arange(2 * N), n_el)
    if eid.min() == UNWRITTEN:
        raise Broken("an element nobody wrote")
    # succ_kernel
    k = np.arange(B)
    v, d = eid >> 1, eid & 1
    i, j = v // cols, v % cols
    o = np.where(d == 0, east[v], south[v])
    ra, rb = rank[v], np.where(o >= 0, rank[np.maximum(o, 0)], NORANK)
    lo, hi = np.minimum(ra, rb), np.maximum(ra, rb)
    l = lo + (k - base[eid])
    if not ((crossings(ra, rb) != 0) & (k >= base[eid]) & (l < hi) & (l < L)).all():
        raise Broken("never: an element that is no crossing of its edge")
    own = l < ra
    T = dict(rows=rows, cols=cols, wrap=wrap, rank=rank, base=base, eid=eid, B=B, z=flat, levels=lv)
    ei = np.where(d == 0, np.where(own, i, i - 1), i)
    ej = np.where(d == 0, j, np.where(own, j - 1, j))
    es = np.where(d == 0, np.where(own, 0, 2), np.where(own, 1, 3))
    xi = np.where(d == 0, np.where(own, i - 1, i), i)
    xj = np.where(d == 0, j, np.where(own, j, j - 1))
    xs = np.where(d == 0, np.where(own, 2, 0), np.where(own, 3, 1))
    succ = partner(T, ei, ej, es, l, True)
    pred = partner(T, xi, xj, xs, l, False)
    # jump_kernel: windows (x, y, z, w), z and w unsigned
    rounds = lc.rounds_of(B)
    if "rounds_one_short" in defects:
        rounds = max(rounds - 1, 0)
    buf = [np.stack([pred, k, np.zeros(B, np.int64), np.ones(B, np.int64)]), np.full((4, B), UNWRITTEN, np.int64)]
    for r in range(rounds):
        a = buf[r & 1]
        if a.min() == UNWRITTEN:
            raise Broken("a window nobody wrote")
        out = a.copy()
        m = (a[0] >= 0) & (a[0] < B)
        b = a[:, np.where(m, a[0], 0)]
        take = b[1] <= a[1] if "jump_tie_taken_by_the_farther_window" in defects else b[1] < a[1]
        if "jump_ignores_a_start_in_the_earlier_window" not in defects:
            take = take | (b[0] < 0)
        take &= m
        out[1] = np.where(take, b[1], a[1])
        out[2] = np.where(take, (a[3] + b[2]) & U32, a[2])
        out[3] = np.where(m, (a[3] + b[3]) & U32, a[3])
        out[0] = np.where(m, b[0], a[0])
        buf[(r & 1) ^ 1] = out
    fin = buf[(rounds & 1) ^ (1 if "fin_from_the_other_buffer" in defects else 0)]
    if fin.min() == UNWRITTEN:
        raise Broken("a result nobody wrote")
    # tails_kernel
    fy, fz = fin[1], fin[2]
    if (fy < 0).any() or (fy >= B).any() or (fz >= B).any():
        raise Broken("never: a head or a distance outside the elements")
    hands = succ < 0
    if "tails_without_the_successor_that_is_the_head" not in defects:
        hands = hands | (succ == fy)
    length, tailat = np.full(B, UNWRITTEN, np.int64), np.full(B, UNWRITTEN, np.int64)
    length[fy[hands]], tailat[fy[hands]] = fz[hands] + 1, k[hands]
    # heads_sum_kernel, scan_chunks_kernel
    is_head = fy == k
    if (length[is_head] == UNWRITTEN).any():
        raise Broken("a head whose length nobody wrote")
    hv = np.stack([is_head.astype(np.int64), np.where(is_head, length, 0)], axis=1)
    hruns = eight_in_a_row(hv, "heads_run_cut_by_the_end_counted_full" in defects)
    excl, side_sums = block_scan(hruns.sum(2), defects)
    drop = (1,) if "scan_chunks_drops_the_vertex_carry" in defects else ()
    side_offs, totals = scan_passes(side_sums, pass_len, assign_carry="scan_chunks_assigns_the_carry" in defects, drop_columns=drop)
    n_lines, n_vertices = int(totals[0]), int(totals[1])
    if n_vertices != B:
        raise Broken("the driver: the lines' lengths do not add up to the elements")
    # heads_write_kernel
    offs = side_offs.copy()
    if "heads_write_without_the_vertex_offset" in defects:
        offs[:, 1] = 0
    at = (offs[:, None, None, :] + excl[:, :, None, :] + np.cumsum(hruns, axis=2) - hruns).reshape(-1, 2)[:B]
    h = np.flatnonzero(is_head)
    ed, ta = eid[h], tailat[h]
    if (at[h, 0] >= n_lines).any() or (ta == UNWRITTEN).any() or (ta >= B).any():
        raise Broken("never: more heads than were counted, or a head without a tail")
    hr = np.maximum(ra[h], rb[h]) if "level_index_from_the_greater_rank" in defects else np.minimum(ra[h], rb[h])
    hl = hr + (h - base[ed])
    if (hl >= L).any():
        raise Broken("never: a head at no level")
    lines = np.zeros(n_lines, cm.LINE)
    written = np.zeros(n_lines, bool)
    lineno = np.full(B, UNWRITTEN, np.int64)
    lines["first"][at[h, 0]], lines["n_vertices"][at[h, 0]] = at[h, 1], hv[h, 1]
    lines["level_index"][at[h, 0]], lines["level"][at[h, 0]] = hl, lv[hl]
    lines["head"][at[h, 0]], lines["tail"][at[h, 0]], lines["closed"][at[h, 0]] = ed, eid[ta], fin[0][h] >= 0
    written[at[h, 0]], lineno[h] = True, at[h, 0]
    if not written.all():
        raise Broken("a line nobody wrote")
    # vertices_kernel
    if (fin[1][fy] != fy).any() or (lineno[fy] == UNWRITTEN).any():
        raise Broken("never: an element whose head is no head")
    rec = lines[lineno[fy]]
    where = rec["first"].astype(np.int64) + fz
    if (fz >= rec["n_vertices"]).any() or (where >= B).any():
        raise Broken("never: an element further from its head than its line is long")
    vertices = np.full(n_vertices, UNWRITTEN, np.int64)
    vertices[where] = eid
    if vertices.min() == UNWRITTEN:
        raise Broken("a vertex nobody wrote")
    return lines, vertices.astype(np.int32)


def lines_or_none(*args, **kw):
    try:
        return simulate(*args, **kw)
    except Broken:
        return None


def same(got, want):
    return got is not None and got[0].shape == want[0].shape and got[1].shape == want[1].shape and \
        all((got[0][f] == want[0][f]).all() for f in cm.LINE.names) and bool((got[1] == want[1]).all())


NAMES = list(lc.tables())
SCALED_PASS = 4


def all_but(*names):
    assert set(names) <= set(NAMES), set(names) - set(NAMES)
    return [n for n in NAMES if n not in names]


def named(*prefixes):
    return [n for n in NAMES if n.startswith(prefixes)]


def changed_by(defect, pass_len=lc.PASS, names=None):
    out = []
    for name in names or NAMES:
        z, levels, wrap = lc.tables()[name]
        if not same(lines_or_none(z, levels, wrap, {defect}, pass_len), lc.traced(name)):
            out.append(name)
    return out


# ---- the tables are what they are built to be
def test_every_event_is_held_by_some_table():
    held = {e: [name for name in NAMES if e in lc.events(name)] for e in lc.EVENTS}
    assert not [e for e, where in held.items() if not where], held
    # the tables built for an edge hold it
    for e, name in (("B_is_0", "stripe_1x1"), ("rounds_0", "stripe_1x2"), ("rounds_0", "rows_2x1"),
                    ("node_chunk_without_a_crossing_between", "gap_row"), ("node_chunk_without_a_crossing_between", "gap_rows_9x683"),
                    ("nodes_wave_offset_after_empty_waves", "gap_row"), ("last_node_chunk_holds_one_node", "gap_row"),
                    ("seam_edge_reaches_back_across_a_chunk", "gap_row"), ("seam_edge_reaches_back_across_a_chunk", "stripe_1x4096_wrapped"),
                    ("south_neighbour_in_the_next_chunk", "random_3x683"), ("seam_edge_reaches_back_across_a_chunk", "random_3x683"),
                    ("nodes_wave_offset_after_full_waves", "stripe_1x4097"), ("heads_wave_offset_after_full_waves", "stripe_1x4098"),
                    ("every_element_is_a_head", "stripe_1x2050"), ("head_first_in_a_later_chunk", "stripe_1x2050"),
                    ("head_last_in_a_chunk", "stripe_1x2049"), ("node_with_more_than_a_chunk_of_elements", "steep_1x4"),
                    ("edge_spans_an_element_chunk_border", "steep_1x4"), ("edge_spans_an_element_chunk_border", "steep_2x2"),
                    ("line_across_element_chunks", "steep_2x2"), ("open_head_is_its_lines_highest_index", "cols_2049x2"),
                    ("head_in_a_later_chunk_than_the_rest_of_its_line", "cols_2049x2"),
                    ("head_in_a_later_chunk_than_the_rest_of_its_line", "cols_4097x2"),
                    ("window_passes_its_head_100_times", "cones_40x60"), ("levels_in_global_memory", "levels_4097"),
                    ("staging_ends_on_a_full_stride", "levels_4096"), ("staging_ends_in_a_partial_stride", "levels_4095"),
                    ("one_open_line_of_2_pow_r_exactly_is_all_of_B", "rows_2x2048"), ("one_closed_line_of_2_pow_r_exactly_is_all_of_B", "rows_2x2048_wrapped"),
                    ("one_open_line_of_2_pow_r_plus_1_is_all_of_B", "rows_2x4097"), ("one_closed_line_of_2_pow_r_plus_1_is_all_of_B", "rows_2x65_wrapped"),
                    ("one_open_line_of_2_pow_r_minus_1_is_all_of_B", "rows_2x511"), ("one_closed_line_of_2_pow_r_minus_1_is_all_of_B", "rows_2x4095_wrapped")):
        assert e in lc.events(name), (e, name)
    # the head of the two-column lattice is at its far end one way and at its near end the other
    assert "open_head_is_its_lines_highest_index" not in lc.events("cols_2049x2_swapped")
    for n in lc.L_SIZES:                                    # every level count meets every height beside its first and last level
        here = set().union(*(lc.events(name) for name in named(f"levels_{n}")))
        assert {e for e in lc.LEVEL_EVENTS if e.startswith("height_")} | {"void_node"} | ({"level_gap_of_1"} if n > 1 else set()) <= here, n


def test_the_sizes_the_issue_names():
    t = {name: lc.layout(name) for name in NAMES}
    assert {t[f"stripe_1x{n}"]["N"] for n in lc.N_SIZES} == set(lc.N_SIZES)
    assert t["random_3x683"]["N"] == 2049 and t["random_7x585_voids"]["N"] == 4095 and t["random_5x820_voids_wrapped"]["N"] == 4100
    for b in lc.B_SIZES:
        S = t[f"stripe_1x{b + 1}"]
        assert S["B"] == S["n_lines"] == b and not S["closed"].any(), b          # dense heads: every element a line of one vertex
        S = t[f"rows_2x{b}"]
        assert S["B"] == b and S["length"].tolist() == [b] and S["closed"].tolist() == [False], b
        if b >= 3:
            S = t[f"rows_2x{b}_wrapped"]
            assert S["B"] == b and S["length"].tolist() == [b] and S["closed"].tolist() == [True], b
    assert "rows_2x1_wrapped" not in t and "rows_2x2_wrapped" not in t            # a wrapped lattice needs three columns
    assert {t[n]["rounds"] & 1 for n in named("rows_2x")} == {0, 1} and t["rows_2x1"]["rounds"] == 0
    for b in (9, 2049, 4097):
        far, near = t[f"cols_{b}x2"], t[f"cols_{b}x2_swapped"]
        assert far["heads"].tolist() == [b - 1] and near["heads"].tolist() == [0] and far["length"].tolist() == near["length"].tolist() == [b]
    S = t["cones_40x60"]
    assert 2 ** 11 <= S["B"] <= 2 ** 12 and S["closed"].sum() >= 96 and int(S["length"][S["closed"]].max()) <= 16
    for name in ("steep_1x4", "steep_2x2"):
        assert t[name]["n_levels"] == 2100 >= 2049 and int(t[name]["cnt"].max()) == 2100 and (t[name]["cnt"] != 0).sum() <= 2
    assert t["steep_2x2"]["length"].tolist() == [2] * 2100
    for n in lc.L_SIZES:
        for name in named(f"levels_{n}"):
            z, lv, _ = lc.tables()[name]
            assert len(lv) == n and (np.diff(lv.astype(np.int64)) >= 1).all() and (n < 3 or len(set(np.diff(lv).tolist())) > 2), name
    # the model traces every table in well under a second: rows x cols x levels stays modest
    assert max(t[n]["N"] * t[n]["n_levels"] for n in NAMES) <= 3 * 65536


# ---- the simulator equals the model
@pytest.mark.parametrize("name", NAMES)
def test_the_simulator_equals_the_model(name):
    z, levels, wrap = lc.tables()[name]
    want = lc.traced(name)
    assert same(simulate(z, levels, wrap), want), name
    assert same(simulate(z, levels, wrap, pass_len=SCALED_PASS), want), (name, "passes of 4 chunks")


def test_identity_the_lds_and_the_global_search_agree():
    """No defect separates count_kernel<true> from count_kernel<false>: they run one search over two copies of one table.
    Asserted as an identity: the ranks of the heights beside the first and the last level, of both bounds and of every level
    itself are searchsorted's, at 4096 levels (LDS) and at 4097 (global), and the shorter table's ranks are the longer one's
    wherever the height lies below the last level."""
    lv = {n: lc.level_table(n).astype(np.int64) for n in (4096, 4097)}
    for n, tab in lv.items():
        z = np.concatenate([tab - 1, tab, tab + 1, [-lc.ZMAX, lc.ZMAX]])
        assert (ranks_of(z, tab, frozenset()) == np.searchsorted(tab, z, side="right")).all(), n
    short = lc.level_table(4097)[:4096].astype(np.int64)
    z = np.arange(short[0] - 2, short[-1] + 3)
    assert (ranks_of(z, short, frozenset()) == np.minimum(ranks_of(z, lc.level_table(4097).astype(np.int64), frozenset()), 4096)).all()


# ---- the composer equals the model
def test_the_composer_equals_the_model_on_a_small_tiling():
    kinds = lc.kinds_of(lc.SMALL_TILING)
    assert set(kinds.reshape(-1).tolist()) == {lc.CLOSED, lc.WITH_VOID, lc.ZERO}
    z = lc.large_z(lc.SMALL_TILING)
    assert z.shape == (3 * lc.P_ROWS, 4 * lc.P_COLS)
    got = lc.compose(lc.SMALL_TILING)
    for wrap in (False, True):                              # the seam cells are all zero: the same lines
        assert same(got, cm.trace(z, lc.LARGE_LEVELS, wrap)), wrap
    assert same(got, lc.traced("small_tiling"))
    c, S = lc.large_counts(lc.SMALL_TILING), lc.layout("small_tiling")
    assert (c["nodes"], c["B"], c["lines"], c["open_lines"]) == (S["N"], S["B"], S["n_lines"], int((~S["closed"]).sum()))


def test_the_simulator_equals_the_composer_in_scaled_passes():
    """With passes of 4 chunks the small tiling's 7 chunks of nodes take two passes and its 14 chunks of elements four, as the
    large table's 2103 and 4731 take three and five passes of 1024."""
    z = lc.large_z(lc.SMALL_TILING)
    assert lc.n_chunks(z.size) == 7 and lc.n_chunks(lc.large_counts(lc.SMALL_TILING)["B"]) == 14
    for wrap in (False, True):
        assert same(simulate(z, lc.LARGE_LEVELS, wrap, pass_len=SCALED_PASS), lc.compose(lc.SMALL_TILING)), wrap


TWO_PASS_TILING = (45, 46)


def test_the_simulator_equals_the_composer_in_two_passes_of_1024():
    """45 x 46 copies, the least tiling of this shape whose nodes need a second pass of 1024 chunks: 1047 chunks of nodes, 2351 of
    elements (three passes), 23 rounds.  The slowest test of this file, about 15 s of numpy."""
    c = lc.large_counts(TWO_PASS_TILING)
    assert lc.PASS < c["node_chunks"] < 1.05 * lc.PASS and 2 * lc.PASS < c["element_chunks"] and c["rounds"] == 23
    assert same(simulate(lc.large_z(TWO_PASS_TILING), lc.LARGE_LEVELS, False), lc.compose(TWO_PASS_TILING))


def test_the_large_table_sees_the_carry_defects_in_passes_of_1024():
    """The large table's own chunk sums, the nodes' from numpy's counts and the heads' from the composed lines, through the two
    scans with the kernels' pass length: each carry defect moves offsets that a kernel then indexes with."""
    z = lc.large_z(lc.LARGE_TILING)
    _, cnt, lo = lc.counts_of(z, lc.LARGE_LEVELS, False)
    starts = np.arange(0, z.size, lc.CHUNK)
    node_sums = np.add.reduceat(cnt.reshape(-1, 2).sum(1), starts)[:, None]
    right = scan_passes(node_sums, lc.PASS)
    assert (right[0][:, 0] == np.cumsum(node_sums[:, 0]) - node_sums[:, 0]).all()
    dropped = scan_passes(node_sums, lc.PASS, drop_carry=True)
    assert (dropped[0][:lc.PASS] == right[0][:lc.PASS]).all() and (dropped[0][lc.PASS:] != right[0][lc.PASS:]).all()
    lines, vertices = lc.compose(lc.LARGE_TILING)
    head = lines["head"].astype(np.int64)
    at = (np.cumsum(cnt) - cnt)[head] + lines["level_index"] - lo[head]            # the heads' compact indices
    B = len(vertices)
    side_sums = np.zeros((lc.n_chunks(B), 2), np.int64)
    np.add.at(side_sums, at // lc.CHUNK, np.stack([np.ones(len(at), np.int64), lines["n_vertices"].astype(np.int64)], axis=1))
    right = scan_passes(side_sums, lc.PASS)
    assert right[1].tolist() == [len(lines), B] and len(side_sums) > 2 * lc.PASS
    assigned = scan_passes(side_sums, lc.PASS, assign_carry=True)
    assert (assigned[0][:2 * lc.PASS] == right[0][:2 * lc.PASS]).all() and (assigned[0][2 * lc.PASS:] != right[0][2 * lc.PASS:]).all()
    assert assigned[1][1] != B                              # the driver's check of the vertex total refuses the call
    half = scan_passes(side_sums, lc.PASS, drop_columns=(1,))
    assert (half[0][:, 0] == right[0][:, 0]).all() and (half[0][lc.PASS:, 1] != right[0][lc.PASS:, 1]).all() and (half[1] == right[1]).all()


def test_the_large_table_is_what_the_issue_asks_for():
    """The chosen numbers: patches of 23 x 45 nodes, 250 closed lines of 2528 elements, and 270 lines of 2435 elements of which
    23 open at the void block; 64 x 65 copies."""
    closed, void = lc.patch_lines(lc.CLOSED)[0], lc.patch_lines(lc.WITH_VOID)[0]
    assert (len(closed), int(closed["n_vertices"].sum()), int((closed["closed"] == 0).sum())) == (250, 2528, 0)
    assert (len(void), int(void["n_vertices"].sum()), int((void["closed"] == 0).sum())) == (270, 2435, 23)
    assert len(lc.patch_lines(lc.ZERO)[0]) == 0
    for kind in (lc.CLOSED, lc.WITH_VOID, lc.ZERO):         # the border of zeros
        p = lc.patch(kind)
        assert not p[0].any() and not p[-1].any() and not p[:, 0].any() and not p[:, -1].any()
    c = lc.large_counts(lc.LARGE_TILING)
    assert c == dict(nodes=4305600, B=9688407, lines=987920, open_lines=23483, node_chunks=2103, element_chunks=4731, rounds=24)
    assert c["node_chunks"] > 2 * lc.PASS and c["element_chunks"] > 2 * lc.PASS
    # one band of copies is all zero: a run of whole chunks of nodes without a crossing, between chunks that hold some
    z = lc.large_z(lc.LARGE_TILING)
    assert z.shape == (1472, 2925) and not z[lc.ZERO_BAND * lc.P_ROWS:(lc.ZERO_BAND + 1) * lc.P_ROWS].any()
    _, cnt, _ = lc.counts_of(z, lc.LARGE_LEVELS, False)
    assert int(cnt.sum()) == c["B"]
    per_chunk = np.add.reduceat(cnt.reshape(-1, 2).sum(1), np.arange(0, z.size, lc.CHUNK))
    some = np.flatnonzero(per_chunk)
    run = best = 0
    for empty in (per_chunk[some[0]:some[-1]] == 0).tolist():
        run = run + 1 if empty else 0
        best = max(best, run)
    assert best >= 31
    assert (lc.counts_of(z, lc.LARGE_LEVELS, True)[1] == cnt).all()          # the seam edges are not crossed


# ---- the named defects
# Which tables see which defect; every table not listed is blind to it.  The carry defects are listed for passes of 4 chunks
# (SCALED_PASS): with the kernels' 1024 no small table takes a second pass, and the large table alone sees them.
ROWS, COLS = named("rows_2x"), named("cols_")
ROWS_WRAPPED = [n for n in ROWS if n.endswith("_wrapped")]
MIXED = ["random_3x683", "random_7x585_voids", "random_5x820_voids_wrapped", "gap_rows_9x683", "cones_40x60"]
MANY_LEVELS = ["levels_4095", "levels_4096", "levels_4097", "levels_65536_bounds"]

CATCHES = {
    "scan_nodes_drops_the_carry": ["rows_2x4097", "rows_2x4097_wrapped", "cols_4097x2", "cols_4097x2_swapped", "small_tiling"],
    "scan_chunks_assigns_the_carry": MANY_LEVELS + ["small_tiling"],
    "scan_chunks_drops_the_vertex_carry": MANY_LEVELS + ["small_tiling"],
    "wave_offset_takes_k_le_w": all_but("stripe_1x1"),
    "heads_run_cut_by_the_end_counted_full": [f"stripe_1x{c}" for c in (2, 3, 4, 5, 6, 7, 8, 64, 66, 255, 256, 258, 511, 512, 514, 2047,
                                                                        2048, 2050, 4096, 4098)] + [
        "rows_2x1", "rows_2x2", "rows_2x4", "cols_9x2", "cols_2049x2", "cols_4097x2", "random_5x820_voids_wrapped", "steep_1x4",
        "levels_1", "levels_255", "levels_257", "levels_4095", "levels_4097", "levels_65536_first", "levels_65536_last"],
    "rank_with_lt_for_le": MIXED + ["steep_1x4", "steep_2x2"] + named("levels_")[:-1] + ["small_tiling"],
    "search_upper_bound_one_short": all_but("stripe_1x1", "levels_65536_first"),
    "staging_stops_at_the_last_full_256": all_but("levels_256", "levels_4096", "levels_4097", "levels_65536_first", "levels_65536_last",
                                                  "levels_65536_bounds"),
    "seam_edge_left_out_of_the_count": ["stripe_1x8_wrapped", "stripe_1x512_wrapped", "stripe_1x2048_wrapped", "stripe_1x4096_wrapped",
                                        "random_3x683", "random_5x820_voids_wrapped", "gap_row", "levels_65536_first", "levels_65536_last"],
    "base_pair_swapped": all_but("stripe_1x1", "steep_2x2", *ROWS),
    "level_index_from_the_greater_rank": all_but("stripe_1x1"),
    "rounds_one_short": [n for n in ROWS if n != "rows_2x1"] + COLS,
    "jump_tie_taken_by_the_farther_window": [f"rows_2x{b}_wrapped" for b in (3, 5, 63, 65, 255, 257, 511, 513, 2047, 2049, 4095, 4097)] + MIXED + [
        "small_tiling"],
    "jump_ignores_a_start_in_the_earlier_window": [f"rows_2x{b}" for b in (2, 4, 64, 256, 512, 2048, 4096)] + [
        "cols_9x2", "cols_2049x2", "cols_4097x2"] + MIXED + ["small_tiling"],
    "tails_without_the_successor_that_is_the_head": ROWS_WRAPPED + MIXED + ["small_tiling"],
    "heads_write_without_the_vertex_offset": ["stripe_1x2050", "stripe_1x4096", "stripe_1x4097", "stripe_1x4098", "stripe_1x4096_wrapped",
                                              "random_3x683", "random_7x585_voids", "random_5x820_voids_wrapped", "gap_row",
                                              "gap_rows_9x683", "cones_40x60", "steep_1x4", "steep_2x2"] + MANY_LEVELS + ["small_tiling"],
    "fin_from_the_other_buffer": ["stripe_1x2"] + ROWS + COLS,
}


def tables_with(event):
    return [name for name in NAMES if event in lc.events(name)]


@pytest.mark.parametrize("defect", DEFECTS)
def test_the_tables_that_catch_a_defect(defect):
    """The matrix: each defect changes the lines of exactly the tables listed, and of at least one; every other table is blind
    to it."""
    assert CATCHES[defect] and set(CATCHES) == set(DEFECTS)
    assert changed_by(defect, SCALED_PASS if defect in CARRY_DEFECTS else lc.PASS) == CATCHES[defect]


@pytest.mark.parametrize("defect", CARRY_DEFECTS)
def test_identity_one_pass_has_no_carry(defect):
    """With the kernels' passes of 1024 chunks no small table takes a second pass, so none sees a carry defect: the large table
    alone does, and tests/test_gpu_contour_layouts.py asserts that both of its scans take more than two passes.  With passes of
    4 chunks the tables of more than 4 chunks of nodes see the first, and those with a head beyond element chunk 4 the others."""
    assert changed_by(defect, names=CATCHES[defect]) == []
    if defect == "scan_nodes_drops_the_carry":
        assert CATCHES[defect] == [n for n in NAMES if lc.n_chunks(lc.layout(n)["N"]) > SCALED_PASS]
    else:
        assert CATCHES[defect] == [n for n in NAMES if lc.layout(n)["B"] and lc.layout(n)["heads"].max() >= SCALED_PASS * lc.CHUNK]
    c = lc.large_counts(lc.LARGE_TILING)
    assert c["node_chunks"] > 2 * lc.PASS and c["element_chunks"] > 2 * lc.PASS


def test_what_the_carry_defects_lose():
    """Dropping the carry restarts the offsets in every pass after the first and keeps the total; assigning it keeps the second
    pass right and loses the third, so it takes more than two passes to show in the offsets; dropping one half loses that half
    alone."""
    sums = np.stack([np.arange(1, 12), 3 * np.arange(1, 12)], axis=1).astype(np.int64)
    right = scan_passes(sums, SCALED_PASS)
    assert (right[0] == np.cumsum(sums, axis=0) - sums).all() and (right[1] == sums.sum(0)).all()
    dropped = scan_passes(sums, SCALED_PASS, drop_carry=True)
    assert (dropped[1] == right[1]).all() and (dropped[0][:4] == right[0][:4]).all() and (dropped[0][4:] != right[0][4:]).all()
    assigned = scan_passes(sums, SCALED_PASS, assign_carry=True)
    assert (assigned[0][:8] == right[0][:8]).all() and (assigned[0][8:] != right[0][8:]).all() and (assigned[1] != right[1]).all()
    half = scan_passes(sums, SCALED_PASS, drop_columns=(1,))
    assert (half[0][:, 0] == right[0][:, 0]).all() and (half[0][4:, 1] != right[0][4:, 1]).all() and (half[1] == right[1]).all()


def test_identities_of_the_scans():
    """block_scan's wave offset: a thread's offset gains its own wave's sum, so any crossing at all shows it.  The cut run: the
    items past the end read the last element again, which adds a head and its vertices to the totals exactly when the end cuts
    a run and the last element is a head; the driver's check of the vertex total then fails the call.  (In base_kernel the same
    slip changes nothing: a cut run is the block's last with nodes, and its surplus only moves the offsets of threads that have
    none.)  heads_write's vertex offset: it shows where heads lie in more than one chunk of elements (a line whose head
    alone lies in a later chunk, as on the two-column lattices, has nothing before it to offset)."""
    assert CATCHES["wave_offset_takes_k_le_w"] == [n for n in NAMES if lc.layout(n)["B"]]
    assert CATCHES["heads_run_cut_by_the_end_counted_full"] == [
        n for n in NAMES if "elements_run_cut_by_the_end" in lc.events(n) and "last_element_is_a_head" in lc.events(n)]
    assert CATCHES["heads_write_without_the_vertex_offset"] == [
        n for n in NAMES if lc.layout(n)["B"] and lc.layout(n)["heads"].max() // lc.CHUNK != lc.layout(n)["heads"].min() // lc.CHUNK]


def test_identities_of_the_count():
    """The staging loop that stops at the last full 256 leaves the slots after it unstaged, which every search over a table of
    no multiple of 256 levels reads; at a multiple of 256, and beyond 4096 levels where nothing is staged, it cannot show.  The
    seam edge shows wherever a level crosses one, a swapped pair wherever one crosses an east edge (its base then lies above its
    south edge's), the level index wherever there is a line.  A search whose upper bound is one short never finds the last
    level: it is blind only where no height reaches it."""
    assert CATCHES["staging_stops_at_the_last_full_256"] == [n for n in NAMES if "staging_ends_in_a_partial_stride" in lc.events(n)]
    seam, east = [], []
    for n in NAMES:
        z, levels, wrap = lc.tables()[n]
        S = lc.layout(n)
        per_node = S["cnt"].reshape(-1, 2)
        if wrap and per_node[S["cols"] - 1::S["cols"], 0].any():
            seam.append(n)
        if per_node[:, 0].any():
            east.append(n)
    assert CATCHES["seam_edge_left_out_of_the_count"] == seam and CATCHES["base_pair_swapped"] == east
    assert CATCHES["level_index_from_the_greater_rank"] == [n for n in NAMES if lc.layout(n)["B"]]
    reach = [n for n in NAMES if (lc.layout(n)["rank"] == lc.layout(n)["n_levels"]).any() and lc.layout(n)["B"]]
    assert CATCHES["search_upper_bound_one_short"] == reach
    at_a_level = [n for n in NAMES if np.isin(lc.tables()[n][0], lc.tables()[n][1]).any()]
    assert set(CATCHES["rank_with_lt_for_le"]) <= set(at_a_level)


def test_identities_of_the_rounds():
    """One round short: the windows are 2^(rounds - 1) long, enough for every line that is no longer.  The other buffer holds
    the round before, which is final under the same condition, and nothing at all when B = 1.  The tie: a window meets its
    line's least index twice only when it is longer than its closed line, so a closed line of exactly 2^rounds elements that is
    all of B is blind to it, and 2^rounds - 1 and 2^(rounds - 1) + 1 are not.  A start in the earlier window matters where it
    is not its line's least index; tails' second condition wherever a line closes."""
    long_lines = tables_with("line_longer_than_half_of_2_pow_rounds")
    assert CATCHES["rounds_one_short"] == long_lines
    assert CATCHES["fin_from_the_other_buffer"] == [n for n in NAMES if lc.layout(n)["B"] == 1 or n in long_lines]
    tie = []
    for n in NAMES:
        S = lc.layout(n)
        if S["closed"].any() and int(S["length"][S["closed"]].min()) < 1 << S["rounds"]:
            tie.append(n)
    assert CATCHES["jump_tie_taken_by_the_farther_window"] == tie
    exact = tables_with("one_closed_line_of_2_pow_r_exactly_is_all_of_B")
    assert exact and not set(exact) & set(tie)
    assert set(tables_with("one_closed_line_of_2_pow_r_minus_1_is_all_of_B") + tables_with("one_closed_line_of_2_pow_r_plus_1_is_all_of_B")) <= set(tie)
    assert CATCHES["jump_ignores_a_start_in_the_earlier_window"] == tables_with("start_is_not_its_lines_least_index")
    assert CATCHES["tails_without_the_successor_that_is_the_head"] == tables_with("closed_line")
