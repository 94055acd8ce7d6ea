"""The lane and chunk map of the contour kernels, lattices built for every edge of it, and a
classifier that says which edges a lattice holds.  A table is (z (rows, cols) int32, levels (n,) int32, wrap).

The map.  count_kernel takes a chunk of 2048 nodes per block and strides by 256: thread t of 256 takes nodes e * 256 + t of
the chunk, e = 0 .. 7, so that a wave's loads coalesce; its staging loop of the level table into LDS strides by 256 too, and
holds up to 4096 levels (count_kernel<true>), beyond which the searches read global memory (count_kernel<false>).  base_kernel
(nodes), heads_sum_kernel and heads_write_kernel (elements by compact index) take eight items in a row: thread t takes items
8 t .. 8 t + 7 of the chunk, a wave 512 items, and block_scan gives every thread the sum of the threads before it through four
per-wave sums.  scan_nodes_kernel (64-bit sums of the nodes' chunks) and scan_chunks_kernel (pairs of 32-bit sums, heads and
vertices, of the elements' chunks) are one block of 1024 each and turn the chunks' sums into prefix sums in passes of 1024
chunks with a carry from pass to pass.  expand_kernel takes one edge per thread, succ, jump, tails and vertices one element per
thread, 256 per block.  The pointer jumping runs rounds = ceil(log2 B) times over two buffers and leaves the result in
jump[rounds & 1]; B = 1 launches no round.

An element is one crossing (edge, level index); its compact index ascends with (edge, level index); edge 2 v + 0 joins node v
to its east neighbour (across the seam under wrap), edge 2 v + 1 to its south neighbour.

Sizes that cannot be built.  A wrapped lattice needs three columns, so the closed line of exactly B vertices on the wrapped
2 x B lattice exists from B = 3 on; B = 1 and 2 have the stripe and the open line only.  A 1 x 1 lattice (N = 1) has no edge:
it is the table with B = 0, which stops after the count.  Every other size the kernels' map names is here.

`tables()` holds the small tables, `layout` the ranks, counts, elements and lines of one (the counts from numpy's searchsorted,
the lines from tests/contour_model.py), `events` the named edges it holds.  The large table at the end is composed, not
traced."""
import functools

import numpy as np

import contour_model as cm

CHUNK, RUN, WAVE_ITEMS, WAVES, PASS, LDS_LEVELS, STRIDE = 2048, 8, 512, 4, 1024, 4096, 256
STRIDED = ("count_kernel", "count_kernel's staging loop")
EIGHT_IN_A_ROW = ("base_kernel", "heads_sum_kernel", "heads_write_kernel")
VOID, ZMAX = cm.VOID, 2 ** 30

N_SIZES = (1, 7, 8, 9, 255, 256, 257, 511, 512, 513, 2047, 2048, 2049, 4096, 4097)
B_SIZES = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 511, 512, 513, 2047, 2048, 2049, 4095, 4096, 4097)
L_SIZES = (1, 255, 256, 257, 4095, 4096, 4097, 65536)

SIZE_EVENTS = tuple(f"N_is_{n}" for n in N_SIZES) + tuple(f"B_is_{b}" for b in B_SIZES) + tuple(f"levels_{n}" for n in L_SIZES)
NODE_EVENTS = ("B_is_0", "nodes_run_cut_by_the_end", "nodes_wave_offset_after_empty_waves", "nodes_wave_offset_after_full_waves",
               "node_chunk_without_a_crossing_between", "south_neighbour_in_the_next_chunk", "seam_edge_reaches_back_across_a_chunk",
               "last_node_chunk_holds_one_node", "node_with_more_than_a_chunk_of_elements", "edge_spans_an_element_chunk_border")
HEAD_EVENTS = ("elements_run_cut_by_the_end", "heads_wave_offset_after_empty_waves", "heads_wave_offset_after_full_waves",
               "every_element_is_a_head", "head_first_in_a_later_chunk", "head_last_in_a_chunk", "last_element_is_a_head",
               "last_element_is_no_head", "open_head_is_its_lines_highest_index", "head_in_a_later_chunk_than_the_rest_of_its_line",
               "line_across_element_chunks", "open_line", "closed_line", "start_is_not_its_lines_least_index")
ROUND_EVENTS = ("rounds_0", "rounds_even", "rounds_odd") + tuple(
    f"one_{kind}_line_of_2_pow_r_{how}_is_all_of_B" for kind in ("open", "closed") for how in ("minus_1", "exactly", "plus_1")) + (
    "window_passes_its_head_100_times", "line_longer_than_half_of_2_pow_rounds")
LEVEL_EVENTS = tuple(f"height_{how}_the_{which}_level" for which in ("first", "last") for how in ("below", "at", "above")) + (
    "height_at_minus_2_pow_30", "height_at_2_pow_30", "void_node", "level_gap_of_1", "levels_irregular",
    "staging_ends_in_a_partial_stride", "staging_ends_on_a_full_stride", "levels_in_global_memory")
EVENTS = SIZE_EVENTS + NODE_EVENTS + HEAD_EVENTS + ROUND_EVENTS + LEVEL_EVENTS


def rounds_of(B):
    r = 0
    while (1 << r) < B:
        r += 1
    return r


def n_chunks(n):
    return -(-n // CHUNK)


# ---- the ranks, the counts and the elements of a table, by numpy
def other_ends(rows, cols, wrap):
    """(N,) the node at the other end of every node's east and south edge, or -1."""
    v = np.arange(rows * cols, dtype=np.int64)
    i, j = v // cols, v % cols
    east = np.where(j + 1 < cols, v + 1, v - j if wrap else -1)
    south = np.where(i + 1 < rows, v + cols, -1)
    return east, south


def counts_of(z, levels, wrap):
    """rank (N,) (-1: void), cnt (2 N,) the elements of every edge, lo (2 N,) the least level index that crosses it."""
    z = np.asarray(z, np.int64)
    rows, cols = z.shape
    flat = z.reshape(-1)
    rank = np.where(flat == VOID, -1, np.searchsorted(np.asarray(levels, np.int64), flat, side="right"))
    cnt, lo = np.zeros((rows * cols, 2), np.int64), np.zeros((rows * cols, 2), np.int64)
    for k, o in enumerate(other_ends(rows, cols, wrap)):
        ro = np.where(o >= 0, rank[np.maximum(o, 0)], -1)
        both = (rank >= 0) & (ro >= 0)
        cnt[:, k] = np.where(both, np.abs(rank - ro), 0)
        lo[:, k] = np.minimum(rank, ro)
    return rank, cnt.reshape(-1), lo.reshape(-1)


@functools.lru_cache(maxsize=None)
def traced(name):
    """The model's lines and vertices of a table, computed once."""
    z, levels, wrap = tables()[name]
    return cm.trace(z, levels, wrap)


@functools.lru_cache(maxsize=None)
def layout(name):
    z, levels, wrap = tables()[name]
    rows, cols = z.shape
    rank, cnt, lo = counts_of(z, levels, wrap)
    B = int(cnt.sum())
    base = np.cumsum(cnt) - cnt
    eid = np.repeat(np.arange(2 * rows * cols), cnt)
    lines, vertices = traced(name)
    assert len(vertices) == B, "numpy's count of the crossings is the model's"
    n = lines["n_vertices"].astype(np.int64)
    line_of = np.repeat(np.arange(len(lines)), n)
    pos = np.arange(B) - np.repeat(lines["first"].astype(np.int64), n)
    e = vertices.astype(np.int64)
    at = base[e] + lines["level_index"].astype(np.int64)[line_of] - lo[e]          # the compact index of every vertex
    assert B == 0 or (np.sort(at) == np.arange(B)).all()
    line, dist = np.empty(B, np.int64), np.empty(B, np.int64)
    line[at], dist[at] = line_of, pos
    heads = at[pos == 0] if B else np.zeros(0, np.int64)
    return dict(rows=rows, cols=cols, N=rows * cols, n_levels=len(levels), B=B, rounds=rounds_of(B), rank=rank, cnt=cnt, base=base,
                eid=eid, line=line, dist=dist, heads=heads, length=n, closed=lines["closed"].astype(bool), n_lines=len(lines))


def scan_events(values, what, ev):
    """The edges of block_scan's wave offsets over per-item values, eight in a row."""
    n = len(values)
    pad = np.zeros(n_chunks(n) * CHUNK, np.int64)
    pad[:n] = values
    waves = pad.reshape(-1, WAVES, WAVE_ITEMS)
    sums = waves.sum(2)
    full = (waves != 0).all(2)
    for w in range(1, WAVES):
        used = sums[:, w] != 0
        if (used & (sums[:, :w] == 0).all(1)).any():
            ev.add(what + "_wave_offset_after_empty_waves")
        if (used & full[:, :w].all(1)).any():
            ev.add(what + "_wave_offset_after_full_waves")
    return sums.sum(1)


@functools.lru_cache(maxsize=None)
def events(name):
    """The named edges that a table holds."""
    z, levels, wrap = tables()[name]
    S = layout(name)
    N, B, cols, rows, L = S["N"], S["B"], S["cols"], S["rows"], S["n_levels"]
    ev = set()
    if N in N_SIZES:
        ev.add(f"N_is_{N}")
    if B in B_SIZES:
        ev.add(f"B_is_{B}")
    if L in L_SIZES:
        ev.add(f"levels_{L}")
    # the levels and the heights
    flat, lv = z.reshape(-1).astype(np.int64), np.asarray(levels, np.int64)
    for which, c in (("first", lv[0]), ("last", lv[-1])):
        for how, h in (("below", c - 1), ("at", c), ("above", c + 1)):
            if (flat == h).any():
                ev.add(f"height_{how}_the_{which}_level")
    if (flat == -ZMAX).any():
        ev.add("height_at_minus_2_pow_30")
    if (flat == ZMAX).any():
        ev.add("height_at_2_pow_30")
    if (flat == VOID).any():
        ev.add("void_node")
    if L > 1 and (np.diff(lv) == 1).any():
        ev.add("level_gap_of_1")
    if L > 2 and len(set(np.diff(lv).tolist())) > 2:
        ev.add("levels_irregular")
    ev.add("levels_in_global_memory" if L > LDS_LEVELS else "staging_ends_in_a_partial_stride" if L % STRIDE else "staging_ends_on_a_full_stride")
    # the nodes
    per_node = S["cnt"].reshape(-1, 2)
    if N % RUN:
        ev.add("nodes_run_cut_by_the_end")
    if N % CHUNK == 1 and N > 1:
        ev.add("last_node_chunk_holds_one_node")
    chunk = scan_events(per_node.sum(1), "nodes", ev) != 0
    some = np.flatnonzero(chunk)
    if some.size and (~chunk[some[0]:some[-1]]).any():
        ev.add("node_chunk_without_a_crossing_between")
    v = np.arange(N)
    if (per_node[:, 1] != 0)[(v + cols) // CHUNK != v // CHUNK].any():
        ev.add("south_neighbour_in_the_next_chunk")
    seam = v[v % cols == cols - 1]
    if wrap and ((per_node[seam, 0] != 0) & ((seam - cols + 1) // CHUNK != seam // CHUNK)).any():
        ev.add("seam_edge_reaches_back_across_a_chunk")
    if (per_node.sum(1) > CHUNK).any():
        ev.add("node_with_more_than_a_chunk_of_elements")
    first, last = S["base"], S["base"] + S["cnt"] - 1
    if ((S["cnt"] > 1) & (first // CHUNK != last // CHUNK)).any():
        ev.add("edge_spans_an_element_chunk_border")
    if not B:
        ev.add("B_is_0")
        assert ev <= set(EVENTS), ev - set(EVENTS)
        return frozenset(ev)
    # the elements, the heads and the lines
    heads, line, length, closed = S["heads"], S["line"], S["length"], S["closed"]
    is_head = np.zeros(B, np.int64)
    is_head[heads] = 1
    if B % RUN:
        ev.add("elements_run_cut_by_the_end")
    scan_events(is_head, "heads", ev)
    if is_head.all():
        ev.add("every_element_is_a_head")
    if (heads[heads >= CHUNK] % CHUNK == 0).any():
        ev.add("head_first_in_a_later_chunk")
    if (heads % CHUNK == CHUNK - 1).any():
        ev.add("head_last_in_a_chunk")
    ev.add("last_element_is_a_head" if is_head[B - 1] else "last_element_is_no_head")
    ev.add("open_line" if not closed.all() else "closed_line")
    if closed.any():
        ev.add("closed_line")
    c = np.arange(B)
    order = np.lexsort((c, line))                               # the elements line by line, ascending inside each
    bounds = np.cumsum(length) - length
    least, most = c[order][bounds], c[order][bounds + length - 1]
    second = c[order][np.minimum(bounds + length - 2, B - 1)]
    long_open = ~closed & (length > 1)
    if (long_open & (heads == most)).any():
        ev.add("open_head_is_its_lines_highest_index")
    if (long_open & (heads == most) & (second // CHUNK < heads // CHUNK)).any():
        ev.add("head_in_a_later_chunk_than_the_rest_of_its_line")
    if (least // CHUNK != most // CHUNK).any():
        ev.add("line_across_element_chunks")
    if (~closed & (heads != least)).any():
        ev.add("start_is_not_its_lines_least_index")
    rounds = S["rounds"]
    ev.add("rounds_0" if rounds == 0 else "rounds_odd" if rounds & 1 else "rounds_even")
    if len(length) == 1 and B >= 3:
        kind = "closed" if closed[0] else "open"
        for how, d in (("minus_1", -1), ("exactly", 0), ("plus_1", 1)):
            if B - d >= 4 and (B - d) & (B - d - 1) == 0:
                ev.add(f"one_{kind}_line_of_2_pow_r_{how}_is_all_of_B")
    if closed.any() and 100 * int(length[closed].min()) <= 1 << rounds:
        ev.add("window_passes_its_head_100_times")
    if rounds and int(length.max()) > 1 << (rounds - 1):
        ev.add("line_longer_than_half_of_2_pow_rounds")
    assert ev <= set(EVENTS), ev - set(EVENTS)
    return frozenset(ev)


# ---- the tables
def level_table(n, seed=0):
    """n ascending levels from -1000 with seeded gaps of 1 .. 8, the first and the last gap 1: no arithmetic progression, and a
    height one beside the first or the last level is the next level where the table has one."""
    gaps = np.random.default_rng(1000 + n + seed).integers(1, 9, max(n - 1, 0))
    if n > 1:
        gaps[0] = gaps[-1] = 1
    if n > 4:
        gaps[n // 2] = 1
    return (-1000 + np.concatenate([[0], np.cumsum(gaps)])).astype(np.int32)


def _stripe(cols):
    """1 x cols of alternating heights under one level: no cell, so every crossed edge is a line of one vertex."""
    return (10 * (np.arange(cols) % 2)).astype(np.int32)[None, :]


def _two_rows(b, swapped=False):
    """2 x b, one row below and one above the level: one line of exactly b vertices, open, or closed under wrap."""
    z = np.zeros((2, b), np.int32)
    z[0 if swapped else 1] = 10
    return z


def _two_cols(b, swapped=False):
    z = np.zeros((b, 2), np.int32)
    z[:, 0 if swapped else 1] = 10
    return z


def _gap_row():
    """1 x 6145, wrapped: chunk 0 holds crossings in its third wave only, chunk 1 none, chunk 2 at every node, and the last
    chunk is one node, whose seam edge reaches back to node 0."""
    z = np.zeros(3 * CHUNK + 1, np.int32)
    z[2 * WAVE_ITEMS:3 * WAVE_ITEMS] = 10 * (np.arange(WAVE_ITEMS) % 2)
    z[2 * CHUNK:3 * CHUNK] = 10 * (np.arange(CHUNK) % 2)
    z[3 * CHUNK] = 10
    return z[None, :]


def _gap_rows():
    """9 x 683: rows 1 .. 6 flat, so the nodes 2048 .. 4095 have no crossed edge; stripes above and a random field below."""
    z = np.zeros((9, 683), np.int32)
    z[0] = 10 * (np.arange(683) % 2)
    z[7:] = np.random.default_rng(9).integers(0, 4, (2, 683)) * 5
    return z


def _random(rows, cols, seed, voids):
    rng = np.random.default_rng(seed)
    z = rng.integers(0, 4, (rows, cols)).astype(np.int32)
    if voids:
        z[rng.random((rows, cols)) < 0.04] = VOID
    return z


def _cones(down, across):
    d = np.abs(np.arange(5) - 2)
    return np.tile((4 - d[:, None] - d[None, :]).astype(np.int32), (down, across))


def _level_row(lv):
    c0, c1 = int(lv[0]), int(lv[-1])
    return np.array([[c0 - 1, c0, c0 + 1, c1 - 1, c1, c1 + 1, -ZMAX, ZMAX, VOID]], np.int32)


@functools.lru_cache(maxsize=None)
def tables():
    """{name: (z (rows, cols) int32, levels (n,) int32, wrap)}, read-only."""
    one = np.array([5], np.int32)
    out = {}
    for cols in sorted(set(N_SIZES) | {b + 1 for b in B_SIZES}):
        out[f"stripe_1x{cols}"] = (_stripe(cols), one, False)
    for cols in (8, 512, 2048, 4096):                           # even: the seam edge is crossed, B = N
        out[f"stripe_1x{cols}_wrapped"] = (_stripe(cols), one, True)
    for b in B_SIZES:
        out[f"rows_2x{b}"] = (_two_rows(b, b % 2 == 0), one, False)
        if b >= 3:
            out[f"rows_2x{b}_wrapped"] = (_two_rows(b, b % 2 == 1), one, True)
    for b in (9, 2049, 4097):
        out[f"cols_{b}x2"] = (_two_cols(b), one, False)
        out[f"cols_{b}x2_swapped"] = (_two_cols(b, True), one, False)
    out["random_3x683"] = (_random(3, 683, 683, False), np.array([1, 2, 3], np.int32), True)
    out["random_7x585_voids"] = (_random(7, 585, 585, True), np.array([1, 3], np.int32), False)
    out["random_5x820_voids_wrapped"] = (_random(5, 820, 820, True), np.array([2], np.int32), True)
    out["gap_row"] = (_gap_row(), one, True)
    out["gap_rows_9x683"] = (_gap_rows(), one, False)
    out["cones_40x60"] = (_cones(8, 12), np.array([2, 3, 4], np.int32), False)
    steep = level_table(2100, 7)
    lo, hi = int(steep[0]) - 1, int(steep[-1])
    out["steep_1x4"] = (np.array([[lo, lo, hi, hi]], np.int32), steep, False)
    out["steep_2x2"] = (np.array([[lo, lo], [hi, hi]], np.int32), steep, False)
    for n in L_SIZES:
        lv = level_table(n)
        if n <= LDS_LEVELS + 1:
            out[f"levels_{n}"] = (_level_row(lv), lv, False)
        else:                                                   # the model loops over the levels: three nodes a table
            row = _level_row(lv)[0]
            out[f"levels_{n}_first"] = (row[None, 0:3].copy(), lv, True)
            out[f"levels_{n}_last"] = (row[None, 3:6].copy(), lv, True)
            out[f"levels_{n}_bounds"] = (row[None, 6:9].copy(), lv, False)
    out["small_tiling"] = (large_z(SMALL_TILING), LARGE_LEVELS, False)
    for z, lv, _ in out.values():
        z.setflags(write=False)
        lv.setflags(write=False)
    return out


# ---- the large table: composed, not traced
P_ROWS, P_COLS = 23, 45
LARGE_LEVELS = np.array([1, 2, 3], np.int32)
LARGE_TILING = (64, 65)                                      # copies down and across: 1472 x 2925 = 4 305 600 nodes
SMALL_TILING = (3, 4)
ZERO_BAND = 30                                               # this row of copies of the large tiling is all zero
CLOSED, WITH_VOID, ZERO = 0, 1, 2


@functools.lru_cache(maxsize=None)
def patch(kind):
    """23 x 45 nodes: seeded heights 0 .. 4 inside a one-node border of 0, with a block of void nodes inside, or all zero."""
    z = np.zeros((P_ROWS, P_COLS), np.int32)
    if kind != ZERO:
        z[1:-1, 1:-1] = np.random.default_rng(2300 + kind).integers(0, 5, (P_ROWS - 2, P_COLS - 2))
    if kind == WITH_VOID:
        z[8:13, 18:27] = VOID
    z.setflags(write=False)
    return z


@functools.lru_cache(maxsize=None)
def kinds_of(tiling):
    """Which patch every copy is: a seeded pattern, every kind in the first row, one band of copies all zero."""
    down, across = tiling
    kinds = np.random.default_rng(down * 100 + across).choice([CLOSED, CLOSED, WITH_VOID, ZERO], size=tiling, p=[0.35, 0.35, 0.25, 0.05])
    kinds[0, :3] = (WITH_VOID, ZERO, CLOSED)
    if down > ZERO_BAND:
        kinds[ZERO_BAND] = ZERO
    kinds.setflags(write=False)
    return kinds


def large_z(tiling):
    down, across = tiling
    patches = np.stack([patch(k) for k in (CLOSED, WITH_VOID, ZERO)])
    return np.ascontiguousarray(patches[kinds_of(tiling)].transpose(0, 2, 1, 3).reshape(down * P_ROWS, across * P_COLS))


@functools.lru_cache(maxsize=None)
def patch_lines(kind):
    lines, vertices = cm.trace(patch(kind), LARGE_LEVELS, False)
    return lines, vertices


def compose(tiling):
    """The lines of large_z(tiling), wrapped or not: no cell between two copies is crossed, so they are the patches' lines moved
    to every copy (edge 2 v + k with v moved by the copy's offset), in the order of (head, level index); first is the running
    sum of n_vertices."""
    down, across = tiling
    cols = across * P_COLS
    kinds = kinds_of(tiling)

    def moved(e):
        """an edge of the patch on the tiling's lattice, in copy (0, 0)"""
        v, k = e.astype(np.int64) >> 1, e.astype(np.int64) & 1
        return 2 * ((v // P_COLS) * cols + v % P_COLS) + k

    recs, keys, shifts, src, pool, pool_at = [], [], [], [], [], 0
    for kind in (CLOSED, WITH_VOID):
        lines, vertices = patch_lines(kind)
        a, b = np.nonzero(kinds == kind)
        shift = 2 * (P_ROWS * a * cols + P_COLS * b)                            # (copies,)
        head = moved(lines["head"])[None, :] + shift[:, None]                   # (copies, lines)
        recs.append(np.tile(lines, len(a)))
        keys.append((head * 4 + lines["level_index"][None, :]).reshape(-1))
        shifts.append(np.repeat(shift, len(lines)))
        src.append(np.tile(lines["first"].astype(np.int64) + pool_at, len(a)))
        pool.append(moved(vertices))
        pool_at += len(vertices)
    rec, key, shift, src, pool = (np.concatenate(x) for x in (recs, keys, shifts, src, pool))
    order = np.argsort(key, kind="stable")
    out, shift, src = rec[order], shift[order], src[order]
    out["head"] = moved(out["head"]) + shift
    out["tail"] = moved(out["tail"]) + shift
    n = out["n_vertices"].astype(np.int64)
    first = np.cumsum(n) - n
    out["first"] = first
    take = np.repeat(src - first, n) + np.arange(int(n.sum()))
    return out, (pool[take] + np.repeat(shift, n)).astype(np.int32)


def large_counts(tiling):
    """dict(nodes, B, lines, open_lines, node_chunks, element_chunks, rounds) of the tiling, from the patches' traces."""
    kinds = kinds_of(tiling)
    B = n_lines = n_open = 0
    for kind in (CLOSED, WITH_VOID):
        lines, vertices = patch_lines(kind)
        copies = int((kinds == kind).sum())
        B += copies * len(vertices)
        n_lines += copies * len(lines)
        n_open += copies * int((lines["closed"] == 0).sum())
    nodes = tiling[0] * P_ROWS * tiling[1] * P_COLS
    return dict(nodes=nodes, B=B, lines=n_lines, open_lines=n_open, node_chunks=n_chunks(nodes), element_chunks=n_chunks(B),
                rounds=rounds_of(B))
