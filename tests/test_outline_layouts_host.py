"""The built tables of the outline kernels without a GPU (tests/outline_layout_cases.py): every named
edge is held by some table; a host simulator of the pipeline, written from the kernels block by block, gives the model's
outlines (tests/outline_model.py) on every table, every field and vertex; the composer of the large table equals the model on
a small tiling; and every named defect, a switch on the simulator, changes the outlines of the tables listed in CAUGHT_BY, so
a kernel with that defect would fail tests/test_gpu_outline_layouts.py on them.  Where a defect cannot show, the identity that
says so is asserted.

The simulator keeps what the kernels keep: chunks of 2048 items with eight in a row per thread, block_scan's wave ladder and
four per-wave sums, scan_chunks in passes with a carry, two jump buffers and the parity of the one that holds the result,
contract's chain elements and their hand-off, the heads scans, and sides_kernel wave by wave with its ballot loop.  A table
slot that no thread wrote is UNWRITTEN; a simulation that reads one, indexes outside a table or fails one of the kernels' own
checks raises Broken: on the device the call fails or the bytes are anyone's, and either way the outlines differ.  Window
totals stay Python-size integers; they wrap on the device only after a window has gone round its ring, when nothing reads
them."""
import numpy as np
import pytest

import outline_layout_cases as lc
import outline_model as om

UNWRITTEN = -(10 ** 15)
FIELDS = ("jump", "mn", "d", "sf", "sx", "tf", "tx", "tl")
CONFIGS = [(conn, mode, variant) for conn in (4, 8) for mode in (om.CORNERS, om.ALL) for variant in ("contract", "jump")]

DEFECTS = ("scan_chunks_forgets_the_carry", "carry_replaced_not_added", "wave_offset_takes_k_le_w", "last_partial_chunk_not_scanned",
           "rounds_floor_log2", "jump_takes_the_later_index_at_a_tie", "fin_from_the_wrong_buffer", "no_local_minimum_starts",
           "head_chain_without_the_ring_totals", "atomic_issued_by_lane_0", "left_clears_first_only", "shortcut_at_popc_above_2",
           "lanes_past_B_in_the_ballot")


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
    """(256, 2) per thread -> the exclusive scan over the block's threads and the block's total."""
    per = v.reshape(lc.WAVES, 64, 2)
    inc = ladder(per.copy())
    sh = inc[:, 63]
    off = np.zeros((lc.WAVES, 2), np.int64)
    for w in range(lc.WAVES):
        for k in range(lc.WAVES):
            if k <= w if "wave_offset_takes_k_le_w" in defects else k < w:
                off[w] += sh[k]
    return (off[:, None, :] + inc - per).reshape(256, 2), sh.sum(0)


def scan_chunks(sums, defects, pass_len):
    """The chunks' sums -> their exclusive prefix sums and the grand totals, in passes of pass_len chunks."""
    n = len(sums)
    out = sums.copy()
    wave = min(64, pass_len)
    carry = np.zeros(2, np.int64)
    for at in range(0, n, pass_len):
        m = min(pass_len, n - at)
        v = np.zeros((pass_len, 2), np.int64)
        v[:m] = sums[at:at + m]
        per = v.reshape(-1, wave, 2)
        inc = ladder(per.copy())
        sh = inc[:, -1]
        off = np.zeros(2, np.int64) if "scan_chunks_forgets_the_carry" in defects else carry.copy()
        offs = off + np.cumsum(sh, axis=0) - sh
        out[at:at + m] = (offs[:, None, :] + inc - per).reshape(-1, 2)[:m]
        carry = sh.sum(0) if "carry_replaced_not_added" in defects else carry + sh.sum(0)
    return out, carry


def chunked_scan(vals, defects, pass_len):
    """(n, 2) per item -> the exclusive prefix sum per item and the totals, as a sum kernel, scan_chunks and an index kernel
    leave them: a thread's eight items in a row, a run cut by the end adds nothing."""
    n = len(vals)
    chunks = lc.n_chunks(n)
    pad = np.zeros((chunks * lc.CHUNK, 2), np.int64)
    pad[:n] = vals
    runs = pad.reshape(chunks, 256, lc.RUN, 2)
    excl, sums = np.zeros((chunks, 256, 2), np.int64), np.zeros((chunks, 2), np.int64)
    for b in range(chunks):
        excl[b], sums[b] = block_scan(runs[b].sum(1), defects)
    scanned = n // lc.CHUNK if "last_partial_chunk_not_scanned" in defects else chunks
    offs = sums.copy()                                       # a chunk that is not scanned keeps its own sum
    offs[:scanned], totals = scan_chunks(sums[:scanned], defects, pass_len)
    inner = np.cumsum(runs, axis=2) - runs
    return (offs[:, None, None, :] + excl[:, :, None, :] + inner).reshape(-1, 2)[:n], totals


def pairs(a, b=None):
    return np.stack([np.asarray(a, np.int64), np.zeros(len(a), np.int64) if b is None else np.asarray(b, np.int64)], axis=1)


# ---- the pointer jumping
def new_buffer(B):
    return {f: np.full(B, UNWRITTEN, np.int64) for f in FIELDS}


def jump_round(src, dst, count, defects):
    if count > len(src["jump"]):
        raise Broken("more elements than sides")
    a = {f: src[f][:count] for f in FIELDS}
    if (a["jump"] == UNWRITTEN).any() or a["jump"].min() < 0 or a["jump"].max() >= len(src["jump"]):
        raise Broken("an element nobody wrote")
    b = {f: src[f][a["jump"]] for f in FIELDS}
    if (b["mn"] == UNWRITTEN).any():
        raise Broken("an element nobody wrote")
    take = b["mn"] <= a["mn"] if "jump_takes_the_later_index_at_a_tie" in defects else b["mn"] < a["mn"]
    dst["mn"][:count] = np.where(take, b["mn"], a["mn"])
    dst["d"][:count] = np.where(take, a["tl"] + b["d"], a["d"])
    dst["sf"][:count] = np.where(take, a["tf"] + b["sf"], a["sf"])
    dst["sx"][:count] = np.where(take, a["tx"] + b["sx"], a["sx"])
    for f in ("tf", "tx", "tl"):
        dst[f][:count] = a[f] + b[f]
    dst["jump"][:count] = b["jump"]


def walk_chain(c, nxt, flag, tx, jflag):
    tl = tf = sx = 0
    t = c
    for _ in range(4096):
        tl, tf, sx = tl + 1, tf + flag[t], sx + tx[t]
        n = nxt[t]
        if jflag[n]:
            return tl, tf, sx, n
        t = n
    raise Broken("a chain longer than a tile has sides")


def simulate(labels, n_regions, conn, wrap, mode, weights, variant, defects=frozenset(), pass_len=lc.PASS):
    """(rings, vertices) as the kernels leave them, or Broken."""
    defects = frozenset(defects)
    assert defects <= set(DEFECTS)
    S = lc.sides_of(labels, n_regions, conn, wrap)
    rows, cols, bits = S["rows"], S["cols"], S["bits"]
    contract = variant == "contract"
    # mark, scan_chunks, base
    popc = np.array([0, 1, 1, 2, 1, 2, 2, 3, 1, 2, 2, 3, 2, 3, 3, 4])
    base, totals = chunked_scan(pairs(popc[bits]), defects, pass_len)
    base, B = base[:, 0], int(totals[0])
    if B == 0:
        return np.zeros(0, om.RING), np.zeros((0, 2), np.int32)
    if B > 4 * rows * cols:
        raise Broken("more sides than the lattice has")
    # succ: every boundary side writes at its compact index
    v, k = S["sid"] >> 2, S["sid"] & 3
    c = base[v] + popc[bits[v] & ((1 << k) - 1)]
    s = base[S["sv"]] + popc[bits[S["sv"]] & ((1 << S["sk"]) - 1)]
    if max(c.max(), s.max()) >= B:
        raise Broken("a compact index past B")
    sid, nxt, flag, jflag = (np.full(B, UNWRITTEN, np.int64) for _ in range(4))
    sid[c], nxt[c] = S["sid"], s
    flag[s] = (mode == om.ALL) | S["turns"]
    jflag[s] = S["enters"] * 1 + (s < c) * 2
    if min(sid.min(), nxt.min(), flag.min(), jflag.min()) == UNWRITTEN:
        raise Broken("a side nobody wrote")
    tx = lc.TX[sid & 3]
    me = np.arange(B)
    rounds = lc.rounds_of(B)
    if "rounds_floor_log2" in defects:
        rounds = B.bit_length() - 1
    buf = [new_buffer(B), new_buffer(B)]
    if contract:
        starts = ((jflag & 1) != 0) | (((jflag & 2) != 0) & (me < nxt) & ("no_local_minimum_starts" not in defects))
        jidx, totals = chunked_scan(pairs(starts), defects, pass_len)
        jidx, count = np.where(starts, jidx[:, 0], UNWRITTEN), int(totals[0])
        if count == 0 or jidx.max() >= B:
            raise Broken("no chains, or a chain number past B")
        nl, fl, tl_, st = nxt.tolist(), flag.tolist(), tx.tolist(), starts.tolist()
        for c0 in np.flatnonzero(starts).tolist():                              # chain_init
            tl, tf, sx, end = walk_chain(c0, nl, fl, tl_, st)
            for f, val in zip(FIELDS, (jidx[end], c0, 0, 0, 0, tf, sx, tl)):
                buf[0][f][jidx[c0]] = val
        for r in range(rounds):
            jump_round(buf[r & 1], buf[(r & 1) ^ 1], count, defects)
        el, out = buf[rounds & 1], buf[(rounds & 1) ^ 1]
        for c0 in np.flatnonzero(starts).tolist():                              # chain_down
            e = {f: int(el[f][jidx[c0]]) for f in ("mn", "d", "sf", "sx")}
            if UNWRITTEN in e.values():
                raise Broken("an element nobody wrote")
            head = e["mn"] == c0
            d, sf, sx = e["d"], e["sf"], e["sx"]
            if head and "head_chain_without_the_ring_totals" not in defects:
                tl, tf, wx, end = walk_chain(c0, nl, fl, tl_, st)
                after = {f: int(el[f][jidx[end]]) for f in ("d", "sf", "sx")}
                d, sf, sx = after["d"] + tl, after["sf"] + tf, after["sx"] + wx
            t = c0
            for step in range(4096):
                first = head and step == 0
                out["mn"][t], out["d"][t], out["sf"][t], out["sx"][t] = e["mn"], 0 if first else d, 0 if first else sf, 0 if first else sx
                d, sf, sx = d - 1, sf - fl[t], sx - tl_[t]
                if st[nl[t]]:
                    break
                t = nl[t]
        fin_at = (rounds & 1) ^ 1
    else:
        for f, val in zip(FIELDS, (nxt, me, 0, 0, 0, flag, tx, 1)):            # jump_init
            buf[0][f][:] = val
        for r in range(rounds):
            jump_round(buf[r & 1], buf[(r & 1) ^ 1], B, defects)
        fin_at = rounds & 1
    fin = buf[fin_at ^ 1 if "fin_from_the_wrong_buffer" in defects else fin_at]
    mn, d, sf, sx = (fin[f] for f in ("mn", "d", "sf", "sx"))
    if min(mn.min(), d.min(), sf.min(), sx.min()) == UNWRITTEN:
        raise Broken("a result nobody wrote")
    # heads_sum, scan_chunks, heads_write
    is_head = mn == me
    tf = flag + sf[nxt]
    hv = pairs(is_head, np.where(is_head, np.where(tf != 0, tf, 1), 0))
    if hv[:, 1].min() < 0:
        raise Broken("a negative vertex count wraps to 2^32")
    at, totals = chunked_scan(hv, defects, pass_len)
    n_rings, n_vertices = int(totals[0]), int(totals[1])
    if 3 * n_rings > B or n_vertices > B:
        raise Broken("more rings or vertices than the dead buffer takes")
    rings = np.zeros(n_rings, om.RING)
    written = np.zeros(n_rings, bool)
    ringno = np.full(B, UNWRITTEN, np.int64)
    for c0 in np.flatnonzero(is_head).tolist():
        r = int(at[c0, 0])
        if r >= n_rings or 1 + d[nxt[c0]] < 0:
            raise Broken("a ring number past the table")
        x = tx[c0] + sx[nxt[c0]]
        v0 = int(sid[c0]) >> 2
        rings[r] = (0, 0, at[c0, 1], 1 + d[nxt[c0]], hv[c0, 1], labels[v0 // cols, v0 % cols], sid[c0],
                    abs(x) // cols * (1 if x >= 0 else -1), 0)
        written[r], ringno[c0] = True, r
    if not written.all():
        raise Broken("a ring nobody wrote")
    # sides_kernel: the checks and the vertices side by side, the sums wave by wave
    if mn.min() < 0 or mn.max() >= B or (mn[mn] != mn).any():
        raise Broken("a side whose head is no head")
    ring = ringno[mn]
    rec = rings[ring]
    nv, first, wind = rec["n_vertices"].astype(np.int64), rec["first"].astype(np.int64), rec["wind"].astype(np.int64)
    if (~is_head & ((sf < 0) | (sf > nv) | (d < 0) | (d >= rec["n_sides"]))).any():
        raise Broken("a side outside its ring")
    i = (sid >> 2) // cols
    kk = sid & 3
    cw = np.concatenate([[0], np.cumsum(np.ones(rows, np.int64) if weights is None else np.asarray(weights, np.int64))])
    a = np.where(kk == 0, -i, np.where(kk == 2, i + 1, 0))
    wa = np.where(kk == 0, -cw[i], np.where(kk == 2, cw[np.minimum(i + 1, rows)], 0))
    key = np.where((kk == 0) | (kk == 2), ring, -1)
    vertices = np.full((n_vertices, 2), UNWRITTEN, np.int64)
    writes = ((flag != 0) & (is_head | (sf > 0))) | (is_head & (flag == 0) & (sf[nxt] == 0))
    hs = rec["head"].astype(np.int64)
    x0 = (hs >> 2) % cols + (((hs & 3) == 1) | ((hs & 3) == 2))
    where = first + np.where(is_head, 0, nv - sf)
    if writes.any() and where[writes].max() >= n_vertices:
        raise Broken("a vertex past the table")
    vertices[where[writes], 0] = (i + (kk >= 2))[writes]
    vertices[where[writes], 1] = np.where(is_head, x0, x0 + wind * cols - sx)[writes]
    if n_vertices and vertices.min() == UNWRITTEN:
        raise Broken("a vertex nobody wrote")
    area, warea = [0] * n_rings, [0] * n_rings
    for w0 in range(0, B, lc.SIDE_WAVE):
        lanes = min(lc.SIDE_WAVE, B - w0)
        wk, wa_, ww = np.full(64, -1, np.int64), np.zeros(64, np.int64), np.zeros(64, np.int64)
        wk[:lanes], wa_[:lanes], ww[:lanes] = key[w0:w0 + lanes], a[w0:w0 + lanes], wa[w0:w0 + lanes]
        if "lanes_past_B_in_the_ballot" in defects:         # they repeat the last side
            wk[lanes:], wa_[lanes:], ww[lanes:] = wk[lanes - 1], wa_[lanes - 1], ww[lanes - 1]
        left = wk >= 0
        while left.any():
            lane = int(np.argmax(left))
            ring_k = int(wk[lane])
            mine = wk == ring_k
            sa, sw = np.where(mine, wa_, 0), np.where(mine, ww, 0)
            if mine.sum() > (2 if "shortcut_at_popc_above_2" in defects else 1):
                sa, sw = np.full(64, sa.sum()), np.full(64, sw.sum())             # the butterfly leaves the sum in every lane
            issuer = 0 if "atomic_issued_by_lane_0" in defects else lane
            if sa[issuer] or sw[issuer]:
                if ring_k < 0:
                    raise Broken("an atomic before the ring table")
                area[ring_k] += int(sa[issuer])
                warea[ring_k] += int(sw[issuer])
            wk[mine] = -1
            if "left_clears_first_only" in defects:
                left[lane] = False
            else:
                left &= ~mine
    rings["area"] = area
    rings["warea"] = area if weights is None else warea
    return rings, vertices.astype(np.int32)


def outlines_or_none(*args, **kw):
    try:
        return simulate(*args, **kw)
    except Broken:
        return None


def same(got, want):
    return got is not None and got[0].shape == want[0].shape and got[1].shape == want[1].shape and \
        all((got[0][f] == want[0][f]).all() for f in om.RING.names) and bool((got[1] == want[1]).all())


_TRACED = {}


def traced(name, conn, mode):
    """The model's outlines with row weights, computed once."""
    if (name, conn, mode) not in _TRACED:
        labels, n, wrap = lc.tables()[name]
        _TRACED[(name, conn, mode)] = om.trace(labels, conn, wrap, mode, lc.weights_for(labels.shape[0]))
    return _TRACED[(name, conn, mode)]


# ---- the tables are what they are built to be
# name: (B, rounds, rings at connectivity 4, rings at 8, chunks of nodes, chunks of sides)
LITERALS = {
    "alternating_1x2047": (8188, 13, 2047, 2047, 1, 4), "alternating_1x2048": (8192, 13, 2048, 2048, 1, 4),
    "alternating_1x2049": (8194, 14, 2048, 2048, 2, 5), "alternating_1x4095": (16378, 14, 4094, 4094, 2, 8),
    "alternating_1x4097": (16388, 15, 4097, 4097, 3, 9), "random_3x683": (2636, 12, 323, 220, 2, 2),
    "gap_row": (10244, 14, 2561, 2561, 4, 6), "rect_2046_sides": (2046, 11, 1, 1, 2, 1), "ring_2048": (2048, 11, 1, 1, 1, 1),
    "ring_2050": (2050, 12, 1, 1, 1, 2), "rect_4096_sides": (4096, 12, 1, 1, 4, 2), "rect_4098_sides": (4098, 13, 1, 1, 4, 3),
    "head_at_2047": (4098, 13, 2, 2, 2, 3), "head_at_2048": (4100, 13, 2, 2, 2, 3), "wrapped_1024": (2048, 11, 2, 2, 1, 1),
    "wrapped_1025": (2050, 12, 2, 2, 1, 2), "1x1": (4, 2, 1, 1, 1, 1), "1x3_wrapped": (6, 3, 2, 2, 1, 1),
    "long_beside_short": (2402, 12, 301, 301, 1, 2), "triples_41": (126, 7, 42, 42, 1, 1), "triples_43": (132, 8, 44, 44, 1, 1),
    "one_tile_rect": (12, 4, 1, 1, 1, 1), "serpentine": (1042, 11, 1, 1, 1, 1), "saddle_rows": (1056, 11, 16, 16, 1, 1),
    "comb_across": (168, 8, 1, 1, 2, 1), "band_60_cols": (120, 7, 2, 2, 1, 1), "band_70_cols": (140, 8, 2, 2, 1, 1),
    "random_15x63": (1118, 11, 108, 78, 1, 1), "random_16x64": (1172, 11, 110, 63, 1, 1), "random_17x65": (1264, 11, 106, 70, 1, 1),
    "random_31x127": (4448, 13, 364, 225, 2, 3), "random_32x128": (4586, 13, 381, 242, 2, 3),
    "random_33x129": (4776, 13, 394, 249, 3, 3), "small_tiling": (21296, 15, 5324, 4631, 7, 11),
}
NAMES = list(LITERALS)


def test_every_table_is_listed():
    assert set(NAMES) == set(lc.tables())


@pytest.mark.parametrize("name", NAMES)
def test_the_sizes_of_every_table(name):
    """B, the rounds, the ring counts and the chunk counts as literals: an edit of a table cannot quietly lose an edge."""
    B, rounds, rings4, rings8, node_chunks, side_chunks = LITERALS[name]
    for conn, rings in ((4, rings4), (8, rings8)):
        S = lc.layout(name, conn)
        assert (S["B"], S["rounds"], len(S["heads"]), lc.n_chunks(S["N"]), lc.n_chunks(S["B"])) == \
            (B, rounds, rings, node_chunks, side_chunks), (name, conn)
        want, _ = traced(name, conn, om.CORNERS)
        # the restated sides and successors give the model's rings: heads, lengths, windings
        assert (S["sid"][S["heads"]] == want["head"]).all() and (S["length"] == want["n_sides"]).all()


def test_the_sizes_the_issue_names():
    t = {name: lc.layout(name, 4) for name in NAMES}
    assert sorted({t[f"alternating_1x{c}"]["N"] for c in (2047, 2048, 2049, 4095, 4097)}) == [2047, 2048, 2049, 4095, 4097]
    assert t["random_3x683"]["N"] == 2049 and t["alternating_1x2049"]["N"] % 8 == 1 and t["alternating_1x4097"]["N"] % 8 == 1
    assert {t[n]["B"] for n in ("rect_2046_sides", "ring_2048", "ring_2050", "rect_4096_sides", "rect_4098_sides")} == \
        {2046, 2048, 2050, 4096, 4098}
    assert t["ring_2048"]["length"].tolist() == [2048] and t["ring_2050"]["length"].tolist() == [2050]
    assert t["wrapped_1024"]["length"].tolist() == [1024, 1024] and t["wrapped_1025"]["length"].tolist() == [1025, 1025]
    assert t["long_beside_short"]["length"].tolist() == [1202] + [4] * 300
    assert t["serpentine"]["length"].tolist() == [1042] and int((lc.tables()["serpentine"][0] >= 0).sum()) == 520
    assert t["head_at_2047"]["heads"].tolist() == [0, 2047] and t["head_at_2048"]["heads"].tolist() == [0, 2048]
    for name in lc.DEAD_BUFFER:
        assert set(t[name]["length"].tolist()) == {3} and 48 * len(t[name]["heads"]) + 8 * t[name]["B"] == 24 * t[name]["B"]
    assert {t[name]["rounds"] & 1 for name in lc.DEAD_BUFFER} == {0, 1}


def test_every_event_is_held_by_some_table():
    held = {e: [(name, conn) for name in NAMES for conn in (4, 8) if e in lc.events(name, conn)] for e in lc.EVENTS}
    assert not [e for e, where in held.items() if not where], held
    # the tables built for an edge hold it
    for e, name in (("empty_chunk_between", "gap_row"), ("wave_offset_after_empty_waves", "gap_row"),
                    ("last_chunk_holds_one_item", "gap_row"), ("wave_offset_after_full_waves", "alternating_1x4097"),
                    ("head_last_in_a_chunk", "head_at_2047"), ("head_first_in_a_later_chunk", "head_at_2048"),
                    ("ring_of_2_pow_rounds_sides", "ring_2048"), ("ring_of_2_pow_k_plus_2_sides", "ring_2050"),
                    ("ring_of_odd_length", "wrapped_1025"), ("window_passes_its_head_twice", "long_beside_short"),
                    ("dead_buffer_as_full_as_it_gets", "triples_41"), ("dead_buffer_as_full_as_it_gets", "triples_43"),
                    ("ring_in_one_tile_started_by_its_head_alone", "band_60_cols"),
                    ("ring_in_one_tile_started_by_its_head_alone", "alternating_1x2048"), ("chain_of_128_sides", "serpentine"),
                    ("head_chain_followed_by_2_chains", "serpentine"), ("head_is_entry_and_minimum", "wrapped_1024"),
                    ("ring_enters_one_tile_4_times", "comb_across"), ("winding_ring_inside_one_tile", "band_60_cols"),
                    ("ring_fills_whole_waves", "ring_2048"), ("sixteen_rings_of_two_keys_in_a_wave", "alternating_1x2048"),
                    ("one_keyed_side_not_at_lane_0", "long_beside_short"), ("partial_sum_is_zero", "wrapped_1024"),
                    ("B_mod_64_is_2", "ring_2050"), ("B_mod_64_is_62", "rect_2046_sides")):
        assert e in lc.events(name, 4), (e, name)
    # the parity of the rounds under both variants: every table runs under both, so one table of each parity is enough
    assert held["rounds_even"] and held["rounds_odd"]
    assert "winding_ring_inside_one_tile" not in lc.events("band_70_cols", 4)      # there the seam is a tile border


# ---- the simulator equals the model
@pytest.mark.parametrize("name", NAMES)
def test_the_simulator_equals_the_model(name):
    labels, n, wrap = lc.tables()[name]
    w = lc.weights_for(labels.shape[0])
    for conn, mode, variant in CONFIGS:
        want = traced(name, conn, mode)
        assert same(simulate(labels, n, conn, wrap, mode, w, variant), want), (name, conn, mode, variant)
    plain = want[0].copy()
    plain["warea"] = plain["area"]
    assert same(simulate(labels, n, conn, wrap, mode, None, variant), (plain, want[1])), (name, "no weights")
    if name in lc.DEAD_BUFFER or name == "long_beside_short":
        assert int(np.abs(want[0]["warea"]).max()) > 2 ** 32


# ---- the composer equals the model
@pytest.mark.parametrize("conn", [4, 8])
def test_the_composer_equals_the_model_on_a_small_tiling(conn):
    labels = lc.large_labels(lc.SMALL_TILING)
    assert labels.shape == (3 * lc.P_ROWS, 4 * lc.P_COLS)
    for mode in (om.CORNERS, om.ALL):
        for weight in (None, lc.LARGE_WEIGHT):
            w = None if weight is None else np.full(labels.shape[0], weight, np.uint32)
            assert same(lc.compose(lc.SMALL_TILING, conn, mode, weight), om.trace(labels, conn, False, mode, w)), (conn, mode, weight)
    nodes, B, rings = lc.large_counts(lc.SMALL_TILING, conn)
    S = lc.layout("small_tiling", conn)
    assert (nodes, B, rings) == (S["N"], S["B"], len(S["heads"]))


def test_the_large_table_is_what_the_issue_asks_for():
    """The chosen numbers: a 23 x 45 pattern of 484 nodes and 1936 sides (484 rings at connectivity 4, 421 at 8) tiled 48 x 47
    with 50 copies blanked, one whole row of copies among them."""
    r4, r8 = lc.pattern_outlines(4, om.CORNERS)[0], lc.pattern_outlines(8, om.CORNERS)[0]
    assert (len(r4), len(r8), int(r4["n_sides"].sum()), int(r8["n_sides"].sum())) == (484, 421, 1936, 1936)
    nodes, B, rings = lc.large_counts(lc.LARGE_TILING, 4)
    assert (nodes, B, rings) == (1104 * 2115, 1936 * 2206, 484 * 2206) == (2334960, 4270816, 1067704)
    assert lc.large_counts(lc.LARGE_TILING, 8)[2] == 421 * 2206
    # more than one pass of scan_chunks over the nodes, more than two over the sides, and 23 rounds
    assert lc.n_chunks(nodes) == 1141 > lc.PASS and lc.n_chunks(B) == 2086 > 2 * lc.PASS and lc.rounds_of(B) == 23
    # the blanked row of copies leaves whole chunks of nodes without a side
    labels = lc.large_labels(lc.LARGE_TILING)
    per_chunk = np.add.reduceat((labels.reshape(-1) >= 0).astype(np.int64), np.arange(0, labels.size, lc.CHUNK))
    some = np.flatnonzero(per_chunk)
    assert (per_chunk[some[0]:some[-1]] == 0).sum() >= 20
    assert lc.P_ROWS % 2 == 1 and lc.P_COLS % 2 == 1 and 2 ** 31 < lc.LARGE_WEIGHT < 2 ** 32


# ---- the named defects
# Which tables see which defect: at connectivity 4, CORNERS mode, with row weights, under the variant the defect lives in (the
# scan defects under both, the ring sums under contract: sides_kernel is shared).  SCALED_PASS: scan_chunks in passes of 4 chunks,
# so that the small tiling's 7 chunks of nodes take two passes and its 11 chunks of sides three, as the large table's 1141 and
# 2086 take two and three passes of 1024.
SCALED_PASS = 4
SIDES_DEFECTS = ("atomic_issued_by_lane_0", "left_clears_first_only", "shortcut_at_popc_above_2", "lanes_past_B_in_the_ballot")
VARIANT_OF = {"jump_takes_the_later_index_at_a_tie": ("jump", "contract"), "no_local_minimum_starts": ("contract",), "head_chain_without_the_ring_totals": ("contract",),
              **{d: ("contract",) for d in SIDES_DEFECTS}}


def all_but(*names):
    return [n for n in NAMES if n not in names]


CAUGHT_BY = {
    # with passes of 4 chunks: every table of more than 4 chunks; with the kernel's 1024 none of these, only the large table
    "scan_chunks_forgets_the_carry": ["alternating_1x2049", "alternating_1x4095", "alternating_1x4097", "gap_row", "small_tiling"],
    "carry_replaced_not_added": ["alternating_1x2049", "alternating_1x4095", "alternating_1x4097", "gap_row", "small_tiling"],
    "wave_offset_takes_k_le_w": all_but(),
    "last_partial_chunk_not_scanned": all_but("alternating_1x2048", "rect_4096_sides", "rect_4098_sides", "head_at_2048"),
    "rounds_floor_log2": ["rect_2046_sides", "ring_2050", "rect_4098_sides", "one_tile_rect", "serpentine", "comb_across"],
    "jump_takes_the_later_index_at_a_tie": all_but(),
    "fin_from_the_wrong_buffer": all_but(),
    "no_local_minimum_starts": all_but(),
    "head_chain_without_the_ring_totals": all_but(),
    "atomic_issued_by_lane_0": ["alternating_1x2049", "alternating_1x4095", "random_3x683", "ring_2050", "rect_4098_sides",
                                "head_at_2047", "wrapped_1025", "long_beside_short", "triples_41", "triples_43", "random_15x63",
                                "random_16x64", "random_17x65", "random_31x127", "random_32x128", "random_33x129"],
    "left_clears_first_only": all_but(),
    "shortcut_at_popc_above_2": all_but("rect_2046_sides", "ring_2048", "ring_2050", "rect_4096_sides", "rect_4098_sides",
                                        "head_at_2047", "wrapped_1024", "wrapped_1025", "1x3_wrapped", "one_tile_rect", "serpentine",
                                        "comb_across", "band_60_cols", "band_70_cols"),
    "lanes_past_B_in_the_ballot": ["rect_2046_sides", "ring_2050", "rect_4098_sides", "head_at_2047", "head_at_2048", "wrapped_1025",
                                   "1x3_wrapped", "triples_41", "triples_43", "one_tile_rect", "comb_across", "band_60_cols",
                                   "band_70_cols", "random_17x65"],
}


def changed_by(defect, pass_len=lc.PASS, names=NAMES, variants=None, conn=4):
    out = []
    for name in names:
        labels, n, wrap = lc.tables()[name]
        want = traced(name, conn, om.CORNERS)
        for variant in variants or VARIANT_OF.get(defect, ("contract", "jump")):
            got = outlines_or_none(labels, n, conn, wrap, om.CORNERS, lc.weights_for(labels.shape[0]), variant, {defect}, pass_len)
            if not same(got, want):
                out.append(name)
                break
    return out


def tables_with(event):
    return [name for name in NAMES if event in lc.events(name, 4)]


@pytest.mark.parametrize("defect", DEFECTS)
def test_the_tables_that_catch_a_defect(defect):
    """The matrix: each defect changes the outlines of exactly the tables listed, and of at least one."""
    assert CAUGHT_BY[defect] and set(CAUGHT_BY) == set(DEFECTS)
    assert changed_by(defect, SCALED_PASS if "carry" in defect else lc.PASS) == CAUGHT_BY[defect]


@pytest.mark.parametrize("defect", ["scan_chunks_forgets_the_carry", "carry_replaced_not_added"])
def test_identity_one_pass_has_no_carry(defect):
    """Defects 1 and 2.  With the kernel's passes of 1024 chunks no small table takes a second pass, so none sees either: the
    large table alone does.  With passes of 4 chunks exactly the tables of more than 4 chunks do.  (Whoever puts defect 1 into
    the kernel to see the large table fail should do so for the heads scan alone: a lost carry in the scan of the nodes or of
    the chains makes compact indices collide, which leaves successor slots unwritten for a later kernel to follow.)"""
    assert changed_by(defect, variants=("contract",)) == []
    assert CAUGHT_BY[defect] == [n for n in NAMES if max(lc.n_chunks(lc.layout(n, 4)["N"]), lc.n_chunks(lc.layout(n, 4)["B"])) > SCALED_PASS]
    nodes, B, _ = lc.large_counts(lc.LARGE_TILING, 4)
    assert lc.n_chunks(nodes) > lc.PASS and lc.n_chunks(B) > 2 * lc.PASS


def test_what_the_carry_defects_lose():
    """Forgetting the carry restarts the offsets in every pass after the first and keeps the totals; replacing it keeps the
    second pass right and loses the third, so it takes more than 2048 chunks to show in the offsets."""
    labels, n, wrap = lc.tables()["small_tiling"]
    nodes = pairs((labels.reshape(-1) >= 0) * 4)
    right = chunked_scan(nodes, frozenset(), SCALED_PASS)
    forgot = chunked_scan(nodes, {"scan_chunks_forgets_the_carry"}, SCALED_PASS)
    assert (forgot[1] == right[1]).all() and (forgot[0][:4 * lc.CHUNK] == right[0][:4 * lc.CHUNK]).all()
    assert (forgot[0][4 * lc.CHUNK:, 0] != right[0][4 * lc.CHUNK:, 0]).all()
    sides = pairs(np.ones(11 * lc.CHUNK - 5))
    right = chunked_scan(sides, frozenset(), SCALED_PASS)
    replaced = chunked_scan(sides, {"carry_replaced_not_added"}, SCALED_PASS)
    assert (replaced[0][:8 * lc.CHUNK] == right[0][:8 * lc.CHUNK]).all() and (replaced[0][8 * lc.CHUNK:, 0] != right[0][8 * lc.CHUNK:, 0]).all()
    assert replaced[1][0] != right[1][0]


def test_identity_the_last_partial_chunk():
    """Defect 4: the last chunk keeps its own sum for an offset and is missing from the totals.  Identity: nothing changes when
    every scan's last partial chunk, if it has one, holds nothing: no side, no chain start, no head."""
    def tail_holds_nothing(values):
        n = len(values)
        return n % lc.CHUNK == 0 or not values[n - n % lc.CHUNK:].any()

    untouched = []
    for name in NAMES:
        S = lc.layout(name, 4)
        heads = np.zeros(S["B"], bool)
        heads[S["heads"]] = True
        if tail_holds_nothing(S["bits"]) and tail_holds_nothing(S["starts"]) and tail_holds_nothing(heads):
            untouched.append(name)
    assert CAUGHT_BY["last_partial_chunk_not_scanned"] == all_but(*untouched)


def test_identity_the_rounds():
    """Defect 5.  Identity: floor(log2 B) rounds are enough while no ring has more elements than 2^floor(log2 B): the sides
    of the ring under jump, its chains under contract.  Only a ring longer than half of everything shows it, and only under
    jump: chains are far fewer."""
    want = [n for n in NAMES if lc.layout(n, 4)["length"].max() > 1 << (lc.layout(n, 4)["B"].bit_length() - 1)]
    assert CAUGHT_BY["rounds_floor_log2"] == want
    assert changed_by("rounds_floor_log2", variants=("jump",)) == want
    assert changed_by("rounds_floor_log2", variants=("contract",)) == []


def test_identity_the_tie_rule():
    """Defect 6.  Identity: a ring of exactly 2^rounds sides, alone in its table, has no window that holds its head twice, so
    no tie is met under jump; the window of the last side before the head of any shorter ring does.  Under contract the
    elements are chains, and the windows go round every ring many times."""
    no_tie = [n for n in NAMES if "window_passes_its_head_twice" not in lc.events(n, 4)]
    assert no_tie == ["ring_2048", "rect_4096_sides", "1x1"]
    assert changed_by("jump_takes_the_later_index_at_a_tie", variants=("jump",)) == all_but(*no_tie)
    assert changed_by("jump_takes_the_later_index_at_a_tie", names=no_tie, variants=("contract",)) == no_tie


def test_identity_the_buffer_parity():
    """Defect 7: the other buffer holds the round before (jump) or the elements (contract).  Under jump that round is already
    final when no ring is longer than 2^(rounds - 1); under contract the elements are no per-side table, and it always shows."""
    stale_is_final = [n for n in NAMES if lc.layout(n, 4)["length"].max() <= 1 << (lc.layout(n, 4)["rounds"] - 1)]
    assert all_but(*stale_is_final) == ["rect_2046_sides", "ring_2048", "ring_2050", "rect_4096_sides", "rect_4098_sides", "1x1",
                                        "one_tile_rect", "serpentine", "comb_across"]
    assert changed_by("fin_from_the_wrong_buffer", variants=("jump",)) == all_but(*stale_is_final)
    assert changed_by("fin_from_the_wrong_buffer", variants=("contract",)) == NAMES


def test_identity_the_chain_starts():
    """Defect 8.  Identity: a ring whose head is a tile entry still has a chain that starts there (the other minima only
    split chains), so only a table in which every head is an entry could miss it.  There is none: the south ring of a
    wrapped row starts inside its tile."""
    assert [n for n in NAMES if lc.layout(n, 4)["entry"][lc.layout(n, 4)["heads"]].all()] == []
    assert CAUGHT_BY["no_local_minimum_starts"] == NAMES


def test_identity_the_head_chain():
    """Defect 9: the head's chain takes its element's d = sf = sx = 0 like any other chain.  Identity: a head's chain of one
    side holds the head alone, which gets zeros either way; every table here has a longer one."""
    one = [n for n in NAMES if lc.layout(n, 4)["starts"][lc.layout(n, 4)["next"][lc.layout(n, 4)["heads"]]].all()]
    assert one == [] and CAUGHT_BY["head_chain_without_the_ring_totals"] == NAMES


def test_identities_of_the_ring_sums():
    """Defects 10 .. 13 against the classifier's events.  10: the butterfly leaves the sum in every lane, so lane 0 holds it
    too unless the ring has one keyed side in the wave, at another lane.  11: the lanes left over are met again once their key
    is cleared, which needs a ring with several keyed sides.  12: only a ring with exactly two keyed sides in a wave skips
    its sum.  13: the lanes past B repeat the last side, which matters when it carries a term."""
    assert CAUGHT_BY["atomic_issued_by_lane_0"] == tables_with("one_keyed_side_not_at_lane_0")
    several = set(tables_with("ring_with_two_keyed_sides_in_a_wave")) | set(tables_with("ring_with_more_keyed_sides_in_a_wave"))
    assert set(CAUGHT_BY["left_clears_first_only"]) <= several
    assert set(CAUGHT_BY["shortcut_at_popc_above_2"]) <= set(tables_with("ring_with_two_keyed_sides_in_a_wave"))
    assert not {"ring_2048", "wrapped_1024"} & set(CAUGHT_BY["shortcut_at_popc_above_2"])     # whole waves of one ring
    assert CAUGHT_BY["lanes_past_B_in_the_ballot"] == tables_with("last_side_is_keyed_in_a_partial_wave")
