"""The lane and chunk map of the outline kernels, label tables built for every edge of it, and a
classifier that says which edges a table holds.

The map.  mark, base, chain_sum, chain_index, heads_sum and heads_write take their items (nodes, or boundary sides by compact
index) in chunks of 2048 per block: thread t of 256 takes items 8 t .. 8 t + 7 of the chunk, a wave 512 items, and block_scan
gives every thread the sum of the threads before it through four per-wave sums.  scan_chunks, one block of 1024, turns the
chunks' sums into prefix sums in passes of 1024 chunks with a carry from pass to pass.  The pointer jumping runs
rounds = ceil(log2 B) times over two buffers; contract's elements are the chains of sides inside a tile of 16 x 64 nodes.
sides_kernel takes one side per thread, 64 per wave and 256 per block, and sums a ring's row terms in the wave before the
atomics; only north and south sides (k = 0, 2) carry a term, they are the keyed sides.

The number of boundary sides is even on every table: each vertical run of one label in a column has one north and one south
side, and each horizontal run one east and one west side (a run that goes round the seam has none).  So B mod 64 is never 1 or
63; the nearest edges, 2 and 62, stand in for them.

`tables()` holds the small tables, `layout` the sides, rings and chains of one at a connectivity (from a vectorised restatement
of the side and successor rules, which tests/test_outline_layouts_host.py compares with tests/outline_model.py), `events` the
named edges it holds.  The large table at the end is composed, not traced.

The longest chain.  A chain ends at the next side whose index is below both neighbours', so along a chain the compact index
rises and then falls.  It rises along north sides going east, east sides going south and the turns N -> E -> S -> W at one
node, and from row to row; it falls across the seam within a row.  North sides of one ring in rows i and i + 1 never share a
column (the node above a north side lies outside the region), so a rising run inside a tile of 16 rows stays short: the
longest chains found are those of the serpentine (133 sides) and of the 1 x k rectangles (129).  The event is therefore a
chain of at least 128 sides, two waves of sides_kernel; nothing in the kernels changes with a chain's length below
MRTX_OL_CHAIN_MAX = 4096, which a tile's 4096 sides bound."""
import functools

import numpy as np

import outline_model as om

CHUNK, RUN, WAVE_ITEMS, WAVES, PASS = 2048, 8, 512, 4, 1024
TILE_H, TILE_W = 16, 64
SIDE_WAVE, SIDE_BLOCK = 64, 256

TY, TX = np.array([0, 1, 0, -1]), np.array([1, 0, -1, 0])   # travel direction of side k
DY, DX = np.array([-1, 0, 1, 0]), np.array([0, 1, 0, -1])   # outward direction of side k

SCAN_EVENTS = ("run_cut_by_the_end", "wave_offset_after_empty_waves", "wave_offset_after_full_waves", "empty_chunk_between",
               "head_first_in_a_later_chunk", "head_last_in_a_chunk", "last_chunk_holds_one_item", "B_fills_its_chunks")
ROUND_EVENTS = ("rounds_even", "rounds_odd", "ring_of_2_pow_rounds_sides", "ring_of_2_pow_k_plus_2_sides", "ring_of_odd_length",
                "window_passes_its_head_twice", "dead_buffer_as_full_as_it_gets")
CHAIN_EVENTS = ("ring_in_one_tile_started_by_its_head_alone", "chain_is_its_whole_ring", "head_chain_followed_by_2_chains",
                "head_is_entry_and_minimum", "ring_enters_one_tile_4_times", "chain_of_128_sides", "winding_ring_inside_one_tile",
                "rows_16k_minus_1", "rows_16k", "rows_16k_plus_1", "cols_64k_minus_1", "cols_64k", "cols_64k_plus_1")
SUM_EVENTS = ("ring_fills_whole_waves", "sixteen_rings_of_two_keys_in_a_wave", "ring_with_one_keyed_side_in_a_wave",
              "one_keyed_side_not_at_lane_0", "ring_with_two_keyed_sides_in_a_wave", "ring_with_more_keyed_sides_in_a_wave",
              "partial_sum_is_zero", "B_mod_64_is_2",
              "B_mod_64_is_62", "B_mod_256_not_0", "last_side_is_keyed_in_a_partial_wave")
EVENTS = SCAN_EVENTS + ROUND_EVENTS + CHAIN_EVENTS + SUM_EVENTS


def rounds_of(B):
    r = 0
    while (1 << r) < B:
        r += 1
    return r


def n_chunks(n):
    return -(-n // CHUNK)


def weights_for(rows):
    """distinct per row and near 2^32, so that warea needs 64 bits (as tests/test_gpu_outline.py)"""
    return (2 ** 32 - 1 - 3 * np.arange(rows)).astype(np.uint32)


# ---- the sides of a table and their successors
def sides_of(labels, n_regions, conn, wrap):
    """The boundary sides of a label table in ascending side id, which is the compact order: bits (N,) per node, sid (B,),
    next (B,) the successor's compact index, turns (B,) whether the successor is another kind of side, enters (B,) whether the
    successor lies in another tile of nodes."""
    lab = np.asarray(labels, np.int64)
    rows, cols = lab.shape
    lab = np.where((lab >= 0) & (lab < n_regions), lab, -1)

    def at(i, j):
        ok = (i >= 0) & (i < rows)
        if wrap:
            j = np.where(j < 0, cols - 1, np.where(j >= cols, 0, j))
        ok &= (j >= 0) & (j < cols)
        out = np.full(i.shape, -1, np.int64)
        out[ok] = lab[i[ok], j[ok]]
        return out, i * cols + j

    I, J = np.divmod(np.arange(rows * cols), cols)
    L = lab.reshape(-1)
    mask = np.stack([(L >= 0) & (at(I + DY[k], J + DX[k])[0] != L) for k in range(4)], axis=1)
    sid = np.flatnonzero(mask.reshape(-1))
    B = sid.size
    compact = np.full(4 * rows * cols, -1, np.int64)
    compact[sid] = np.arange(B)
    v, k = sid >> 2, sid & 3
    i, j, l = I[v], J[v], L[v]
    la, av = at(i + TY[k], j + TX[k])
    lb, bv = at(i + TY[k] + DY[k], j + TX[k] + DX[k])
    left = (lb == l) & ((la == l) | (conn == 8))
    straight = ~left & (la == l)
    sv = np.where(left, bv, np.where(straight, av, v))
    sk = np.where(left, (k + 3) & 3, np.where(straight, k, (k + 1) & 3))
    nxt = compact[4 * sv + sk]
    assert (nxt >= 0).all(), "the successor of a boundary side is a boundary side"
    enters = (I[sv] // TILE_H != i // TILE_H) | (J[sv] // TILE_W != j // TILE_W)
    bits = (mask * (1 << np.arange(4))).sum(1)
    return dict(rows=rows, cols=cols, N=rows * cols, B=B, bits=bits, sid=sid, next=nxt, turns=sk != k, enters=enters, sv=sv, sk=sk)


def cycles(nxt):
    """ring (B,) the number of each side's ring in order of the heads, pos (B,) its distance from the head along the ring."""
    B = len(nxt)
    ring, pos, heads = np.full(B, -1, np.int64), np.zeros(B, np.int64), []
    nx = nxt.tolist()
    for c in range(B):
        if ring[c] >= 0:
            continue
        t, p = c, 0
        while ring[t] < 0:
            ring[t], pos[t] = len(heads), p
            t, p = nx[t], p + 1
        assert t == c, "the successor map is a permutation"
        heads.append(c)
    return ring, pos, np.array(heads, np.int64)


@functools.lru_cache(maxsize=None)
def layout(name, conn):
    labels, n, wrap = tables()[name]
    S = sides_of(labels, n, conn, wrap)
    B = S["B"]
    S["rounds"] = rounds_of(B)
    S["ring"], S["pos"], S["heads"] = cycles(S["next"])
    S["length"] = np.bincount(S["ring"], minlength=len(S["heads"]))
    # contract's chain starts: the ring enters the side's tile there, or the side's index is below both neighbours'
    pred = np.empty(B, np.int64)
    pred[S["next"]] = np.arange(B)
    entry = np.empty(B, bool)
    entry[S["next"]] = S["enters"]
    c = np.arange(B)
    S["pred"], S["entry"] = pred, entry
    S["starts"] = entry | ((c < pred) & (c < S["next"]))
    return S


def chain_lengths(S):
    """The length of every chain, by walking each ring once from a start."""
    out, nx, st = [], S["next"].tolist(), S["starts"].tolist()
    for h in S["heads"].tolist():
        t, n = h, 0                                            # a head is a start
        while True:
            n += 1
            t = nx[t]
            if st[t]:
                out.append(n)
                n = 0
            if t == h:
                break
    return out


def scan_events(values, ev):
    """The edges of one chunked scan over per-item values."""
    n = len(values)
    if n % RUN:
        ev.add("run_cut_by_the_end")
    if n % CHUNK == 1:
        ev.add("last_chunk_holds_one_item")
    pad = np.zeros(n_chunks(n) * CHUNK, np.int64)
    pad[:n] = values
    waves = pad.reshape(-1, WAVES, WAVE_ITEMS)
    sums = waves.sum(2)
    full = (waves != 0).all(2)
    for w in range(1, WAVES):
        used = sums[:, w] != 0
        if (used & (sums[:, :w] == 0).all(1)).any():
            ev.add("wave_offset_after_empty_waves")
        if (used & full[:, :w].all(1)).any():
            ev.add("wave_offset_after_full_waves")
    chunk = sums.sum(1) != 0
    some = np.flatnonzero(chunk)
    if some.size and (~chunk[some[0]:some[-1]]).any():
        ev.add("empty_chunk_between")


@functools.lru_cache(maxsize=None)
def events(name, conn):
    """The named edges that a table holds at a connectivity."""
    S = layout(name, conn)
    B, ev = S["B"], set()
    if not B:
        return frozenset()
    rows, cols, wrap = S["rows"], S["cols"], tables()[name][2]
    heads, length, ring = S["heads"], S["length"], S["ring"]
    is_head = np.zeros(B, np.int64)
    is_head[heads] = 1
    scan_events(np.array([bin(b).count("1") for b in S["bits"].tolist()]), ev)
    scan_events(S["starts"].astype(np.int64), ev)
    scan_events(is_head, ev)
    if (heads[heads >= CHUNK] % CHUNK == 0).any():
        ev.add("head_first_in_a_later_chunk")
    if (heads % CHUNK == CHUNK - 1).any():
        ev.add("head_last_in_a_chunk")
    if B % CHUNK == 0:
        ev.add("B_fills_its_chunks")
    # rounds
    rounds = S["rounds"]
    ev.add("rounds_odd" if rounds & 1 else "rounds_even")
    if (length == 1 << rounds).any():
        ev.add("ring_of_2_pow_rounds_sides")
    if (length == (1 << (rounds - 1)) + 2).any():
        ev.add("ring_of_2_pow_k_plus_2_sides")
    if (length % 2 == 1).any():
        ev.add("ring_of_odd_length")
    if length.min() + 2 <= 1 << rounds:                     # the window of the last side before the head holds it twice
        ev.add("window_passes_its_head_twice")
    if 48 * len(heads) + 8 * B >= 24 * B:                   # ALL mode: a vertex per side
        ev.add("dead_buffer_as_full_as_it_gets")
    # chains
    starts_in = np.bincount(ring[S["starts"]], minlength=len(heads))
    entries_in = np.bincount(ring[S["entry"]], minlength=len(heads))
    assert S["starts"][heads].all() and starts_in.min() >= 1, "every ring has a chain that starts at its head"
    if ((starts_in == 1) & (entries_in == 0)).any():
        ev.add("ring_in_one_tile_started_by_its_head_alone")
    if (starts_in == 1).any():
        ev.add("chain_is_its_whole_ring")
    if (starts_in >= 3).any():
        ev.add("head_chain_followed_by_2_chains")
    if S["entry"][heads].any():
        ev.add("head_is_entry_and_minimum")
    v = S["sid"] >> 2
    tile = (v // cols // TILE_H) * (-(-cols // TILE_W)) + v % cols // TILE_W
    e = np.flatnonzero(S["entry"])
    if e.size and np.unique(np.stack([ring[e], tile[e]]), axis=1, return_counts=True)[1].max() >= 4:
        ev.add("ring_enters_one_tile_4_times")
    if max(chain_lengths(S)) >= 128:
        ev.add("chain_of_128_sides")
    k = S["sid"] & 3
    wind = (np.bincount(ring[k == 0], minlength=len(heads)) - np.bincount(ring[k == 2], minlength=len(heads))) // cols
    if wrap and cols <= TILE_W and ((wind != 0) & (entries_in == 0)).any():
        ev.add("winding_ring_inside_one_tile")
    for what, size, tile_size in (("rows_16k", rows, TILE_H), ("cols_64k", cols, TILE_W)):
        r = size % tile_size
        if r in (tile_size - 1, 0, 1) and size >= tile_size - 1:
            ev.add(what + {tile_size - 1: "_minus_1", 0: "", 1: "_plus_1"}[r])
    # ring sums
    keyed = (k == 0) | (k == 2)
    term = np.where(k == 0, -(v // cols), np.where(k == 2, v // cols + 1, 0))
    c = np.arange(B)
    wave = c // SIDE_WAVE
    per_wave = np.bincount(wave, minlength=-(-B // SIDE_WAVE))
    one_ring = np.array([len(set(ring[a:a + SIDE_WAVE].tolist())) == 1 for a in range(0, B, SIDE_WAVE)])
    whole = one_ring & (per_wave == SIDE_WAVE)
    if (whole[1:] & whole[:-1] & (ring[SIDE_WAVE::SIDE_WAVE][:len(whole) - 1] == ring[:-SIDE_WAVE:SIDE_WAVE][:len(whole) - 1])).any():
        ev.add("ring_fills_whole_waves")
    pairs, first, inv, count = np.unique(np.stack([wave[keyed], ring[keyed]]), axis=1, return_index=True, return_inverse=True,
                                         return_counts=True)
    sums = np.zeros(len(count), np.int64)
    np.add.at(sums, inv.reshape(-1), term[keyed])
    if (np.bincount(pairs[0][count == 2], minlength=1) >= 16).any():
        ev.add("sixteen_rings_of_two_keys_in_a_wave")
    if (count == 1).any():
        ev.add("ring_with_one_keyed_side_in_a_wave")
        if (c[keyed][first][count == 1] % SIDE_WAVE != 0).any():
            ev.add("one_keyed_side_not_at_lane_0")
    if (count == 2).any():
        ev.add("ring_with_two_keyed_sides_in_a_wave")
    if (count > 2).any():
        ev.add("ring_with_more_keyed_sides_in_a_wave")
    if (sums == 0).any():
        ev.add("partial_sum_is_zero")
    if B % SIDE_WAVE in (2, 62):
        ev.add(f"B_mod_64_is_{B % SIDE_WAVE}")
    if B % SIDE_BLOCK:
        ev.add("B_mod_256_not_0")
    if B % SIDE_WAVE and keyed[B - 1]:
        ev.add("last_side_is_keyed_in_a_partial_wave")
    assert ev <= set(EVENTS), ev - set(EVENTS)
    return frozenset(ev)


# ---- the tables
def _alternating(cols):
    """One row of labels 0, 1, 0, 1, ...: every node its own ring of four sides, so every item of every scan counts."""
    return (np.arange(cols) % 2).astype(np.int32)[None, :]


def _gap_row():
    """1 x 6145: chunk 0 holds nodes in its third wave only, chunk 1 none, chunk 2 every node, and the last chunk is one node."""
    m = np.full(3 * CHUNK + 1, -1, np.int32)
    m[2 * WAVE_ITEMS:3 * WAVE_ITEMS] = np.arange(WAVE_ITEMS) % 2
    m[2 * CHUNK:3 * CHUNK] = np.arange(CHUNK) % 2
    m[3 * CHUNK] = 0
    return m[None, :]


def _rect_inside(k):
    """A 1 x k rectangle, 2 k + 2 sides, in the middle row of a 3 x (k + 2) lattice."""
    m = np.full((3, k + 2), -1, np.int32)
    m[1, 1:k + 1] = 0
    return m


def _head_at(c):
    """Two rows: a 2 x (c - 2) rectangle, which has c sides on row 0, and a node of another label after it on row 0, whose
    north side is side c."""
    m = np.full((2, c), -1, np.int32)
    m[:, :c - 2] = 0
    m[0, c - 1] = 1
    return m


def _long_beside_short():
    """3 x 600: row 0 is one ring of 1202 sides, row 2 holds 300 rings of four sides."""
    m = np.full((3, 600), -1, np.int32)
    m[0] = 0
    m[2, ::2] = 1
    return m


def _triples(rows):
    """rows x 3, wrapped, every second row set: every ring has three sides, the least a ring can have."""
    m = np.full((rows, 3), -1, np.int32)
    m[::2] = np.arange((rows + 1) // 2, dtype=np.int32)[:, None]
    return m


def _one_tile_rect():
    """A 3 x 3 block inside one tile.  Its ring has two chains: the turn from the south side to the west side of its last
    row's first node rises in index, so that south side is a minimum too.  Only a one-node ring, or a ring that winds inside
    one tile, is started by its head alone."""
    m = np.full((TILE_H, TILE_W), -1, np.int32)
    m[2:5, 2:5] = 0
    return m


def _serpentine():
    """One path that fills a tile: the even rows, joined at alternating ends, and a last node on row 15: 520 nodes."""
    m = np.full((TILE_H, TILE_W), -1, np.int32)
    m[0:15:2] = 0
    m[1:14:4, TILE_W - 1] = 0
    m[3:14:4, 0] = 0
    m[15, TILE_W - 1] = 0
    return m


def _saddle_rows():
    """16 x 64, wrapped: columns 0 .. 62 of every even row and column 63 of every odd row.  At connectivity 8 each odd node
    joins the rows above and below it through four saddles, two of them across the seam, which is no tile border here."""
    m = np.full((TILE_H, TILE_W), -1, np.int32)
    m[0::2, :TILE_W - 1] = 0
    m[1::2, TILE_W - 1] = 0
    return m


def _comb_across():
    """20 x 130: a spine in column 60 with seven teeth that reach across the tile border at column 64."""
    m = np.full((20, 130), -1, np.int32)
    m[1:14, 60] = 0
    m[1:14:2, 60:71] = 0
    return m


def _band(rows, cols, a, b):
    m = np.full((rows, cols), -1, np.int32)
    m[a:b] = 0
    return m


def _random(rows, cols, seed):
    rng = np.random.default_rng(seed)
    mask = rng.random((rows, cols)) < 0.55
    return np.where(mask, (np.arange(cols) // 5 % 3)[None, :], -1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def tables():
    """{name: (labels (rows, cols) int32, n_regions, wrap)}, read-only."""
    out = {}
    for cols, wrap in ((2047, False), (2048, False), (2049, True), (4095, True), (4097, False)):
        out[f"alternating_1x{cols}"] = (_alternating(cols), 2, wrap)
    out["random_3x683"] = (_random(3, 683, 683), 3, True)     # 2049 nodes
    out["gap_row"] = (_gap_row(), 2, False)
    out["rect_2046_sides"] = (_rect_inside(1022), 1, False)
    out["ring_2048"] = (np.zeros((1, 1023), np.int32), 1, False)
    out["ring_2050"] = (np.zeros((1, 1024), np.int32), 1, False)
    out["rect_4096_sides"] = (_rect_inside(2047), 1, False)
    out["rect_4098_sides"] = (_rect_inside(2048), 1, True)
    out["head_at_2047"] = (_head_at(2047), 2, False)
    out["head_at_2048"] = (_head_at(2048), 2, False)
    out["wrapped_1024"] = (np.zeros((1, 1024), np.int32), 1, True)
    out["wrapped_1025"] = (np.zeros((1, 1025), np.int32), 1, True)
    out["1x1"] = (np.zeros((1, 1), np.int32), 1, False)
    out["1x3_wrapped"] = (np.zeros((1, 3), np.int32), 1, True)
    out["long_beside_short"] = (_long_beside_short(), 2, False)
    out["triples_41"] = (_triples(41), 21, True)
    out["triples_43"] = (_triples(43), 22, True)
    out["one_tile_rect"] = (_one_tile_rect(), 1, False)
    out["serpentine"] = (_serpentine(), 1, False)
    out["saddle_rows"] = (_saddle_rows(), 1, True)
    out["comb_across"] = (_comb_across(), 1, False)
    out["band_60_cols"] = (_band(7, 60, 2, 5), 1, True)
    out["band_70_cols"] = (_band(7, 70, 2, 5), 1, True)
    for k, (rows, cols) in enumerate(((15, 63), (16, 64), (17, 65), (31, 127), (32, 128), (33, 129))):
        out[f"random_{rows}x{cols}"] = (_random(rows, cols, rows), 3, bool(k & 1))
    out["small_tiling"] = (large_labels(SMALL_TILING), 7, False)
    for labels, _, _ in out.values():
        labels.setflags(write=False)
    return out


DEAD_BUFFER = ("triples_41", "triples_43")


# ---- the large table: composed, not traced
P_ROWS, P_COLS = 23, 45                                      # the pattern's periods, both odd
LARGE_TILING = (48, 47)                                      # copies down and across: 1104 x 2115 = 2 334 960 nodes
LARGE_BLANK = tuple((20, b) for b in range(47)) + ((0, 3), (31, 46), (47, 0))    # a whole row of copies, and three more
SMALL_TILING = (3, 4)
SMALL_BLANK = ((1, 2),)
LARGE_WEIGHT = 4000000007                                    # one weight for every row, near 2^32


def pattern():
    """A checkerboard of 22 x 44 nodes with an empty last row and column: copies touch at neither connectivity."""
    i, j = np.mgrid[0:P_ROWS, 0:P_COLS]
    return (i < P_ROWS - 1) & (j < P_COLS - 1) & ((i + j) % 2 == 0)


def blanks_of(tiling):
    return LARGE_BLANK if tiling == LARGE_TILING else SMALL_BLANK


def large_labels(tiling):
    """The pattern tiled; copy (a, b) carries the label (a * across + b) mod 7, and the blanked copies nothing."""
    down, across = tiling
    copy = (np.arange(down)[:, None] * across + np.arange(across)[None, :]) % 7
    for a, b in blanks_of(tiling):
        copy[a, b] = -1
    lab = np.kron(copy, np.ones((P_ROWS, P_COLS), np.int64))
    return np.where(np.tile(pattern(), tiling) & (lab >= 0), lab, -1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def pattern_outlines(conn, mode):
    rings, vertices = om.trace(np.where(pattern(), 0, -1), conn, False, mode)
    assert (rings["wind"] == 0).all() and rings["first"].tolist() == (np.cumsum(rings["n_vertices"]) - rings["n_vertices"]).tolist()
    return rings, vertices


def compose(tiling, conn, mode, weight=None):
    """The outlines of large_labels(tiling): the pattern's rings moved to every copy (the head and the vertices move, the areas
    of a ring that does not wind do not), in the order of their heads; first is the running sum of n_vertices; with one weight
    for every row warea = weight * area."""
    down, across = tiling
    cols = across * P_COLS
    rings, vertices = pattern_outlines(conn, mode)
    a, b = np.mgrid[0:down, 0:across]
    keep = np.ones(tiling, bool)
    for blank in blanks_of(tiling):
        keep[blank] = False
    a, b = a[keep], b[keep]
    head = rings["head"].astype(np.int64)
    v, k = head >> 2, head & 3
    moved = 4 * ((v // P_COLS + P_ROWS * a[:, None]) * cols + v % P_COLS + P_COLS * b[:, None]) + k      # (copies, rings)
    order = np.argsort(moved.reshape(-1), kind="stable")
    copy, r = np.divmod(order, len(rings))
    out = rings[r]
    out["head"] = moved.reshape(-1)[order]
    out["label"] = ((a * across + b) % 7)[copy]
    out["warea"] = out["area"] * (1 if weight is None else int(weight))
    out["first"] = np.cumsum(out["n_vertices"].astype(np.uint64)) - out["n_vertices"]
    # the vertices of ring r of the pattern, per output ring
    nv = rings["n_vertices"].astype(np.int64)
    take = np.repeat(rings["first"].astype(np.int64)[r] - (np.cumsum(nv[r]) - nv[r]), nv[r]) + np.arange(int(nv[r].sum()))
    shift = np.stack([np.repeat(P_ROWS * a[copy], nv[r]), np.repeat(P_COLS * b[copy], nv[r])], axis=1)
    return out, (vertices[take] + shift).astype(np.int32)


def large_counts(tiling, conn):
    """(nodes, B, rings) of the tiling."""
    down, across = tiling
    copies = down * across - len(blanks_of(tiling))
    rings, _ = pattern_outlines(conn, om.CORNERS)
    return down * P_ROWS * across * P_COLS, int(rings["n_sides"].sum()) * copies, len(rings) * copies
