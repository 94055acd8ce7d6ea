"""The lane map of the region kernels' run reductions, label tables built for every edge of it, and a classifier that says
which edge a step of a table drives (DESIGN.md sections 4.26 and 4.27; the comments of stats_sum_kernel, wave_runs and
zonal_hist_kernel).

The lane map.  The sum kernels (stats_sum_kernel, zonal_sum_kernel, shape_sum_kernel, zonal_hist_kernel) walk the label table
as a flat array whatever rows x cols is: node n lies in stretch n // 1024, step (n % 1024) // 64, lane n % 64.  One wave owns
one stretch (a second one only above 2^28 nodes, which is not covered here) and takes it one step of 64 nodes at a time.  A
lane past the table's last node, or with an entry outside 0 .. n_regions - 1, is outside every region.  Inside a step a lane
outside every region takes the label of the last lane before it that is inside one, or the carried label when there is none,
and adds nothing; lanes that follow each other with one label are a run, summed into its first lane, the head.

Two carry rules.  The catalogue (stats_sum_kernel<true>): the carried run takes every run of its label among the step's heads
(one: a read from that lane; several: a butterfly); the other heads add to their records.  Only when no head has the carried
label is the carried run added to its record and the run that reaches lane 63 carried instead.  Zonal and shapes (wave_runs):
lane 0's run goes on the carried run when it has its label, else lane 0 adds the carried run to its record; the run that
reaches lane 63 is carried on and every other head adds its run.  In both, what is carried after the stretch's last step is
added then, and the next stretch starts with nothing carried.

The histogram (zonal_hist_kernel<true>): with rows of at most 128 columns a wave carries the columns of one region, that of the
step's first open lane (inside a region, value not NaN), column c in accumulator c // 64 of lane c % 64; they are added when
the carried region changes and after the stretch.  The open lanes of other regions (every open lane with wider rows) are
peeled by (region, column) key, first open lane first, 8 keys deep; the lanes still open add on their own.

Tables are flat int32 arrays with a list of lattices (rows, cols) to lay them on, no cols a multiple of 64, so that row ends
fall on every lane; `tables()` holds them, `cases()` every (table, lattice, wrap).  `classify` and `classify_hist` report the named
events per (stretch, step).  The closed forms at the end are the label tables and catalogues of sets far too large for the
Python model: isolated nodes and stripes."""
import functools

import numpy as np

WAVE, STEPS = 64, 16
STRETCH = WAVE * STEPS
PEEL, HCOLS = 8, 128
CHUNK = 4096                                                 # nodes per chunk of label_flatten_kernel's root counts

CATALOGUE_EVENTS = ("single_match", "several_matches", "flush_no_match", "no_match_nothing_carried", "lane0_hole_takes_carry",
                    "run_reaches_lane_63", "carry_emitted_after_last_step", "partial_last_step", "step_entirely_outside")
ZONAL_EVENTS = ("lane0_joins", "lane0_emits", "one_run_spans_step", "run_reaches_lane_63", "carry_emitted_after_last_step",
                "partial_last_step", "step_entirely_outside")
HIST_EVENTS = ("carried_region_changes", "first_open_lane_not_lane0", "keys_left_after_8_peels", "second_accumulator_used")


def lane_map(n):
    """(stretch, step, lane) of node n."""
    return n // STRETCH, (n % STRETCH) // WAVE, n % WAVE


def n_stretches(N):
    return (N + STRETCH - 1) // STRETCH


def steps_in(N, stretch):
    """The steps a wave takes in a stretch: it stops at the first step that starts at or past node N."""
    return min(STEPS, (N - stretch * STRETCH + WAVE - 1) // WAVE)


def step_labels(flat, n_regions, stretch, step, past=-1):
    """The 64 labels a wave sees in a step: -1 for a bad entry, `past` for a lane past the last node."""
    base = stretch * STRETCH + step * WAVE
    got = [int(v) if 0 <= v < n_regions else -1 for v in flat[base:base + WAVE]]
    return got + [past] * (WAVE - len(got))


def step_runs(labs, carry_l, holes_inherit=True):
    """The runs of a step as [label, first lane, lane after the last]: a lane outside every region takes the label before it."""
    runs, cur = [], carry_l
    for lane, l in enumerate(labs):
        cur = l if l >= 0 or not holes_inherit else cur
        if runs and runs[-1][0] == cur:
            runs[-1][2] = lane + 1
        else:
            runs.append([cur, lane, lane + 1])
    return runs


def classify(flat, n_regions):
    """{(stretch, step): {"catalogue": set of CATALOGUE_EVENTS, "zonal": set of ZONAL_EVENTS}} of a flat label table."""
    flat = np.asarray(flat).reshape(-1)
    N, out = flat.size, {}
    for s in range(n_stretches(N)):
        c_l, c_n, z_l, z_n = -1, 0, -1, 0                   # the carried label and its count of nodes, under either rule
        last = steps_in(N, s) - 1
        for t in range(last + 1):
            labs = step_labels(flat, n_regions, s, t)
            inside = [l >= 0 for l in labs]
            both = set()
            if N - s * STRETCH - t * WAVE < WAVE:
                both.add("partial_last_step")
            if not any(inside):
                both.add("step_entirely_outside")
            if inside[WAVE - 1]:
                both.add("run_reaches_lane_63")
            cat, zon = set(both), set(both)
            # the catalogue's rule
            runs = step_runs(labs, c_l)
            cnt = [sum(inside[a:b]) for _, a, b in runs]
            if not inside[0] and c_l >= 0:
                cat.add("lane0_hole_takes_carry")
            mine = [k for (l, _, _), k in zip(runs, cnt) if l >= 0 and k and l == c_l]
            if mine:
                cat.add("single_match" if len(mine) == 1 else "several_matches")
                c_n += sum(mine)
            else:
                cat.add("flush_no_match" if c_l >= 0 and c_n else "no_match_nothing_carried")
                c_l, c_n = runs[-1][0], cnt[-1]
            # wave_runs' rule
            runs = step_runs(labs, z_l)
            cnt = [sum(inside[a:b]) for _, a, b in runs]
            joined = runs[0][0] == z_l
            if z_l >= 0 and z_n:
                zon.add("lane0_joins" if joined else "lane0_emits")
            if len(runs) == 1 and runs[0][0] >= 0 and cnt[0]:
                zon.add("one_run_spans_step")
            z_n = cnt[-1] + (z_n if joined and len(runs) == 1 else 0)
            z_l = runs[-1][0]
            if t == last:
                if c_l >= 0 and c_n:
                    cat.add("carry_emitted_after_last_step")
                if z_l >= 0 and z_n:
                    zon.add("carry_emitted_after_last_step")
            out[(s, t)] = {"catalogue": cat, "zonal": zon}
    return out


def classify_hist(flat, n_regions, is_open, col, width):
    """{(stretch, step): set of HIST_EVENTS}: is_open (N,) bool says whose value is not NaN, col (N,) the column it falls in."""
    flat = np.asarray(flat).reshape(-1)
    N, out = flat.size, {}
    carrying = width <= HCOLS
    for s in range(n_stretches(N)):
        carried = -1
        for t in range(steps_in(N, s)):
            base = s * STRETCH + t * WAVE
            labs = step_labels(flat, n_regions, s, t)
            lanes = [k for k in range(min(WAVE, N - base)) if labs[k] >= 0 and is_open[base + k]]
            ev = set()
            if lanes and lanes[0] != 0:
                ev.add("first_open_lane_not_lane0")
            if carrying and lanes:
                if labs[lanes[0]] != carried:
                    if carried >= 0:
                        ev.add("carried_region_changes")
                    carried = labs[lanes[0]]
                if any(labs[k] == carried and col[base + k] >= WAVE for k in lanes):
                    ev.add("second_accumulator_used")
            keys = {(labs[k], int(col[base + k])) for k in lanes if not (carrying and labs[k] == carried)}
            if len(keys) > PEEL:
                ev.add("keys_left_after_8_peels")
            out[(s, t)] = ev
    return out


def events_of(classified, rule=None):
    """Every event that occurs somewhere, with the first (stretch, step) it occurs at."""
    seen = {}
    for key in sorted(classified):
        for e in sorted(classified[key][rule] if rule else classified[key]):
            seen.setdefault(e, key)
    return seen


# ---- the tables
def _steps(*steps):
    """A flat table from steps, each a list of (label, length) runs that fill 64 lanes."""
    out = []
    for runs in steps:
        lanes = [l for l, k in runs for _ in range(k)]
        assert len(lanes) == WAVE, (runs, len(lanes))
        out += lanes
    return out


PAIRS = [(a, b) for a in range(WAVE) for b in range(a, WAVE)]
PAIR_FILL = (len(PAIRS), len(PAIRS) + 1)                     # the two labels of the lanes round the runs


def pairs_table():
    """One step per (head lane a, last lane b): region k, the k-th pair's, fills lanes a .. b.  The lanes before it are outside
    every region (k odd) or region 2080; the lanes after it are outside (k & 2), else region 2080 or 2081 (k & 4): a filler that
    reaches lane 63 is carried and meets the next step's filler (a match) or another label (a flush)."""
    lanes = []
    for k, (a, b) in enumerate(PAIRS):
        before = -1 if k & 1 else PAIR_FILL[0]
        after = -1 if k & 2 else PAIR_FILL[1 if k & 4 else 0]
        lanes += [before] * a + [k] * (b - a + 1) + [after] * (WAVE - 1 - b)
    return np.array(lanes, np.int32), len(PAIRS) + 2


A, B, C_, D, E, F, H, I_ = range(8)
CARRY_UNUSED = 8                                             # a label no node carries
CARRY_64 = 9                                                 # the first of 64 labels that share one step


def carry_table():
    """Two stretches and a ragged end, step by step (the comments name what the step is there for)."""
    hole = -1
    islands5 = [(D, 5), (E, 3), (D, 5), (F, 3), (D, 5), (E, 3), (D, 5), (F, 3), (D, 5), (E, 3), (D, 24)]
    flat = _steps(
        [(hole, 10), (A, 54)],                               # 0  a run that ends exactly at lane 63 ...
        [(A, 20), (B, 44)],                                  # 1  ... goes on from lane 0; B reaches lane 63, A stays carried
        [(C_, 64)],                                          # 2  another label at lane 0: A is over; C's first node at lane 0
        [(hole, 5), (C_, 59)],                               # 3  lanes 0 .. 4 outside, then the carried label again
        [(hole, 7), (D, 57)],                                # 4  lanes 0 .. 6 outside, then another label
        [(D, 64)],                                           # 5  one run spans the step
        [(hole, 64)],                                        # 6  64 lanes outside in the middle of a carried run
        [(D, 64)],                                           # 7  ... which goes on
        [(E, 5), (D, 59)],                                   # 8  an island at the step's start: one match beside another head
        [(D, 20), (E, 5), (D, 39)],                          # 9  one island: two runs match
        [(D, 10), (E, 5), (D, 10), (F, 5), (D, 34)],         # 10 two islands: three runs match
        islands5,                                            # 11 five islands: six runs match
        [(A, 1), (B, 1)] * 32,                               # 12 a, b, a, b, ...: D is over, the B of lane 63 is carried
        [(A, 1), (B, 1)] * 32,                               # 13 32 runs match
        [(CARRY_64 + k, 1) for k in range(64)],              # 14 64 labels in one step
        [(hole, 4), (H, 60)],                                # 15 a run that crosses node 1024: added after the stretch ...
        [(H, 64)],                                           # 16 ... and the next wave starts with nothing carried
        [(H, 63), (I_, 1)],                                  # 17 I's first node sits at lane 63
        [(I_, 64)],                                          # 18
        [(hole, 64)],                                        # 19 I is over: nothing of it is left to add at the next step
        [(hole, 64)],                                        # 20 no head and nothing carried
        [(hole, 63), (I_, 1)],                               # 21 a run of one node at lane 63 ...
        [(hole, 1), (I_, 1), (hole, 62)],                    # 22 ... lane 0 outside takes its label, lane 1 goes on
        [(B, 64)],                                           # 23
    )
    # the rest of the second stretch: runs of random lengths over regions A .. F and outside
    rng = np.random.default_rng(64)
    while len(flat) < 2 * STRETCH:
        flat += [int(rng.integers(-1, 6))] * int(rng.integers(1, 40))
    flat = flat[:2 * STRETCH]
    flat += [F] * 30 + [hole] * 20 + [A] * 61                # 17 x 127 = 2159 nodes: a third stretch of 111 nodes, 47 in its last step
    assert len(flat) == 17 * 127
    return np.array(flat, np.int32), CARRY_64 + 64


TAIL_SIZES = {1: [(1, 1)], 63: [(9, 7), (1, 63)], 64: [(2, 32)], 65: [(5, 13)], 1023: [(11, 93)], 1024: [(32, 32)],
              1025: [(25, 41)], 2 * 1024 + 1: [(3, 683)], 2 * 1024 + 63: [(1, 2111)]}


def tail_table(N):
    """N nodes: runs of random lengths over regions 0 .. 2 and outside, and region 3 from some node on to the last.  One node:
    region 0 alone, as a table cannot hold more regions than nodes."""
    if N == 1:
        return np.array([0], np.int32), 1
    rng = np.random.default_rng(N)
    flat = []
    while len(flat) < N:
        flat += [int(rng.integers(-1, 3))] * int(rng.integers(1, 30))
    flat = flat[:N]
    k = min(N, 70)                                           # from 1025 nodes on it crosses the last stretch's start
    flat[N - k:] = [3] * k
    return np.array(flat, np.int32), 4


HIST_WIDTHS = (64, 65, 128, 129)
HIST_MANY = 4                                                # the first of 20 regions that share one step


def hist_table():
    """(flat labels, n_regions, flat float32 field).  The field's values are k + 0.5 for integers k in -2 .. 131 and NaN; with
    lo = 0 and hi = n_bins they fall in column 0 (below), k + 1, and n_bins + 1 (at or above the top)."""
    many = [(HIST_MANY + k, 2) for k in range(20)]
    flat = _steps(
        [(A, 64)],                                           # 0  region A carried
        [(A, 20), (B, 24), (A, 20)],                         # 1  B's lanes are peeled beside the carried A
        [(B, 64)],                                           # 2  the carried region changes ...
        [(A, 64)],                                           # 3  ... and comes back
        [(A, 1), (B, 10), (A, 53)],                          # 4  lane 0 NaN: lane 1, of B, decides, and A's lanes are peeled
        [(B, 4)] + many + [(B, 20)],                         # 5  B carried, 40 lanes of 20 other regions: more than 8 keys
        [(-1, 30), (C_, 34)],                                # 6  the first open lane is lane 30
        [(C_, 64)],                                          # 7
    )
    rng = np.random.default_rng(128)
    while len(flat) < STRETCH + 5 * WAVE:                    # into a second stretch
        flat += [int(rng.integers(-1, 4))] * int(rng.integers(1, 50))
    flat = flat[:STRETCH + 5 * WAVE]
    flat += [C_] * (11 * 127 - len(flat))                    # 11 x 127 = 1397 nodes: 53 in the last step
    lab = np.array(flat, np.int32)
    n = lab.size
    k = np.arange(n, dtype=np.uint64)
    h = (k * 2654435761 + 12345) % 4294967296
    h = ((h ^ (h >> 15)) * 2246822519) % 4294967296
    h ^= h >> 13
    x = ((h % 134).astype(np.float64) - 2.0 + 0.5).astype(np.float32)
    x[h % 19 == 0] = np.nan
    # columns 0, 63, 64 and 127 of the carried region in step 0 (width 128: n_bins = 126), and the top column at every width
    x[0:8] = np.array([-1.5, 62.5, 63.5, 126.5, 200.0, -0.5, 61.5, 127.5], np.float32)
    x[4 * WAVE] = np.nan                                     # step 4, lane 0
    x[4 * WAVE + 1:4 * WAVE + 12] = np.float32(70.5)         # open, and in the second accumulator
    x[5 * WAVE:6 * WAVE] = (np.arange(64) % 7 + 60.5).astype(np.float32)       # step 5: open, columns on both sides of 64
    return lab, HIST_MANY + 20, x


def hist_columns(x, n_bins):
    """(is_open, col) of field values with lo = 0, hi = n_bins, as zonal_hist_kernel bins them."""
    x = np.asarray(x, np.float32).reshape(-1)
    is_open = ~np.isnan(x)
    t = np.where(is_open, x, 0).astype(np.float64)
    col = np.where(t < 0, 0, np.where(t >= n_bins, n_bins + 1, 1 + np.floor(np.clip(t, 0, n_bins)).astype(np.int64)))
    return is_open, col


@functools.lru_cache(maxsize=None)
def tables():
    """{name: (flat labels, n_regions, [(rows, cols), ...])}, read-only."""
    out = {"pairs": (*pairs_table(), [(2048, 65)]), "carry": (*carry_table(), [(17, 127), (127, 17)])}
    for N, shapes in TAIL_SIZES.items():
        out[f"tails_{N}"] = (*tail_table(N), shapes)
    lab, n, _ = hist_table()
    out["hist"] = (lab, n, [(11, 127)])
    for flat, _, shapes in out.values():
        flat.setflags(write=False)
        assert all(r * c == flat.size and c % 64 for r, c in shapes)
    return out


def cases():
    """[(table, rows, cols, wrap)]: every table on every lattice of its own, wrapped (cols >= 3) and not."""
    return [(name, r, c, w) for name, (_, _, shapes) in tables().items() for r, c in shapes for w in (False, True) if c >= 3 or not w]


def case_id(case):
    name, r, c, w = case
    return f"{name}-{r}x{c}{'-wrapped' if w else ''}"


def row_weights(rows, heavy=False):
    """(rows,) uint32, distinct per row; heavy: near 2^32 - 1."""
    return ((2 ** 32 - 1 - rows if heavy else 1000) + np.arange(rows)).astype(np.uint32)


# ---- closed forms: sets whose labelling and catalogue are known without a union-find
RECORD = np.dtype([("weight", "<u8"), ("sum_i", "<i8"), ("sum_dj", "<i8"), ("count", "<u4"), ("root_i", "<i4"),
                   ("root_j", "<i4"), ("i_min", "<i4"), ("i_max", "<i4"), ("dj_min", "<i4"), ("dj_max", "<i4"),
                   ("reserved", "<u4")])


def even_nodes(rows, cols, wrap):
    """The nodes with even i and even j, with wrap and odd cols without the last column, which would touch column 0: no two
    touch at either connectivity."""
    i, j = np.mgrid[0:rows, 0:cols]
    even = (i % 2 == 0) & (j % 2 == 0)
    if wrap and cols % 2:
        even &= j != cols - 1
    return even


def isolated_mask(rows, cols, wrap, seed, target=200000, band=32):
    """A random subset of even_nodes.  The density goes by bands of rows through 0, 1 and a value between chosen so that about
    `target` nodes are set: some chunks of 4096 nodes hold no root, some every root they can."""
    i = np.arange(rows)[:, None]
    even = even_nodes(rows, cols, wrap)
    p = min(max((target / max(int(even.sum()), 1) - 0.125) / 0.75, 0.02), 0.9)
    density = np.array([0.0, 1.0, p, p, p, p, p, p])[(i // band) % 8]
    return (even & (np.random.default_rng(seed).random((rows, cols)) < density)).astype(np.uint8)


def isolated_answer(mask, weights=None):
    """(labels, K, catalogue) of a mask of nodes no two of which touch: every node its own region, in row-major order."""
    m = np.asarray(mask) != 0
    labels = np.where(m, np.cumsum(m.reshape(-1)).reshape(m.shape) - 1, -1).astype(np.int32)
    i, j = np.nonzero(m)                                    # row-major
    t = np.zeros(i.size, RECORD)
    t["weight"] = 1 if weights is None else np.asarray(weights)[i]
    t["sum_i"], t["count"], t["root_i"], t["root_j"], t["i_min"], t["i_max"] = i, 1, i, j, i, i
    return labels, int(i.size), t


def stripes_mask(rows, cols):
    m = np.zeros((rows, cols), np.uint8)
    m[0::2, :] = 1
    return m


def stripes_answer(rows, cols, wrap, weights=None):
    """(labels, K, catalogue) of every second row full: region k is row 2 k, its root (2 k, 0).  dj runs over 0 .. cols - 1
    without wrap.  With wrap, dj = ((j + h) mod cols) - h with h = cols // 2: for even cols j < h keeps dj = j and j >= h gives
    j - cols, so dj runs over -h .. h - 1 and sums to -h; for odd cols = 2 h + 1, j <= h keeps dj = j and j > h gives
    j - cols = -h .. -1, so dj runs over -h .. h and sums to 0."""
    K = (rows + 1) // 2
    labels = np.full((rows, cols), -1, np.int32)
    labels[0::2, :] = np.arange(K, dtype=np.int32)[:, None]
    i = 2 * np.arange(K, dtype=np.int64)
    t = np.zeros(K, RECORD)
    t["weight"] = cols if weights is None else np.asarray(weights, np.uint64)[i] * np.uint64(cols)
    t["sum_i"], t["count"], t["root_i"], t["root_j"], t["i_min"], t["i_max"] = i * cols, cols, i, 0, i, i
    h = cols // 2
    if not wrap:
        t["sum_dj"], t["dj_min"], t["dj_max"] = cols * (cols - 1) // 2, 0, cols - 1
    elif cols % 2 == 0:
        t["sum_dj"], t["dj_min"], t["dj_max"] = -h, -h, h - 1
    else:
        t["sum_dj"], t["dj_min"], t["dj_max"] = 0, -h, h
    return labels, K, t


RANK_LATTICES = ((1024, 1024), (1030, 1021), (1536, 2731))  # 256, 257 and 1025 chunks of 4096 nodes


def scan_split(n_chunks):
    """How label_scan_kernel's 256 lanes share the chunks: (chunks per lane, lanes that hold any, lanes clipped to the end)."""
    per = (n_chunks + 255) // 256
    used = (n_chunks + per - 1) // per
    return per, used, 256 - used
