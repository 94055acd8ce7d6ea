"""What the host and the GPU tests of mrtx_contours share: the built cases, the random lattices, the raw call and the list of
refusals.  A case is (z (rows, cols) int32, levels, wrap)."""
import ctypes as C

import numpy as np

from moonrtx_amd import _lib

VOID = 2 ** 31 - 1


def arr(rows):
    return np.array(rows, np.int32)


def comb(n=67, is_open=False):
    """One serpentine line: a spine along row 1 with a tooth down every odd column, clear of the border (closed), or with
    the spine run out to column 0 (open)."""
    z = np.zeros((n, n), np.int32)
    z[1, 1:n - 1] = 1
    z[1:n - 1, 1:n - 1:2] = 1
    if is_open:
        z[1, 0] = 1
    return z


def built_cases():
    out = {}
    # all 16 corner patterns of a single cell (bit 0 NW, 1 NE, 2 SE, 3 SW)
    for p in range(16):
        out[f"pattern_{p:02d}"] = (arr([[p & 1, p >> 1 & 1], [p >> 3 & 1, p >> 2 & 1]]), [1], False)
    # both saddles with the centre above, below and at the tie sum == 4 c - 2
    out["saddle_nw_se_above"] = (arr([[2, 0], [0, 2]]), [1], False)
    out["saddle_nw_se_below"] = (arr([[1, -5], [-5, 1]]), [1], False)
    out["saddle_nw_se_tie"] = (arr([[1, 0], [0, 1]]), [1], False)
    out["saddle_nw_se_just_below"] = (arr([[1, 0], [-1, 1]]), [1], False)
    out["saddle_ne_sw_above"] = (arr([[0, 2], [2, 0]]), [1], False)
    out["saddle_ne_sw_below"] = (arr([[-5, 1], [1, -5]]), [1], False)
    out["saddle_ne_sw_tie"] = (arr([[0, 1], [1, 0]]), [1], False)
    out["saddle_tie_at_the_bounds"] = (arr([[2 ** 30, 2 ** 30 - 1], [2 ** 30 - 1, 2 ** 30]]), [2 ** 30], False)
    out["saddle_on_the_seam"] = (arr([[0, 0, 3], [3, 0, 0], [0, 0, 3]]), [1, 2, 3], True)
    # lattices without cells: every crossed edge is a line of one vertex
    out["1x1"] = (arr([[5]]), [1, 5, 6], False)
    out["1x2"] = (arr([[0, 4]]), [1, 4], False)
    out["2x1"] = (arr([[0], [4]]), [1, 4], False)
    out["1x5"] = (arr([[0, 4, 0, 4, 2]]), [1, 3], False)
    out["5x1"] = (arr([[0], [4], [0], [4], [2]]), [1, 3], False)
    out["1x5_wrapped"] = (arr([[0, 4, 0, 4, 2]]), [1, 3], True)
    out["2x5"] = (arr([[0, 4, 0, 4, 2], [4, 0, 2, 2, 0]]), [1, 3], False)
    out["5x2"] = (arr([[0, 4], [4, 0], [0, 2], [4, 2], [2, 0]]), [1, 3], False)
    # a cone: one closed line per level
    d = np.abs(np.arange(5) - 2)
    out["cone"] = ((4 - d[:, None] - d[None, :]).astype(np.int32), [3, 4], False)
    out["pit"] = ((d[:, None] + d[None, :]).astype(np.int32), [1, 2], False)
    # a ramp: open lines from edge to edge
    ramp = np.tile(10 * np.arange(5, dtype=np.int32), (4, 1))
    out["ramp"] = (ramp, [5, 15, 25], False)
    out["ramp_down_the_rows"] = (np.ascontiguousarray(ramp.T), [5, 15, 25], False)
    # one edge crossed by three levels at once, and levels that cross nothing
    out["three_levels_on_an_edge"] = (arr([[0, 10], [0, 10]]), [-5, 1, 5, 10, 11], False)
    out["levels_that_cross_nothing"] = (ramp, [-7, 0, 41, 99], False)
    # void nodes
    v = np.tile(10 * np.arange(5, dtype=np.int32), (5, 1))
    v[2, 2] = VOID
    out["void_in_the_middle"] = (v, [5, 15, 25, 35], False)
    v = np.tile(10 * np.arange(5, dtype=np.int32), (5, 1))
    v[2, :] = VOID
    out["void_row"] = (v, [5, 15], False)
    out["all_void"] = (np.full((4, 5), VOID, np.int32), [0, 1], False)
    # wrap
    out["wrap_cols_3"] = (arr([[0, 3, 1], [2, 0, 3], [3, 1, 0]]), [1, 2, 3], True)
    s = np.zeros((4, 6), np.int32)
    s[1:3, 5] = s[1:3, 0] = 5
    out["across_the_seam"] = (s, [3], True)
    out["across_the_seam_unwrapped"] = (s, [3], False)
    pole = np.tile(10 * np.arange(4, dtype=np.int32)[:, None], (1, 6))
    out["ring_round_the_pole"] = (pole, [15], True)
    out["ring_round_the_pole_other_way"] = (np.ascontiguousarray(-pole), [-15], True)
    out["ring_round_the_pole_unwrapped"] = (pole, [15], False)
    # counts that cross a node chunk and an element chunk of 2048
    stripes = np.tile((10 * (np.arange(1400) % 2)).astype(np.int32), (3, 1))
    out["stripes_3x1400"] = (stripes, [3, 7], False)
    out["stripes_3x1400_wrapped"] = (stripes, [3, 7], True)
    # one serpentine line of more than 4096 elements: 13 rounds of the pointer jumping
    out["comb_closed"] = (comb(67, False), [1], False)
    out["comb_open"] = (comb(67, True), [1], False)
    # more levels than the level table in LDS holds
    out["many_levels"] = (arr([[0, 5000, 0], [5000, 0, 5000], [0, 5000, 0]]), list(range(1, 5001)), False)
    return out


FLAVOURS = [(0, 0), (0, 1), (1, 0), (1, 1)]          # (wrap, voids)


def random_cases(flavour, n=200):
    """n seeded lattices of 1 .. 8 x 1 .. 10 nodes (3 .. 10 columns under wrap) with heights in 0 .. 3, so that ties abound,
    and 1 .. 5 levels out of -1 .. 5."""
    wrap, voids = flavour
    rng = np.random.default_rng(7000 + 10 * wrap + voids)
    out = []
    for _ in range(n):
        rows, cols = int(rng.integers(1, 9)), int(rng.integers(3 if wrap else 1, 11))
        z = rng.integers(0, 4, (rows, cols)).astype(np.int32)
        if voids:
            z[rng.random((rows, cols)) < rng.choice([0.05, 0.2, 0.5])] = VOID
        levels = np.sort(rng.choice(np.arange(-1, 6), int(rng.integers(1, 6)), replace=False)).tolist()
        out.append((z, levels, bool(wrap)))
    return out


# ---- the raw call
def block(rows=8, cols=9, wrap=0, n_levels=3, reserved=0):
    return _lib.MrtxContours(rows, cols, wrap, n_levels, reserved)


def contour_call(lib, ctx, k, z=None, dev_z=None, levels=None, dev_lines=None, lines=None, line_cap=0, dev_vertices=None,
                 vertices=None, vertex_cap=0, counts=None, block=True, st=None):
    """mrtx_contours with numpy arrays for the host tables and integers for the device tables."""
    ptr = lambda a: None if a is None else a.ctypes.data
    nl, nv = counts if counts is not None else (C.c_uint64(0), C.c_uint64(0))
    return lib.mrtx_contours(ctx, C.byref(k) if block else None, dev_z, ptr(z), ptr(levels), dev_lines, ptr(lines), line_cap,
                             dev_vertices, ptr(vertices), vertex_cap, C.byref(nl) if nl is not None else None,
                             C.byref(nv) if nv is not None else None, C.byref(st) if st is not None else None)


def refusal_tables():
    """(z (8, 9), levels (3,), lines (4,), vertices (16,)): the host tables of the refusal cases; the outputs zeroed."""
    return np.zeros((8, 9), np.int32), np.array([1, 2, 3], np.int32), np.zeros(4, _lib.CONTOUR_LINE_DTYPE), np.zeros(16, np.int32)


def refusal_cases(z, levels, lines, vertices, dev):
    """[(a pattern of the refusal's text, keyword arguments of contour_call)]; dev: the address of 8192 bytes of device memory, or
    any 16-byte aligned number where no device is present: no case gets as far as reading it."""
    F = dict(z=z, levels=levels, lines=lines, line_cap=4, vertices=vertices, vertex_cap=16)
    D = dict(dev_z=dev, levels=levels, dev_lines=dev + 512, line_cap=4, dev_vertices=dev + 1024, vertex_cap=16)
    lv = lambda *a: np.array(a, np.int32)
    return [
        ("null contours block", dict(F, k=block(), block=False)),
        ("reserved must be 0", dict(F, k=block(reserved=1))),
        ("empty lattice", dict(F, k=block(rows=0))),
        ("empty lattice", dict(F, k=block(cols=-3))),
        ("at most 2\\^31 nodes", dict(F, k=block(rows=65536, cols=32769))),
        ("at most 2\\^28 nodes", dict(F, k=block(rows=16384, cols=16385))),
        ("wrap must be 0 or 1", dict(F, k=block(wrap=2))),
        ("cols >= 3", dict(F, k=block(cols=2, wrap=1))),
        ("n_levels must lie in 1 .. 65536 \\(got 0\\)", dict(F, k=block(n_levels=0))),
        ("n_levels must lie in 1 .. 65536 \\(got 65537\\)", dict(F, k=block(n_levels=65537))),
        ("n_levels must lie in 1 .. 65536 \\(got -1\\)", dict(F, k=block(n_levels=-1))),
        ("null host_levels", dict(F, k=block(), levels=None)),
        ("the levels must ascend strictly \\(level 2 = 2 follows 2\\)", dict(F, k=block(), levels=lv(1, 2, 2))),
        ("the levels must ascend strictly \\(level 1 = 0 follows 1\\)", dict(F, k=block(), levels=lv(1, 0, 2))),
        ("level 0 must lie in -2\\^30 \\+ 1 .. 2\\^30 \\(got -1073741824\\)", dict(F, k=block(), levels=lv(-2 ** 30, 0, 2))),
        ("level 2 must lie in -2\\^30 \\+ 1 .. 2\\^30 \\(got 1073741825\\)", dict(F, k=block(), levels=lv(0, 1, 2 ** 30 + 1))),
        ("exactly one of dev_z and host_z", dict(F, k=block(), z=None)),
        ("exactly one of dev_z and host_z", dict(F, k=block(), dev_z=dev)),
        ("null n_lines or n_vertices", dict(F, k=block(), counts=(None, C.c_uint64(5)))),
        ("null n_lines or n_vertices", dict(F, k=block(), counts=(C.c_uint64(5), None))),
        ("at most one of dev_lines and host_lines", dict(F, k=block(), dev_lines=dev)),
        ("at most one of dev_vertices and host_vertices", dict(F, k=block(), dev_vertices=dev)),
        ("a line table and a vertex table, or neither", dict(F, k=block(), lines=None)),
        ("a line table and a vertex table, or neither", dict(F, k=block(), vertices=None)),
        ("without tables line_cap and vertex_cap must be 0", dict(z=z, levels=levels, k=block(), line_cap=1)),
        ("without tables line_cap and vertex_cap must be 0", dict(z=z, levels=levels, k=block(), vertex_cap=1)),
        ("dev_z must be 4-byte aligned", dict(D, k=block(), dev_z=dev + 2)),
        ("dev_lines must be 8-byte aligned", dict(D, k=block(), dev_lines=dev + 516)),
        ("dev_vertices must be 4-byte aligned", dict(D, k=block(), dev_vertices=dev + 1026)),
        ("must not overlap", dict(D, k=block(), dev_lines=dev + 280)),
        ("must not overlap", dict(D, k=block(), dev_vertices=dev + 284)),
        ("must not overlap", dict(D, k=block(), dev_vertices=dev + 512 + 124)),
    ]


def assert_refused(lib, ctx, text, kw, lines, vertices):
    """One refusal: the code, the text, the counts and the statistics as they were, the host tables untouched."""
    import re
    kw = dict(kw)
    nl, nv = kw.pop("counts", (C.c_uint64(5), C.c_uint64(5)))
    st = _lib.MrtxStats()
    st.launches, st.kernel_ms = 0xABCD, -7.0
    assert contour_call(lib, ctx, counts=(nl, nv), st=st, **kw) == -1, text
    msg = lib.mrtx_last_error(ctx).decode()
    assert re.search(text, msg), (text, msg)
    assert (nl is None or nl.value == 5) and (nv is None or nv.value == 5), text
    assert st.launches == 0xABCD and st.kernel_ms == -7.0, text
    assert (lines.view(np.uint8) == 0).all() and (vertices == 0).all(), text
