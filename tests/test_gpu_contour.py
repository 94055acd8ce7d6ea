"""The contour lines on the GPU: mrtx_contours / MoonRT.contours against tests/contour_model.py.
Every field of every line record and every vertex is compared with ==."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import contour_cases as cc
import contour_model as cm
import model_cases as mc
from common import assert_bit_equal
from moonrtx_amd import _lib
from moonrtx_amd import contours as ct
from moonrtx_amd.renderer import DeviceBuffer, MoonRT, MoonRTError
from moonrtx_amd.scene import named_scene
from test_gpu_illumination import make

pytestmark = pytest.mark.gpu

LINE = _lib.CONTOUR_LINE_DTYPE
CASES = cc.built_cases()


@pytest.fixture(scope="module")
def rt(native_lib):
    """One context for the module, without a DEM, a light or a Moon frame: the stage needs none of them."""
    r = MoonRT(16, 16)
    yield r
    r.close()


def assert_contours_equal(got, lines, vertices, what):
    assert got.lines.shape == lines.shape, (what, got.lines.shape, lines.shape)
    for name in LINE.names:
        bad = np.flatnonzero(got.lines[name] != lines[name])
        assert bad.size == 0, (what, name, int(bad[0]), got.lines[bad[0]], lines[bad[0]])
    assert got.vertices.shape == vertices.shape, (what, got.vertices.shape, vertices.shape)
    bad = np.flatnonzero(got.vertices != vertices)
    assert bad.size == 0, (what, "vertex", int(bad[0]), int(got.vertices[bad[0]]), int(vertices[bad[0]]))


def run(rt, z, levels, wrap, device, stats=None):
    z = np.ascontiguousarray(z, np.int32)
    if not device:
        return rt.contours(z, levels, wrap, stats=stats)
    buf = DeviceBuffer(max(z.size * 4, 4))
    try:
        buf.upload(z)
        got = rt.contours(buf, levels, wrap, shape=z.shape, stats=stats)
        assert (got.z == z).all()
        return got
    finally:
        buf.free()


def check(rt, z, levels, wrap, what):
    """From a host and from a device table, against the model."""
    lines, vertices = cm.trace(z, levels, wrap)
    for device in (False, True):
        assert_contours_equal(run(rt, z, levels, wrap, device), lines, vertices, (what, device))


@pytest.mark.parametrize("name", list(CASES))
def test_built_cases_equal_the_model(rt, name):
    check(rt, *CASES[name], name)


@pytest.mark.parametrize("flavour", cc.FLAVOURS)
def test_random_lattices_equal_the_model(rt, flavour):
    cases = cc.random_cases(flavour)
    assert len(cases) >= 200
    for n, (z, levels, wrap) in enumerate(cases):
        check(rt, z, levels, wrap, (flavour, n))


def test_a_larger_lattice_equals_the_model(rt):
    """128 x 128 with ties, voids and the seam: several chunks of nodes and of elements, lines of every length."""
    rng = np.random.default_rng(11)
    y, x = np.mgrid[0:128, 0:128]
    z = np.rint(6.0 * np.sin(x * (2 * np.pi / 128) * 3) * np.cos(y * 0.21) + rng.integers(-1, 2, (128, 128))).astype(np.int32)
    z[40:44, 100:110] = cc.VOID
    z[90, 127] = z[91, 0] = cc.VOID
    for wrap in (False, True):
        check(rt, z, [-4, -1, 0, 1, 3, 5], wrap, ("128x128", wrap))


# ---- the cap protocol
def contour_call(rt, k, z=None, **kw):
    return cc.contour_call(rt._lib, rt._ctx, k, z, **kw)


def test_the_cap_protocol(rt):
    z, levels, wrap = CASES["wrap_cols_3"]
    lv = np.array(levels, np.int32)
    want_l, want_v = cm.trace(z, levels, wrap)
    L, V = len(want_l), len(want_v)
    k = cc.block(*z.shape, int(wrap), len(levels))
    nl, nv = C.c_uint64(77), C.c_uint64(77)
    assert contour_call(rt, k, z, levels=lv, counts=(nl, nv)) == 0                      # the count call
    assert (nl.value, nv.value) == (L, V)
    for device in (False, True):
        lines, vertices = np.zeros(L + 2, LINE), np.zeros(V + 2, np.int32)
        lb, vb = DeviceBuffer(32 * (L + 2)), DeviceBuffer(4 * (V + 2))
        try:
            def call(line_cap, vertex_cap):
                nl.value = nv.value = 77
                lines.view(np.uint8)[:] = 0xAB
                vertices.view(np.uint8)[:] = 0xAB
                lb.upload(lines)
                vb.upload(vertices)
                if device:
                    rc_ = contour_call(rt, k, z, levels=lv, dev_lines=lb.ptr, line_cap=line_cap, dev_vertices=vb.ptr, vertex_cap=vertex_cap,
                                       counts=(nl, nv))
                    return rc_, lb.download(LINE, (L + 2,)), vb.download(np.int32, (V + 2,))
                rc_ = contour_call(rt, k, z, levels=lv, lines=lines, line_cap=line_cap, vertices=vertices, vertex_cap=vertex_cap,
                                   counts=(nl, nv))
                return rc_, lines.copy(), vertices.copy()
            for caps in ((L, V), (L + 2, V + 2)):                                       # exact caps fill, and so do larger ones
                rc_, gl, gv = call(*caps)
                assert rc_ == 0 and (nl.value, nv.value) == (L, V)
                assert_contours_equal(ct.Contours(gl[:L], gv[:V], z, levels, wrap), want_l, want_v, ("caps", caps, device))
                assert (gl[L:].view(np.uint8) == 0xAB).all() and (gv[V:].view(np.uint8) == 0xAB).all()
            for caps in ((L - 1, V), (L, V - 1), (0, 0)):                               # a cap one short
                rc_, gl, gv = call(*caps)
                assert rc_ == -1 and (nl.value, nv.value) == (L, V), caps
                msg = rt._lib.mrtx_last_error(rt._ctx).decode()
                assert f"{L} lines and {V} vertices are needed" in msg, msg
                assert (gl.view(np.uint8) == 0xAB).all() and (gv.view(np.uint8) == 0xAB).all(), caps
        finally:
            lb.free()
            vb.free()


def test_every_refusal(rt):
    """Each text, the counts and the statistics as they were, no table touched, on the host or on the device (that no refusal
    makes a device call is shown without a device, in tests/test_contour_host.py)."""
    z, levels, lines, vertices = cc.refusal_tables()
    dev = DeviceBuffer(8192)
    try:
        dev.upload(np.full(8192, 0xAB, np.uint8))
        for text, kw in cc.refusal_cases(z, levels, lines, vertices, dev.ptr):
            cc.assert_refused(rt._lib, rt._ctx, text, kw, lines, vertices)
        assert (dev.download(np.uint8, (8192,)) == 0xAB).all()
        check(rt, *CASES["wrap_cols_3"], "after the refusals")                          # the context still works
    finally:
        dev.free()


def test_a_bad_height_is_refused_after_the_first_launches(rt):
    z, levels, wrap = CASES["void_in_the_middle"]
    lv = np.array(levels, np.int32)
    k = cc.block(*z.shape, int(wrap), len(levels))
    lines, vertices = np.zeros(64, LINE), np.zeros(64, np.int32)
    for bad in (2 ** 30 + 1, -2 ** 30 - 1, -2 ** 31, 2 ** 31 - 2):
        mine = z.copy()
        mine[1, 3] = bad
        nl, nv = C.c_uint64(5), C.c_uint64(5)
        st = _lib.MrtxStats()
        assert contour_call(rt, k, mine, levels=lv, counts=(nl, nv), st=st) == -1, bad
        assert "1 heights lie outside -2^30 .. 2^30" in rt._lib.mrtx_last_error(rt._ctx).decode()
        assert st.launches == 3 and st.kernel_ms > 0.0                                  # out says what ran
        assert contour_call(rt, k, mine, levels=lv, lines=lines, line_cap=64, vertices=vertices, vertex_cap=64, counts=(nl, nv)) == -1, bad
        assert (nl.value, nv.value) == (5, 5) and (lines.view(np.uint8) == 0).all() and (vertices == 0).all()
        with pytest.raises(MoonRTError, match="heights lie outside"):
            run(rt, mine, levels, wrap, True)
    # the bounds themselves are heights, and MRTX_FILL_NONE is a void node
    edge = z.copy()
    edge[0, 0], edge[4, 4], edge[1, 3] = 2 ** 30, -2 ** 30, cc.VOID
    check(rt, edge, levels, wrap, "heights at the bounds")


def test_too_many_crossings_are_refused_after_the_count(rt):
    """A checkerboard of the two bounds under 65536 levels: every edge is crossed by every level, almost 2^33 elements.  The
    chunks' sums are scanned in 64 bits, so the text names the true number."""
    i, j = np.mgrid[0:256, 0:256]
    z = np.where((i + j) % 2 == 0, 2 ** 30, -2 ** 30).astype(np.int32)
    levels = (np.arange(65536, dtype=np.int64) * 32768 - 2 ** 30 + 1).astype(np.int32)
    assert levels[0] == -2 ** 30 + 1 and levels[-1] <= 2 ** 30 and (np.diff(levels) > 0).all()
    B = 2 * 256 * 255 * 65536
    assert B >= 2 ** 32
    k = cc.block(256, 256, 0, 65536)
    lines, vertices = np.zeros(4, LINE), np.zeros(16, np.int32)
    for tables in (dict(), dict(lines=lines, line_cap=4, vertices=vertices, vertex_cap=16)):
        nl, nv = C.c_uint64(5), C.c_uint64(5)
        st = _lib.MrtxStats()
        assert contour_call(rt, k, z, levels=levels, counts=(nl, nv), st=st, **tables) == -1
        msg = rt._lib.mrtx_last_error(rt._ctx).decode()
        assert f"{B} times" in msg and "2^31" in msg, msg
        assert st.launches == 3 and (nl.value, nv.value) == (5, 5)
        assert (lines.view(np.uint8) == 0).all() and (vertices == 0).all()
    check(rt, *CASES["wrap_cols_3"], "after the refusal")


def rounds_of(B):
    r = 0
    while (1 << r) < B:
        r += 1
    return r


def test_launches_depend_on_the_lattice_the_levels_and_the_crossings_alone(rt):
    rng = np.random.default_rng(5)
    z = rng.integers(0, 4, (37, 61)).astype(np.int32)
    mirror = np.ascontiguousarray(z[:, ::-1])
    levels = [1, 2, 3]
    seen = []
    for tab in (z, mirror):
        st = {}
        got = rt.contours(tab, levels, stats=st)
        B = int(got.vertices.shape[0])
        assert st["launches"] > 0 and st["kernel_ms"] > 0.0 and st["count_ms"] > 0.0 and st["fill_ms"] > 0.0
        seen.append((st["launches"], B))
    assert seen[0] == seen[1], seen
    # the count call: three launches of the count, five and ceil(log2 B) of the trace; the fill call: two more
    B = seen[0][1]
    assert seen[0][0] == 2 * (3 + 5 + rounds_of(B)) + 2
    lv = np.array(levels, np.int32)
    s1 = _lib.MrtxStats()
    assert contour_call(rt, cc.block(37, 61, 0, 3), z, levels=lv, st=s1) == 0 and s1.launches == 3 + 5 + rounds_of(B)
    # nothing crossed: the count alone
    s0 = _lib.MrtxStats()
    assert contour_call(rt, cc.block(37, 61, 0, 3), z, levels=np.array([7, 8, 9], np.int32), st=s0) == 0 and s0.launches == 3


def test_leaves_the_render_state_alone(native_lib):
    s = named_scene("S1", 16, 16).with_size(48, 32, spp_per_launch=16)
    dem = mc.crater_dem()
    z, levels, wrap = CASES["wrap_cols_3"]
    want = cm.trace(z, levels, wrap)

    def go(with_contours):
        r = make(s, dem, _lib.F_COUNT_STATS)
        st1 = r.render(1)
        if with_contours:
            assert_contours_equal(run(r, z, levels, wrap, False), *want, "between two renders")
            run(r, *CASES["comb_closed"], True)
        st2 = r.render(1)
        out = r.read_linear(), r.read_hits(), r.samples_done(), st1, st2
        r.close()
        return out
    a, b = go(False), go(True)
    assert_bit_equal(b[0], a[0], "linear radiance")
    assert_bit_equal(b[1], a[1], "hit buffer")
    assert b[2] == a[2] == 32
    for key in ("primary_hits", "shadow_rays", "height_samples", "bounce_rays"):
        assert b[4][key] == a[4][key], key


def test_the_contour_tool(native_lib, tmp_path):
    """tools/contour_map.py end to end on a small saved map: a warm patch across the seam with a gap in the data."""
    import csv
    import json
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import contour_map as tool
    rows, cols = 40, 96
    y, x = np.mgrid[0:rows, 0:cols]
    dx = (x + 48) % cols - 48
    temps = np.zeros((rows, cols, 2), np.float32)
    temps[:, :, 1] = 150.0 * np.exp(-(dx * dx + (y - 20) ** 2) / 90.0).astype(np.float32) + 40.0
    temps[19:22, 7:10, 1] = np.nan
    np.save(tmp_path / "temps.npy", temps)
    window = (2000, 0, rows, cols, 480, 1)
    p = subprocess.run([sys.executable, os.path.join(root, "tools", "contour_map.py"), "--map", str(tmp_path / "temps.npy"), "--channel", "1",
                        "--unit", "0.01", "--window", *[str(v) for v in window], "--levels", "110", "60.5", "500", "--min-vertices", "4",
                        "--geojson", str(tmp_path / "c.geojson"), "--csv", str(tmp_path / "c.csv")], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    z = tool.quantise(temps[:, :, 1], 0.01)
    levels = tool.level_table(z, 0.01, levels=[110, 60.5, 500])
    assert levels.tolist() == [6050, 11000, 50000] and (z == ct.VOID).sum() == 9
    lines, vertices = cm.trace(z, levels, True)
    cs = ct.Contours(lines, vertices, z, levels, True)
    assert len(cs) >= 2 and not lines["closed"].all() and lines["closed"].any()
    with open(tmp_path / "c.geojson") as f:
        fc = json.load(f)
    assert fc == json.loads(json.dumps(tool.feature_collection(cs, window, (23040, 46080), 0.01, 4)))
    assert {f["properties"]["level"] for f in fc["features"]} == {60.5, 110.0}
    closed = [f for f in fc["features"] if f["properties"]["closed"]]
    assert closed and all(f["geometry"]["coordinates"][0] == f["geometry"]["coordinates"][-1] for f in closed)
    lon = [pt[0] for f in closed for pt in f["geometry"]["coordinates"]]
    assert min(lon) < -180.0 and max(lon) - min(lon) < 180.0                            # continuous across the seam
    with open(tmp_path / "c.csv") as f:
        got = list(csv.reader(f))
    want = [[str(v) for v in row] for row in tool.vertex_rows(cs, window, (23040, 46080), 0.01, 4)]
    assert got[0] == tool.HEADER and got[1:] == want and len(want) > 20


# ---- one large lattice, device only, against numpy's own crossed-edge sets
def crossed_sets(z, levels):
    """Per level the sorted ids of the crossed edges of a lattice without wrap, by numpy."""
    rows, cols = z.shape
    valid = z != cc.VOID
    v = np.arange(rows * cols, dtype=np.int64).reshape(rows, cols)
    out = []
    for c in levels:
        a = z >= c
        east = valid[:, :-1] & valid[:, 1:] & (a[:, :-1] != a[:, 1:])
        south = valid[:-1, :] & valid[1:, :] & (a[:-1, :] != a[1:, :])
        out.append(np.sort(np.concatenate([2 * v[:, :-1][east], 2 * v[:-1, :][south] + 1])))
    return out


def cells_of(e, rows, cols, cell_ok):
    """(n, 2) the ids of the two cells an edge may be a side of, -1 where the cell does not exist or has a void corner."""
    v, k = e >> 1, e & 1
    i, j = v // cols, v % cols
    ci = np.stack([i, np.where(k == 0, i - 1, i)], -1)
    cj = np.stack([j, np.where(k == 0, j, j - 1)], -1)
    inside = (ci >= 0) & (ci < rows - 1) & (cj >= 0) & (cj < cols - 1)
    ok = inside & cell_ok[np.clip(ci, 0, rows - 2), np.clip(cj, 0, cols - 2)]
    return np.where(ok, ci * cols + cj, -1), inside


def share_a_cell(a, b):
    hit = np.zeros(a.shape[0], bool)
    for p in (0, 1):
        for q in (0, 1):
            hit |= (a[:, p] >= 0) & (a[:, p] == b[:, q])
    return hit


def test_a_1024_lattice_on_the_device_keeps_the_identities(rt):
    rows = cols = 1024
    rng = np.random.default_rng(3)
    y, x = np.mgrid[0:rows, 0:cols].astype(np.float64)
    f = np.zeros((rows, cols))
    for _ in range(12):                                             # a smooth random field
        ky, kx, ph = rng.uniform(-0.06, 0.06), rng.uniform(-0.06, 0.06), rng.uniform(0, 2 * np.pi)
        f += rng.uniform(0.3, 1.0) * np.sin(ky * y + kx * x + ph)
    z = np.rint(1000.0 * f).astype(np.int32)
    z[300:340, 500:560] = cc.VOID
    levels = ct.levels_for(-2000, 2000, 500)
    assert levels.size == 8
    st = {}
    got = run(rt, z, levels, False, True, stats=st)
    lines, verts = got.lines, got.vertices.astype(np.int64)
    n = lines["n_vertices"].astype(np.int64)
    first = lines["first"].astype(np.int64)
    assert len(lines) > 100 and lines["closed"].any() and not lines["closed"].all()
    assert (first == np.concatenate([[0], np.cumsum(n)[:-1]])).all() and int(n.sum()) == verts.size and (n >= 1).all()
    last = first + n - 1
    assert (verts[first] == lines["head"]).all() and (verts[last] == lines["tail"]).all()
    assert (levels[lines["level_index"]] == lines["level"]).all()
    key = lines["head"].astype(np.int64) * 8 + lines["level_index"]
    assert (np.diff(key) > 0).all()                                 # numbered by ascending head
    closed = lines["closed"] == 1
    assert (np.minimum.reduceat(verts, first)[closed] == lines["head"][closed]).all()
    # 1: the vertices of a level are exactly its crossed edges, each once; so the lines are disjoint
    level_of = np.repeat(lines["level_index"], n)
    want = crossed_sets(z, levels.tolist())
    assert sum(w.size for w in want) == verts.size and st["launches"] > 0
    for l in range(levels.size):
        assert np.array_equal(np.sort(verts[level_of == l]), want[l]), l
    # 2: consecutive vertices, and tail to head of a closed line, are two sides of one void-free cell
    valid = z != cc.VOID
    cell_ok = valid[:-1, :-1] & valid[:-1, 1:] & valid[1:, :-1] & valid[1:, 1:]
    cells, inside = cells_of(verts, rows, cols, cell_ok)
    inner = np.ones(verts.size, bool)
    inner[last] = False                                             # the pairs (k, k + 1) inside one line
    k = np.flatnonzero(inner)
    assert share_a_cell(cells[k], cells[k + 1]).all()
    assert share_a_cell(cells[last[closed]], cells[first[closed]]).all()
    # 3: an open line's ends are sides of fewer than two void-free cells
    ends = np.concatenate([first[~closed], last[~closed]])
    assert ((cells[ends] >= 0).sum(axis=1) < 2).all()
    # 4: and where no cell of theirs has a void corner, they are border edges
    at_void = (inside[ends] & (cells[ends] < 0)).any(axis=1)
    e = verts[ends]
    i, j = (e >> 1) // cols, (e >> 1) % cols
    border = (((i == 0) | (i == rows - 1)) & (e & 1 == 0)) | (((j == 0) | (j == cols - 1)) & (e & 1 == 1))
    assert (at_void | border).all() and at_void.any() and border.any()

