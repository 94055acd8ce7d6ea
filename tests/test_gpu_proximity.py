"""The proximity maps and the reach of labelled regions on the MI355X (DESIGN.md sections 3.22 and 4.28): nearest, dist2 and
every reach field equal to the model's (tests/proximity_model.py) byte for byte, in the pruned and the brute variant, from host
and from device tables; ties, duplicates, extreme corners, scrambled positions, a wrapped polar window; every refusal; the launch
count; the render state; the tool.

The kernels take one lattice tile of 8 x 8 nodes per 64-lane workgroup, so the lattices here have whole tiles (64 x 64), one row
or one column of partial tiles (1 x 130, 130 x 1, 33 x 3), a corner tile of a single node (17 x 65) and several whole tiles with
a partial last column (96 x 130); there is no 256-lane block whose last part could be partial.  96 columns at stride 12 go once
round only on a DEM of 1152 columns, so the wrapped polar window is (22560, 0, 40, 96, 12, 1) of a 23040 x 1152 DEM: its last
row lies 0.1 degrees from the pole."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

import lattice_cases as lc
import model_cases as mc
import proximity_model as pm
import regions_cases as rc
from common import assert_bit_equal
from moonrtx_amd import _lib
from moonrtx_amd import regions as rg
from moonrtx_amd.renderer import DeviceBuffer, MoonRT, MoonRTError
from moonrtx_amd.scene import named_scene
from test_gpu_illumination import make

pytestmark = pytest.mark.gpu

NONE = 2 ** 64 - 1
CMAX = lc.CMAX
VARIANTS = ("prune", "brute")
POLAR = ((22560, 0, 40, 96, 12, 1), (23040, 1152))


@pytest.fixture(scope="module")
def rt(native_lib):
    """One context for the module, without a DEM, a light or a Moon frame: the stage needs none of them."""
    r = MoonRT(16, 16)
    yield r
    r.close()


# ---- positions and feature sets
def planar(rows, cols, a=3, b=2):
    """(j a, i b, 0): integer spacings, so equal distances abound."""
    i, j = np.mgrid[0:rows, 0:cols]
    return np.ascontiguousarray(np.stack([j * a, i * b, np.zeros_like(i)], -1), np.int32)


def scrambled(rows, cols, seed):
    """The planar positions dealt out at random over the nodes: the tiles' boxes prove nothing."""
    p = planar(rows, cols).reshape(-1, 3)
    return np.ascontiguousarray(p[np.random.default_rng(seed).permutation(rows * cols)].reshape(rows, cols, 3))


def sprinkle(rows, cols, share, seed):
    lab = np.where(np.random.default_rng(seed).random((rows, cols)) < share, 0, -1).astype(np.int32)
    return lab


def only(rows, cols, *nodes):
    lab = np.full(rows * cols, -1, np.int32)
    lab[list(nodes)] = 0
    return lab.reshape(rows, cols)


@functools.lru_cache(maxsize=None)
def expected(key):
    """The model's answer of a registered case, computed once and shared."""
    labels, pos, outside = CASES[key]
    near, d2 = pm.proximity(labels, pos, outside)
    near.setflags(write=False)
    d2.setflags(write=False)
    return near, d2


CASES = {}


def case(key, labels, pos, outside=False):
    labels = np.ascontiguousarray(labels, np.int32)
    pos = np.ascontiguousarray(pos, np.int32)
    labels.setflags(write=False)
    pos.setflags(write=False)
    CASES[key] = (labels, pos, outside)
    return key


def run(rt, labels, pos, outside=False, device=False, stats=None):
    """(nearest, dist2) through the facade, from host tables or from device tables."""
    to = "outside" if outside else "set"
    if not device:
        m = rt.proximity(labels, pos, to=to, stats=stats)
        return m.nearest, m.dist2
    lb, pb = DeviceBuffer(labels.nbytes), DeviceBuffer(pos.nbytes)
    try:
        lb.upload(labels)
        pb.upload(pos)
        m = rt.proximity(lb, pb, to=to, shape=labels.shape, stats=stats)
    finally:
        lb.free()
        pb.free()
    return m.nearest, m.dist2


def check(rt, monkeypatch, key, devices=(False,)):
    labels, pos, outside = CASES[key]
    want_near, want_d2 = expected(key)
    for variant in VARIANTS:
        monkeypatch.setenv("MOONRT_PROXIMITY", variant)
        for device in devices:
            near, d2 = run(rt, labels, pos, outside, device)
            what = f"{key}, {variant}, {'device' if device else 'host'} tables"
            assert near.dtype == np.int32 and d2.dtype == np.uint64 and near.shape == labels.shape == d2.shape
            assert near.tobytes() == want_near.tobytes(), what
            assert d2.tobytes() == want_d2.tobytes(), what


LATTICES = [(1, 1), (1, 130), (130, 1), (17, 65), (33, 3), (64, 64), (96, 130)]

for _r, _c in LATTICES:
    case(f"planar_{_r}x{_c}", sprinkle(_r, _c, 0.08, _r * 1000 + _c), planar(_r, _c))
    case(f"planar_{_r}x{_c}_outside", sprinkle(_r, _c, 0.9, _r * 1000 + _c + 1), planar(_r, _c), True)
    case(f"scrambled_{_r}x{_c}", sprinkle(_r, _c, 0.1, _r * 1000 + _c + 2), scrambled(_r, _c, _r + _c))


@pytest.mark.parametrize("shape", LATTICES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_planar_positions_ties_go_to_the_least_index(rt, monkeypatch, shape):
    r, c = shape
    main = shape in ((17, 65), (96, 130))
    check(rt, monkeypatch, f"planar_{r}x{c}", (False, True) if main else (False,))
    check(rt, monkeypatch, f"planar_{r}x{c}_outside")
    near, d2 = expected(f"planar_{r}x{c}")
    if r * c > 1:                                           # the case does hold ties: some node has two features at its d2
        labels, pos, _ = CASES[f"planar_{r}x{c}"]
        feat = np.flatnonzero(labels.reshape(-1) >= 0)
        p = pos.reshape(-1, 3).astype(np.int64)
        ties = 0
        for v in range(0, r * c, max(r * c // 200, 1)):
            ties += int((((p[feat] - p[v]) ** 2).sum(-1) == int(d2.reshape(-1)[v])).sum() > 1)
        assert ties > 0


@pytest.mark.parametrize("shape", LATTICES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_scrambled_positions(rt, monkeypatch, shape):
    check(rt, monkeypatch, f"scrambled_{shape[0]}x{shape[1]}", (False, True) if shape == (96, 130) else (False,))


case("equal_in_two_tiles", only(17, 65, 10 * 65 + 57, 14 * 65 + 55), planar(17, 65, 1, 1))


def test_an_equal_distance_in_a_later_tile_is_not_pruned(rt, monkeypatch):
    """Node (16, 64) is alone in the corner tile.  Features (14, 55) and (10, 57) both lie at d2 = 85 from it; the first is
    in the tile walked first, the second has the lower index and sits in a tile whose lower bound equals the tile's upper
    bound exactly: a prune on >= would lose it."""
    check(rt, monkeypatch, "equal_in_two_tiles", (False, True))
    near, d2 = expected("equal_in_two_tiles")
    assert near[16, 64] == 10 * 65 + 57 and d2[16, 64] == 85
    monkeypatch.setenv("MOONRT_PROXIMITY", "prune")
    got, _ = run(rt, *CASES["equal_in_two_tiles"][:2])
    assert got[16, 64] == 707


def polar_labels():
    lab = np.full((40, 96), -1, np.int32)
    lab[30:40, 44:53] = 0                                   # beside the pole, on the far side of column 0
    lab[0:4, 93:] = 1                                       # across the seam, 3.6 degrees from the pole
    lab[0:4, :3] = 1
    return lab


case("polar", polar_labels(), rg.node_positions(*POLAR))
case("polar_outside", polar_labels(), rg.node_positions(*POLAR), True)


def test_a_wrapped_polar_window(rt, monkeypatch):
    check(rt, monkeypatch, "polar", (False, True))
    check(rt, monkeypatch, "polar_outside")
    near, _ = expected("polar")
    # the nearest feature of the last row's column 0 lies across the pole, half the columns away
    assert 30 <= near[39, 0] // 96 and 44 <= near[39, 0] % 96 <= 52
    # and on either side of the seam: column 4 goes to column 2, column 88 to column 93
    assert near[1, 4] % 96 == 2 and near[1, 88] % 96 == 93 and near[1, 4] // 96 <= 3 and near[1, 88] // 96 <= 3


def corner_positions():
    """3 x 9: the eight corners of the cube of +-2^29, a second node on one of them, and small coordinates between."""
    pos = np.zeros((27, 3), np.int64)
    for k in range(8):
        pos[k] = [CMAX if k & 1 else -CMAX, CMAX if k & 2 else -CMAX, CMAX if k & 4 else -CMAX]
    pos[8] = pos[7]
    pos[9:] = np.random.default_rng(5).integers(-1000, 1001, (18, 3))
    return pos.reshape(3, 9, 3).astype(np.int32)


case("corners_one", only(3, 9, 0), corner_positions())
case("corners_small", only(3, 9, 13, 20), corner_positions())
case("corners_mixed", only(3, 9, 7, 2, 17), corner_positions())
case("corners_outside", only(3, 9, *range(1, 27)), corner_positions(), True)


def test_extreme_corners(rt, monkeypatch):
    for key in ("corners_one", "corners_small", "corners_mixed", "corners_outside"):
        check(rt, monkeypatch, key, (False, True))
    near, d2 = expected("corners_one")
    assert d2.reshape(-1)[7] == 3 * 2 ** 60 == d2.reshape(-1)[8] and d2.reshape(-1)[0] == 0 and (near == 0).all()


def duplicate_case():
    """20 x 20 planar positions in which whole blocks share one position; features among the twins."""
    pos = planar(20, 20, 1, 1)
    pos[5:9, 5:9] = pos[5, 5]
    pos[12:20, 10:20] = pos[0, 0]                           # twins of node 0, far away in the lattice
    pos[3, 17] = pos[18, 2]
    lab = np.full((20, 20), -1, np.int32)
    lab[6, 6] = lab[7, 7] = 0                               # both twins features: 6 * 20 + 6 takes the block
    lab[15, 15] = 1                                         # a twin of node 0, which is no feature
    lab[18, 2] = lab[3, 17] = 2                             # the lower-indexed twin (3, 17) takes (18, 2)
    return lab, pos


case("duplicates", *duplicate_case())
case("duplicates_outside", *duplicate_case(), True)
case("all_one_position", sprinkle(9, 17, 0.3, 4), np.full((9, 17, 3), 12345, np.int32))


def test_duplicate_positions(rt, monkeypatch):
    for key in ("duplicates", "duplicates_outside", "all_one_position"):
        check(rt, monkeypatch, key, (False, True))
    near, d2 = expected("duplicates")
    assert near[7, 7] == 6 * 20 + 6 and d2[7, 7] == 0 and near[18, 2] == 3 * 20 + 17 and near[0, 0] == 15 * 20 + 15 and d2[0, 0] == 0
    near, d2 = expected("all_one_position")
    assert (d2 == 0).all() and (near == near.reshape(-1)[0]).all()


SETS = []
for _r, _c in ((33, 3), (17, 65)):
    _n = _r * _c
    SETS += [case(f"none_{_r}x{_c}", np.full((_r, _c), -1), planar(_r, _c)),
             case(f"all_{_r}x{_c}", np.zeros((_r, _c)), planar(_r, _c)),
             case(f"none_outside_{_r}x{_c}", np.zeros((_r, _c)), planar(_r, _c), True),
             case(f"first_{_r}x{_c}", only(_r, _c, 0), planar(_r, _c)),
             case(f"last_{_r}x{_c}", only(_r, _c, _n - 1), planar(_r, _c)),
             case(f"last_tile_{_r}x{_c}", only(_r, _c, _n - 1, _n - 3 if _c == 3 else _n - 1), planar(_r, _c))]
SETS += [case("first_96x130", only(96, 130, 0), planar(96, 130)),
         case("last_96x130", only(96, 130, 96 * 130 - 1), planar(96, 130)),
         case("last_tile_96x130", only(96, 130, 89 * 130 + 128, 95 * 130 + 129, 92 * 130 + 129), planar(96, 130)),
         case("tenth_96x130", sprinkle(96, 130, 0.1, 77), planar(96, 130, 5, 7))]


@pytest.mark.parametrize("key", SETS)
def test_feature_sets(rt, monkeypatch, key):
    check(rt, monkeypatch, key, (False, True) if key == "tenth_96x130" else (False,))
    near, d2 = expected(key)
    if key.startswith("none"):
        assert (near == -1).all() and (d2 == np.uint64(NONE)).all()
    if key.startswith("all"):
        assert np.array_equal(near.reshape(-1), np.arange(near.size)) and (d2 == 0).all()


REGION_NAMES = ("1x40", "40x1", "33x65", "comb", "seam_ring", "seam_root_last")


@functools.lru_cache(maxsize=None)
def region_case(name):
    labels, n = rc.answer(rc.BY_NAME[name], 4)
    labels = np.array(labels, np.int32)
    pos = planar(*labels.shape, 2, 3)
    for outside in (False, True):
        case(f"regions_{name}_{int(outside)}", labels, pos, outside)
    return labels, int(n), pos


def assert_reach_equal(got, want, what):
    assert got.dtype == rg.REACH_DTYPE and got.shape == want.shape, what
    for f in rg.REACH_DTYPE.names:
        assert got[f].tobytes() == want[f].tobytes(), (what, f, got[f], want[f])


@pytest.mark.parametrize("name", REGION_NAMES)
def test_both_modes_and_the_reach_on_region_labels(rt, monkeypatch, name):
    labels, n, pos = region_case(name)
    for outside in (False, True):
        key = f"regions_{name}_{int(outside)}"
        check(rt, monkeypatch, key, (False, True) if name == "33x65" else (False,))
        near, d2 = expected(key)
        # n + 2 regions: the last two numbers are carried by no node
        got = rt.region_reach(labels, n + 2, rg.ProximityMap(near, d2))
        assert_reach_equal(got, pm.reach(labels, n + 2, d2, near), key)
        assert (got["count"][n:] == 0).all() and (got["max_at"][n:] == -1).all() and (got["d2_min"][n:] == np.uint64(NONE)).all()
    # the inscribed circle through the facade: the to="outside" distances of the regions' own labels
    m = rg.RegionMap(labels, np.zeros(n, rg.REGION_DTYPE))
    radius, centre = m.inscribed(rt, pos, unit_m=0.5)
    near, d2 = expected(f"regions_{name}_1")
    want = pm.reach(labels, n, d2, near)
    assert np.array_equal(centre, want["max_at"])
    assert np.array_equal(radius, np.where(want["d2_max"] == np.uint64(NONE), np.inf, np.sqrt(want["d2_max"].astype(np.float64)) * 0.5))


def reach_call(rt, rows, cols, *args, **kw):
    return lc.reach_call(rt._lib, rt._ctx, rows, cols, *args, **kw)


def test_the_reach_from_device_tables_and_on_a_caller_s_table(rt):
    labels = np.random.default_rng(9).integers(-1, 6, (37, 70)).astype(np.int32)
    labels[labels == 3] = -1                                # number 3 has no node; the others are scattered
    d2 = np.random.default_rng(10).integers(0, 40, (37, 70)).astype(np.uint64) * np.uint64(2 ** 57)      # many equal extremes
    near = np.random.default_rng(11).integers(-1, 37 * 70, (37, 70)).astype(np.int32)
    want = pm.reach(labels, 6, d2, near)
    assert_reach_equal(rt.region_reach(labels, 6, (d2, near)), want, "host tables")
    bufs = [DeviceBuffer(a.nbytes) for a in (labels, d2, near)] + [DeviceBuffer(32 * 6)]
    try:
        for b, a in zip(bufs, (labels, d2, near)):
            b.upload(a)
        assert reach_call(rt, 37, 70, n=6, dev_labels=bufs[0].ptr, dev_d2=bufs[1].ptr, dev_near=bufs[2].ptr, dev_out=bufs[3].ptr) == 0
        assert_reach_equal(bufs[3].download(rg.REACH_DTYPE, (6,)), want, "device tables")
        # a mix: labels on the device, the map on the host
        assert_reach_equal(rt.region_reach(bufs[0], 6, (d2, near), shape=(37, 70)), want, "mixed tables")
    finally:
        for b in bufs:
            b.free()
    # one region over every node of whole waves and of a partial one; dist2 of UINT64_MAX everywhere
    for shape in ((8, 64), (5, 77)):
        lab = np.zeros(shape, np.int32)
        far = np.full(shape, NONE, np.uint64)
        none = np.full(shape, -1, np.int32)
        got = rt.region_reach(lab, 2, (far, none))
        assert_reach_equal(got, pm.reach(lab, 2, far, none), "no feature anywhere")
        assert got[0].tolist() == (NONE, NONE, 0, 0, -1, shape[0] * shape[1]) and got[1].tolist() == (0, NONE, -1, -1, -1, 0)
        ramp = np.arange(lab.size, dtype=np.uint64).reshape(shape) // np.uint64(3)
        ids = np.arange(lab.size, dtype=np.int32).reshape(shape)[::-1].copy()
        assert_reach_equal(rt.region_reach(lab, 1, (ramp, ids)), pm.reach(lab, 1, ramp, ids), "a ramp")


def test_the_reach_refuses_a_bad_label_table_after_the_launch(rt):
    labels = np.array(rc.answer(rc.BY_NAME["33x65"], 4)[0], np.int32)
    n = int(rc.answer(rc.BY_NAME["33x65"], 4)[1])
    d2 = np.ones(labels.shape, np.uint64)
    near = np.zeros(labels.shape, np.int32)
    out = np.zeros(n, rg.REACH_DTYPE)
    for bad in (n, n + 1000, 2 ** 31 - 1, -2, -2 ** 31):
        mine = labels.copy()
        mine[17, 23] = bad
        assert reach_call(rt, 33, 65, mine, n, d2, near, out) == -1, bad
        assert "1 entries outside -1" in rt._lib.mrtx_last_error(rt._ctx).decode()
        with pytest.raises(MoonRTError, match="entries outside -1"):
            rt.region_reach(mine, n, (d2, near))
    # no regions: the table is checked, nothing is written
    none = np.full((5, 5), -1, np.int32)
    st = _lib.MrtxStats()
    mark = np.full(1, 0x5A, np.uint8).repeat(32).view(rg.REACH_DTYPE)
    assert reach_call(rt, 5, 5, none, 0, np.zeros((5, 5), np.uint64), none, mark, st=st) == 0 and st.launches == 1
    assert (mark.view(np.uint8) == 0x5A).all()
    assert rt.region_reach(none, 0, (np.zeros((5, 5), np.uint64), none)).shape == (0,)
    one = none.copy()
    one[2, 2] = 0
    with pytest.raises(MoonRTError, match="entries outside -1"):
        rt.region_reach(one, 0, (np.zeros((5, 5), np.uint64), none))
    assert rt._lib.mrtx_last_error(rt._ctx).decode() != ""
    # and the context goes on
    assert_reach_equal(rt.region_reach(labels, n, (d2, near)), pm.reach(labels, n, d2, near), "afterwards")


def prox_call(rt, **kw):
    return lc.prox_call(rt._lib, rt._ctx, **kw)


def test_every_refusal(rt, monkeypatch):
    pos, labels = planar(8, 9), sprinkle(8, 9, 0.3, 1)
    near, d2 = np.zeros((8, 9), np.int32), np.zeros((8, 9), np.uint64)
    dev = DeviceBuffer(8192)
    dev.upload(np.zeros(2048, np.int32))
    base = dict(pos=pos, labels=labels, near=near, d2=d2)
    D = lc.prox_device_tables(dev.ptr)
    off = lc.prox_off_positions(pos)
    try:
        for text, kw in lc.prox_refusals(pos, labels, near, d2, dev.ptr):
            lc.refused(rt._lib, rt._ctx, prox_call(rt, **kw), text)
            assert (near == 0).all() and (d2 == 0).all(), text
        # an unknown value of the switch is refused by name
        monkeypatch.setenv("MOONRT_PROXIMITY", "fast")
        assert prox_call(rt, **base) == -1 and "MOONRT_PROXIMITY" in rt._lib.mrtx_last_error(rt._ctx).decode()
        monkeypatch.delenv("MOONRT_PROXIMITY")
        # a device table's coordinates are checked in the kernel: refused after the launch, in both variants
        dev.upload(off, 0)
        dev.upload(labels, 1024)
        for variant in VARIANTS:
            monkeypatch.setenv("MOONRT_PROXIMITY", variant)
            assert prox_call(rt, **D) == -1
            assert re.search("1 coordinates of the device position table lie outside", rt._lib.mrtx_last_error(rt._ctx).decode())
        monkeypatch.delenv("MOONRT_PROXIMITY")
        # the facade checks a host table itself
        with pytest.raises(ValueError, match="larger unit"):
            rt.proximity(labels, off.astype(np.int64))
        # the reach's own refusals
        out = np.zeros(4, rg.REACH_DTYPE)
        for text, kw in lc.reach_refusals(labels, d2, near, out, dev.ptr):
            lc.refused(rt._lib, rt._ctx, reach_call(rt, **kw), text)
            assert (out.view(np.uint8) == 0).all(), text
        # the context still works
        want = pm.proximity(labels, pos)
        got = run(rt, labels, pos)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    finally:
        dev.free()


def test_launches_and_pairs_do_not_depend_on_the_run_or_the_data(rt, monkeypatch):
    pos = planar(96, 130)
    sets = [sprinkle(96, 130, 0.1, 77), only(96, 130, 5000), np.full((96, 130), -1, np.int32), np.zeros((96, 130), np.int32)]
    for variant in VARIANTS:
        monkeypatch.setenv("MOONRT_PROXIMITY", variant)
        launches = []
        for k, lab in enumerate(sets):
            seen = []
            for _ in range(2):
                st = {}
                rt.proximity(lab, pos, stats=st)
                assert st["launches"] > 0 and st["kernel_ms"] > 0.0
                seen.append((st["launches"], st["pairs"]))
            assert seen[0] == seen[1], (variant, seen)
            launches.append(seen[0][0])
            if variant == "brute":
                assert seen[0][1] == 96 * 130 * int((lab >= 0).sum())
            elif k == 2:
                assert seen[0][1] == 0
        assert len(set(launches)) == 1, (variant, launches)
    st = {}
    rt.region_reach(sets[0], 3, rt.proximity(sets[0], pos), stats=st)
    a = st["launches"]
    st = {}
    rt.region_reach(sets[3], 3, rt.proximity(sets[1], pos), stats=st)
    assert a == st["launches"] > 0


def test_leaves_the_render_state_alone(native_lib):
    s = named_scene("S1", 16, 16).with_size(48, 32, spp_per_launch=16)
    dem = mc.crater_dem()
    labels, pos, _ = CASES["planar_17x65"]

    def go(with_stage):
        r = make(s, dem, _lib.F_COUNT_STATS)
        st1 = r.render(1)
        if with_stage:
            near, d2 = run(r, labels, pos)
            want = expected("planar_17x65")
            assert near.tobytes() == want[0].tobytes() and d2.tobytes() == want[1].tobytes()
            run(r, labels, pos, True, True)
            assert_reach_equal(r.region_reach(labels, 1, (d2, near)), pm.reach(labels, 1, d2, near), "between two renders")
        st2 = r.render(1)
        out = r.read_linear(), r.read_hits(), r.samples_done(), st1, st2
        r.close()
        return out
    a, b = go(False), go(True)
    assert_bit_equal(b[0], a[0], "linear radiance")
    assert_bit_equal(b[1], a[1], "hit buffer")
    assert b[2] == a[2] == 32
    for k in ("primary_hits", "shadow_rays", "height_samples", "bounce_rays"):
        assert b[4][k] == a[4][k], k


def test_scale_prune_agrees_with_brute_and_evaluates_fewer_pairs(rt, monkeypatch):
    """256 x 256 nodes of a wrapped polar window with compact blobs, too large for the model."""
    pos = rg.node_positions((22560 - 216 * 12, 0, 256, 256, 12, 1), (23040, 3072))
    i, j = np.mgrid[0:256, 0:256]
    lab = np.full((256, 256), -1, np.int32)
    for k, (ci, cj, rad) in enumerate(((40, 250, 9), (200, 30, 14), (120, 128, 11), (250, 100, 6), (10, 60, 12), (90, 200, 16))):
        dj = (j - cj + 128) % 256 - 128
        lab[(i - ci) ** 2 + dj ** 2 <= rad ** 2] = k
    got = {}
    for variant in VARIANTS:
        monkeypatch.setenv("MOONRT_PROXIMITY", variant)
        st = {}
        m = rt.proximity(lab, pos, stats=st)
        got[variant] = (m.nearest, m.dist2, st["pairs"])
    assert got["prune"][0].tobytes() == got["brute"][0].tobytes() and got["prune"][1].tobytes() == got["brute"][1].tobytes()
    assert got["brute"][2] == 65536 * int((lab >= 0).sum())
    assert 0 < got["prune"][2] < got["brute"][2]
    # a spot check by hand of the model's rule on a few nodes
    feat = np.flatnonzero(lab.reshape(-1) >= 0)
    p = pos.reshape(-1, 3).astype(np.int64)
    for v in (0, 255, 32767, 40000, 65535):
        d = ((p[feat] - p[v]) ** 2).sum(-1)
        assert got["prune"][0].reshape(-1)[v] == feat[np.argmin(d)] and got["prune"][1].reshape(-1)[v] == d.min()


def test_the_proximity_tool(native_lib, tmp_path):
    """tools/proximity_map.py on a saved map: the map, the buffer and the CSV's inscribed radius and closest approach are
    the model's."""
    import csv
    import os
    import subprocess
    import sys
    rows, cols = 40, 96
    window, dem_hw = POLAR
    cold = np.ones((rows, cols, 2), np.float32)
    cold[30:40, 44:53, 1] = 0.0
    cold[2:9, 90:, 1] = 0.0
    cold[2:9, :5, 1] = 0.0
    lit = np.zeros((rows, cols), np.float32)
    lit[20:23, 10:14] = 1.0
    np.save(tmp_path / "cold.npy", cold)
    np.save(tmp_path / "lit.npy", lit)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "tools", "proximity_map.py"), "--map", str(tmp_path / "cold.npy"), "--channel", "1",
           "--below", "0.5", "--window", *[str(v) for v in window], "--dem-size", *[str(v) for v in dem_hw],
           "--out", str(tmp_path / "prox.npy"), "--buffer", "20000", "--buffer-out", str(tmp_path / "mask.npy"),
           "--to-map", str(tmp_path / "lit.npy"), "--to-above", "0.8", "--csv", str(tmp_path / "regions.csv")]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    import regions_model as model
    labels, n = model.label((cold[:, :, 1] <= 0.5).astype(np.uint8), 4, True)
    assert n == 2
    pos = rg.node_positions(window, dem_hw)
    near, d2 = pm.proximity(labels, pos)
    out = np.load(tmp_path / "prox.npy")
    assert out.shape == (rows, cols, 3)
    assert np.array_equal(out[:, :, 0], np.sqrt(d2.astype(np.float64)) * 0.01) and np.array_equal(out[:, :, 1], near)
    assert np.array_equal(out[:, :, 2], labels.reshape(-1)[near])
    assert np.array_equal(np.load(tmp_path / "mask.npy"), d2 <= np.uint64(int((20000 / 0.01) ** 2)))
    inner = pm.reach(labels, n, *pm.proximity(labels, pos, True)[::-1])
    second = np.where(lit >= 0.8, 0, -1)
    near2, d22 = pm.proximity(second, pos)
    appr = pm.reach(labels, n, d22, near2)
    with open(tmp_path / "regions.csv") as f:
        lines = list(csv.reader(f))
    assert len(lines) == 1 + n
    for line in lines[1:]:
        rec = dict(zip(lines[0], line))
        r = int(rec["region"])
        assert float(rec["inscribed_radius_m"]) == float(np.sqrt(np.float64(inner[r]["d2_max"])) * 0.01)
        assert int(rec["centre_node"]) == int(inner[r]["max_at"])
        i, j = divmod(int(inner[r]["max_at"]), cols)
        assert float(rec["centre_lat"]) == 90.0 - (window[0] + i * 12 + 0.5) * (180.0 / dem_hw[0])
        assert float(rec["centre_lon"]) == -180.0 + ((j * 12) % dem_hw[1] + 0.5) * (360.0 / dem_hw[1])
        assert float(rec["approach_m"]) == float(np.sqrt(np.float64(appr[r]["d2_min"])) * 0.01)
        assert int(rec["from_node"]) == int(appr[r]["min_at"]) and int(rec["to_node"]) == int(appr[r]["min_nearest"])
        assert lit.reshape(-1)[int(rec["to_node"])] == 1.0 and labels.reshape(-1)[int(rec["from_node"])] == r
