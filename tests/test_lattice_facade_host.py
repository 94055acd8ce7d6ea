"""The lattice methods of MoonRT (moonrtx_amd/lattice_calls.py) without a GPU, through the fake library of fake_moonrt.py on
3 x 4 lattices: the host call and the DeviceBuffer call of each method return equal arrays from equal outputs and use the same
pointer positions, each on its own side; the two-call methods size their tables by the counts of the first call; every
DeviceBuffer a method makes is freed, whether it returns or a call is refused; and the refusals made in Python keep their
texts."""
import numpy as np
import pytest

from fake_moonrt import SPEC, FakeLib
from moonrtx_amd import _lib
from moonrtx_amd import basins as bs
from moonrtx_amd import regions as rg
from moonrtx_amd.renderer import DeviceBuffer, MoonRT, MoonRTError

R, CO = 3, 4
RNG = np.random.default_rng(36)
LAB = RNG.integers(-1, 3, (R, CO)).astype(np.int32)
FIELD = RNG.normal(size=(R, CO, 2)).astype(np.float32)
MASK = RNG.integers(0, 2, (R, CO)).astype(np.uint8)
POS = RNG.integers(-50, 50, (R, CO, 3)).astype(np.int32)
Z = RNG.integers(-9, 9, (R, CO)).astype(np.int32)
FILL = np.maximum(Z, 0).astype(np.int32)
OUTLETS = RNG.integers(0, 2, (R, CO)).astype(np.uint8)
D2 = RNG.integers(0, 99, (R, CO)).astype(np.uint64)
WEIGHTS, EW, NS = np.arange(R) + 1, np.arange(R) + 2, np.arange(R + 1) + 3
LEVELS = np.array([-2, 0, 3])


@pytest.fixture
def fake(monkeypatch):
    lib = FakeLib()
    monkeypatch.setattr(_lib, "load", lambda: lib)
    monkeypatch.setattr(DeviceBuffer, "__del__", lambda self: None)         # only a free the code asks for counts as one
    return lib


def dev(array):
    b = DeviceBuffer(array.nbytes)
    b.upload(array)
    return b


# method: (the call on host tables, the call on DeviceBuffers, the counts the library reports, its entry points in call
# order, the pointer pairs that stay on the host in the DeviceBuffer call: host-only inputs and region_reach's tables)
CASES = {
    "regions": (lambda rt: rt.regions(field=FIELD, channel=1, row_weights=WEIGHTS),
                lambda rt: rt.regions(field=dev(FIELD), shape=(R, CO, 2), channel=1, row_weights=WEIGHTS),
                {"n_regions": 2}, ["mrtx_regions_label", "mrtx_regions_stats"], ()),
    "region_statistics": (lambda rt: rt.region_statistics(LAB, 3, FIELD, row_weights=WEIGHTS, hist=(1, 4, -1.0, 1.0)),
                          lambda rt: rt.region_statistics(dev(LAB), 3, dev(FIELD), row_weights=WEIGHTS, hist=(1, 4, -1.0, 1.0), shape=(R, CO, 2)),
                          {}, ["mrtx_regions_zonal"], ()),
    "region_shapes": (lambda rt: rt.region_shapes(LAB, 3, side_ew=EW, side_ns=NS),
                      lambda rt: rt.region_shapes(dev(LAB), 3, side_ew=EW, side_ns=NS, shape=(R, CO)), {}, ["mrtx_regions_shape"], ()),
    "proximity": (lambda rt: rt.proximity(LAB, POS, to="outside"), lambda rt: rt.proximity(dev(LAB), dev(POS), to="outside", shape=(R, CO)),
                  {"pairs": 5}, ["mrtx_proximity"], ()),
    "region_reach": (lambda rt: rt.region_reach(LAB, 3, (D2, LAB)), lambda rt: rt.region_reach(dev(LAB), 3, (D2, LAB), shape=(R, CO)),
                     {}, ["mrtx_regions_reach"], ("d2_d d2_h", "near_d near_h", "rec_d rec_h")),
    "region_outlines": (lambda rt: rt.region_outlines(LAB, 3, row_weights=WEIGHTS), lambda rt: rt.region_outlines(dev(LAB), 3, row_weights=WEIGHTS, shape=(R, CO)),
                        {"rings": 2, "vertices": 5}, ["mrtx_regions_outline"] * 2, ()),
    "contours": (lambda rt: rt.contours(Z, LEVELS), lambda rt: rt.contours(dev(Z), LEVELS, shape=(R, CO)),
                 {"lines": 2, "vertices": 3}, ["mrtx_contours"] * 2, ()),
    "fill_depressions": (lambda rt: rt.fill_depressions(Z, outlets=OUTLETS), lambda rt: rt.fill_depressions(dev(Z), outlets=OUTLETS, shape=(R, CO)),
                         {"visits": 4}, ["mrtx_fill"], ("out_d out_h",)),
    "basins": (lambda rt: rt.basins(LAB, 3, (Z, FILL), row_weights=WEIGHTS), lambda rt: rt.basins(dev(LAB), 3, (dev(Z), dev(FILL)), row_weights=WEIGHTS, shape=(R, CO)),
               {}, ["mrtx_fill_basins"], ()),
    "bowls": (lambda rt: rt.bowls(Z, outlets=OUTLETS, row_weights=WEIGHTS), lambda rt: rt.bowls(dev(Z), outlets=OUTLETS, row_weights=WEIGHTS, shape=(R, CO)),
              {"bowls": 3, "rounds": 2}, ["mrtx_bowls"] * 2, ("out_d out_h",)),
}
# the count-sized tables of the two-call methods: (capacity argument, script key, the table's pair, bytes per record)
COUNTED = {
    "regions": [("n", "n_regions", "rec_d rec_h", 56)],
    "region_outlines": [("cap_r", "rings", "ring_d ring_h", 48), ("cap_v", "vertices", "vert_d vert_h", 8)],
    "contours": [("cap_l", "lines", "line_d line_h", 32), ("cap_v", "vertices", "vert_d vert_h", 4)],
    "bowls": [("cap", "bowls", "rec_d rec_h", 64)],
}


def arrays(x):
    """Every array of a method's result, in a fixed order."""
    if isinstance(x, np.ndarray):
        return [x]
    if isinstance(x, (tuple, list)):
        return [a for v in x for a in arrays(v)]
    return [a for _, v in sorted(vars(x).items()) for a in arrays(v)] if hasattr(x, "__dict__") else []


def result_of(fake, call, script=None, refuse=()):
    """The arrays one method call returns, on a fresh record."""
    fake.reset()
    fake.script, fake.refuse = dict(script or {}), set(refuse)
    return arrays(call(MoonRT(4, 4)))


def inputs(fake):
    """The allocations that were uploaded to: the inputs of the test itself, which the method must not free."""
    return sorted({int(e[1][3:].split("+")[0]) for e in fake.log if e[0] == "upload"})


def side(value):
    return value.split()[0].rstrip("+0123456789")


@pytest.mark.parametrize("method", sorted(CASES))
def test_host_and_device_calls_agree(fake, method):
    host_call, dev_call, script, names, stay = CASES[method]
    host = result_of(fake, host_call, script)
    host_calls = fake.calls()
    assert [n for n, _ in host_calls] == names and not fake.allocs
    device = result_of(fake, dev_call, script)
    dev_calls = fake.calls()
    assert [n for n, _ in dev_calls] == names
    assert len(host) == len(device) and len(host) > 0
    for h, d in zip(host, device):
        assert h.dtype == d.dtype and h.shape == d.shape and h.tobytes() == d.tobytes()
    for (name, ha), (_, da) in zip(host_calls, dev_calls):
        assert {k: v for k, v in ha.items() if not isinstance(v, str)} == {k: v for k, v in da.items() if not isinstance(v, str)}      # scalars, structs
        for key in list(SPEC[name][1]) + list(SPEC[name][2]):
            if " " not in key:          # a host-only table: the same on both sides
                assert side(ha[key]) == side(da[key]) != "dev"
                continue
            d, h = key.split()
            assert side(ha[d]) == "null"
            if key in stay:
                assert (side(da[d]), side(da[h])) == ("null", side(ha[h]))
            else:
                assert side(da[h]) == "null" and (side(da[d]) == "dev") == (side(ha[h]) == "host")
    assert fake.live() == inputs(fake)


@pytest.mark.parametrize("method", sorted(COUNTED))
@pytest.mark.parametrize("empty", [False, True])
def test_second_call_takes_the_counts_of_the_first(fake, method, empty):
    host_call, dev_call, script, names, _ = CASES[method]
    script = {k: 0 if empty and k != "rounds" else v for k, v in script.items()}
    for call in (host_call, dev_call):
        result = result_of(fake, call, script)
        first, second = (a for _, a in fake.calls())
        made = {f"dev{e[1]}": e[2] for e in fake.log if e[0] == "alloc"}
        for cap, key, pair, record in COUNTED[method]:
            assert second[cap] == script[key]
            if method != "regions":
                assert first[cap] == 0 and [side(first[p]) for p in pair.split()] == ["null", "null"]
            d, h = pair.split()
            if call is dev_call:        # exactly the count's records, one where there are none
                assert made[second[d].split("+")[0]] == max(record * script[key], record) and side(second[h]) == "null"
            else:
                assert side(second[h]) == "host" and side(second[d]) == "null"
        if empty:                   # one record was there to write to, and none is returned
            assert sum(a.ndim > 0 and a.shape[0] == 0 for a in result) >= len(COUNTED[method])
            assert all(a.shape[0] == 0 for a in result if a.dtype.names is not None)


@pytest.mark.parametrize("method", sorted(CASES))
def test_device_tables_are_freed_on_every_exit(fake, method):
    _, dev_call, script, names, _ = CASES[method]
    result_of(fake, dev_call, script)
    made = len(fake.allocs) - len(inputs(fake))
    assert fake.live() == inputs(fake) and (made > 0 or method == "region_reach")
    seen = {}
    for name in names:              # refuse each call of the method in turn
        k = seen.get(name, 0)
        seen[name] = k + 1
        with pytest.raises(MoonRTError, match="refused by the script"):
            result_of(fake, dev_call, script, refuse=[(name, k)])
        assert fake.live() == inputs(fake)
        assert [n for n, _ in fake.calls()] == names[:names.index(name) + k + 1]


def test_host_only_inputs_go_to_the_device_call_unchanged(fake):
    """row_weights, side tables and host outlets are host pointers with the same bytes, whichever side the tables are on."""
    for method, keys in (("regions", ["w"]), ("region_statistics", ["w"]), ("region_shapes", ["ew", "ns"]), ("region_outlines", ["w"]),
                         ("fill_depressions", ["out_h"]), ("basins", ["w"]), ("bowls", ["w", "out_h"])):
        host_call, dev_call, script = CASES[method][:3]
        result_of(fake, host_call, script)
        host_args = fake.calls()[-1][1]
        result_of(fake, dev_call, script)
        for key in keys:
            assert fake.calls()[-1][1][key] == host_args[key] and host_args[key].startswith("host crc ")
    fake.reset()
    z, o = dev(Z), dev(OUTLETS)
    MoonRT(4, 4).bowls(z, outlets=o, shape=(R, CO))
    assert [(side(a["out_d"]), a["out_h"]) for _, a in fake.calls("mrtx_bowls")] == [("dev", "null")] * 2


REFUSALS = [
    (lambda rt: rt.regions(field=FIELD, mask=MASK), "give exactly one of field and mask"),
    (lambda rt: rt.regions(), "give exactly one of field and mask"),
    (lambda rt: rt.regions(field=dev(FIELD)), "a DeviceBuffer needs shape = (rows, cols[, n_ch])"),
    (lambda rt: rt.regions(mask=dev(MASK), shape=(R + 1, CO)), "the DeviceBuffer is smaller than its shape"),
    (lambda rt: rt.regions(mask=MASK, row_weights=[1, 2, 2 ** 32]), "row_weights must be (rows,) integers in 0 .. 2^32 - 1"),
    (lambda rt: rt.regions(mask=MASK, row_weights=[1, 2]), "row_weights must be (rows,) integers in 0 .. 2^32 - 1"),
    (lambda rt: rt.region_statistics(LAB, 3, dev(FIELD), shape=(R, CO, 2)), "labels and field must both be numpy arrays or both DeviceBuffers"),
    (lambda rt: rt.region_statistics(dev(LAB), 3, dev(FIELD)), "DeviceBuffers need shape = (rows, cols, n_ch)"),
    (lambda rt: rt.region_statistics(dev(LAB), 3, dev(FIELD), shape=(R, CO, 3)), "the field DeviceBuffer is smaller than its shape"),
    (lambda rt: rt.region_statistics(dev(LAB), 3, dev(FIELD), shape=(R + 1, CO, 1)), "the label DeviceBuffer is smaller than its shape"),
    (lambda rt: rt.region_statistics(LAB, 3, FIELD, row_weights=[-1, 0, 1]), "row_weights must be (3,) integers in 0 .. 2^32 - 1"),
    (lambda rt: rt.region_statistics(LAB, 3, FIELD, hist=(0, 0, 0.0, 1.0)), "hist = (channel, n_bins >= 1, lo, hi > lo)"),
    (lambda rt: rt.region_statistics(LAB, 3, FIELD, hist=(0, 4, 1.0, 1.0)), "hist = (channel, n_bins >= 1, lo, hi > lo)"),
    (lambda rt: rt.region_shapes(LAB, 3, side_ew=EW), "give both of side_ew and side_ns or neither"),
    (lambda rt: rt.region_shapes(dev(LAB), 3, side_ns=NS, shape=(R, CO)), "give both of side_ew and side_ns or neither"),
    (lambda rt: rt.region_shapes(dev(LAB), 3), "a DeviceBuffer needs shape = (rows, cols)"),
    (lambda rt: rt.proximity(dev(LAB), POS, shape=(R, CO)), "labels and positions must both be numpy arrays or both DeviceBuffers"),
    (lambda rt: rt.proximity(dev(LAB), dev(POS[:, :, :2]), shape=(R, CO)), "the position DeviceBuffer is smaller than its shape"),
    (lambda rt: rt.proximity(LAB, np.full((R, CO, 3), 2 ** 29 + 1)), "a coordinate leaves +-2^29: choose a larger unit"),
    (lambda rt: rt.proximity(LAB, np.full((R, CO, 3), -2 ** 29 - 1)), "a coordinate leaves +-2^29: choose a larger unit"),
    (lambda rt: rt.region_outlines(dev(LAB), 3), "a DeviceBuffer needs shape = (rows, cols)"),
    (lambda rt: rt.region_outlines(LAB, 3, row_weights=np.ones(R)), "row_weights must be (3,) integers in 0 .. 2^32 - 1"),
    (lambda rt: rt.contours(dev(Z), LEVELS), "a DeviceBuffer needs shape = (rows, cols)"),
    (lambda rt: rt.contours(dev(Z), LEVELS, shape=(R, CO + 1)), "the z DeviceBuffer is smaller than its shape"),
    (lambda rt: rt.contours(Z, []), "levels must be 1 .. 65536 integers"),
    (lambda rt: rt.contours(Z, [0.5, 1.5]), "levels must be 1 .. 65536 integers"),
    (lambda rt: rt.contours(Z, [0, 2 ** 31]), "levels leave int32"),
    (lambda rt: rt.fill_depressions(dev(Z)), "a DeviceBuffer needs shape = (rows, cols)"),
    (lambda rt: rt.fill_depressions(dev(Z), shape=(R, CO + 1)), "the heights DeviceBuffer is smaller than its shape"),
    (lambda rt: rt.fill_depressions(Z, outlets=dev(OUTLETS[1:])), "the outlet DeviceBuffer is smaller than its shape"),
    (lambda rt: rt.basins(LAB, 3, (dev(Z[1:]), FILL)), "the heights DeviceBuffer is smaller than its shape"),
    (lambda rt: rt.basins(LAB, 3, (Z, FILL), row_weights=[1, 2, 2 ** 32]), "row_weights must be (3,) integers in 0 .. 2^32 - 1"),
    (lambda rt: rt.bowls(dev(Z)), "a DeviceBuffer needs shape = (rows, cols)"),
    (lambda rt: rt.bowls(dev(Z), shape=(R + 1, CO)), "the heights DeviceBuffer is smaller than its shape"),
    (lambda rt: rt.bowls(Z, row_weights=[1.0, 2.0, 3.0]), "row_weights must be (3,) integers in 0 .. 2^32 - 1"),
]


@pytest.mark.parametrize("k", range(len(REFUSALS)))
def test_python_side_refusals_keep_their_texts(fake, k):
    call, text = REFUSALS[k]
    with pytest.raises(ValueError) as e:
        call(MoonRT(4, 4))
    assert str(e.value) == text
    assert not fake.calls()             # refused before any library call


def test_result_classes(fake):
    """The methods still hand their tables to the result classes: one of each."""
    rt = MoonRT(4, 4)
    fake.script = {"n_regions": 2, "rings": 2, "vertices": 5, "bowls": 3}
    assert isinstance(rt.regions(mask=MASK), rg.RegionMap) and isinstance(rt.proximity(LAB, POS), rg.ProximityMap)
    assert isinstance(rt.region_outlines(dev(LAB), 3, shape=(R, CO)), rg.Outlines)
    assert isinstance(rt.fill_depressions(dev(Z), shape=(R, CO)), bs.FillMap) and isinstance(rt.peaks(Z), bs.BowlTree)
