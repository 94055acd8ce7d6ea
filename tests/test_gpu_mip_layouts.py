"""The five device structures every march trusts, downloaded and compared BIT FOR BIT with their numpy
model (tests/mip_model.py) on ragged DEMs, and held to the covering invariants their consumers rely on: the padded row-pair
DEM, the colour row pairs, the max-mip in row pairs, the medium max-mip, the horizon mip.  No tolerance anywhere: they are
copies and maxima."""
import numpy as np
import pytest

import mip_model as mm
from common import assert_bit_equal
from moonrtx_amd import _lib
from moonrtx_amd.renderer import MoonRT, MoonRTError
from moonrtx_amd.scene import named_scene

pytestmark = pytest.mark.gpu

SMALL = [(2, 2), (3, 5), (16, 32), (17, 33), (31, 47), (64, 129)]
MIPS = (_lib.BUF_MIP, _lib.BUF_MIP2, _lib.BUF_HMIP)


def context(D, T, step=None):
    s = named_scene("S1", 16, 16)
    rt = MoonRT(s.width, s.height)
    rt.upload_dem(D)
    rt.upload_color(T)
    rt.apply_scene(s)
    if step is not None:
        rt.set_params(marching_step=step)
    return rt, s


def march(rt):
    """The cheapest marching call: one point, one Sun sample.  It builds the structures for the step in force."""
    rt.illumination_at(10.0, 20.0, n_sun=1)


def check_structures(rt, s, D, T):
    """mip_info against the float64 rule, the five structures against the model bit for bit, the invariants on what was
    downloaded.  Returns mip_info."""
    h, w = D.shape
    step = float(rt.params.marching_step)
    info = rt.mip_info()
    assert tuple(info[k] for k in MoonRT.MIP_INFO) == mm.mip_info(h, w, s.radius, step), (D.shape, step, info)
    shift, m2, hs = info["mip_shift"], info["m2_shift"], info["hm_shift"]
    want = mm.build_all(D, T, shift, m2)
    got = {"dem": rt.read_structure(_lib.BUF_DEM), "color": rt.read_structure(_lib.BUF_COLOR),
           "mip": rt.read_structure(_lib.BUF_MIP), "mip2": rt.read_structure(_lib.BUF_MIP2),
           "hmip": rt.read_structure(_lib.BUF_HMIP)}
    for k in ("dem", "color", "mip", "mip2", "hmip"):
        assert got[k] is not None and got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (k, D.shape, shift)
        assert_bit_equal(got[k], want[k], f"{k} of the {h} x {w} DEM at shift {shift}")
    # the byte counts of the contract: the row-pair mip without its slack element
    assert rt.device_ptr(_lib.BUF_DEM)[1] == (h + 4) * (w + 4) * 8
    assert rt.device_ptr(_lib.BUF_MIP)[1] == (info["mip_h"] + 2) * (info["mip_w"] + 2) * 8
    assert rt.device_ptr(_lib.BUF_MIP2)[1] == (info["m2_h"] + 2) * (info["m2_w"] + 2) * 4
    assert rt.device_ptr(_lib.BUF_HMIP)[1] == info["hm_h"] * info["hm_w"] * 4
    assert mm.check_A(got["mip"], D, shift) == []
    assert mm.check_B(got["mip2"], D, m2) == []
    assert mm.check_H(got["hmip"], D, hs) == []
    return info


def one_shape(h, w):
    """Both spike sets of spiked_dem: the edges of the last cell, and its middle (what only that cell holds)."""
    T = mm.noise_colour(h + 3, max(w - 1, 2) + 4)
    for interior in (False, True):
        D = mm.spiked_dem(h, w, interior=interior)
        rt, s = context(D, T)
        try:
            march(rt)
            info = check_structures(rt, s, D, T)
            assert info["mip_shift"] == 4 and info["m2_shift"] == 2        # the default step on these DEMs
        finally:
            rt.close()


def test_small_ragged_shapes(native_lib):
    for h, w in SMALL:
        one_shape(h, w)


def test_130_x_257(native_lib):
    one_shape(130, 257)


def test_366_x_731(native_lib):
    """The seam regression's shape (tests/test_gpu_parity.py::seam_ridge_case): 731 = 45 x 16 + 11."""
    one_shape(366, 731)


def step_for(h, w, radius, shift):
    """A marching step in the middle of the band that gives `shift`: span = 16 step / texel + 3.5 = 0.75 x 2^shift."""
    texel = min(np.pi * radius / h, 2.0 * np.pi * radius / w)
    return (0.75 * (1 << shift) - 3.5) * texel / 16.0


def test_every_shift(native_lib):
    """Shifts 4 .. 10 on the 64 x 129 and the 130 x 257 DEM, reached by raising marching_step (parameter validation admits any
    positive step): cells larger than the whole map (mip_w == 1 from shift 8 / 9, hm_w == 1 from shift 5 / 6: the "dilated
    range wraps the whole map" branch) and m2_shift at its floor of 2 (shift 4).

    Reached on the MI355X: shifts {4, 5, 6, 7, 8, 9, 10} on both DEMs; mip_w == 1 at shifts 8, 9, 10 (64 x 129) and 9, 10
    (130 x 257); hm_w == 1 at shifts 5 .. 10 and 6 .. 10; m2_shift == 2 at shift 4."""
    for h, w in ((64, 129), (130, 257)):
        T = mm.noise_colour(h - 1, w + 2)
        rt, s = context(mm.spiked_dem(h, w), T)
        reached, whole_w, whole_hw, m2_floor = set(), set(), set(), set()
        try:
            for shift in range(4, 11):
                D = mm.spiked_dem(h, w, shift, interior=bool(shift & 1))
                rt.upload_dem(D)
                assert all(rt.device_ptr(b) == (None, 0) for b in MIPS)      # a new DEM: nothing is built for it yet
                rt.set_params(marching_step=step_for(h, w, s.radius, shift))
                march(rt)
                info = check_structures(rt, s, D, T)
                assert info["mip_shift"] == shift
                reached.add(info["mip_shift"])
                for seen, hit in ((whole_w, info["mip_w"] == 1), (whole_hw, info["hm_w"] == 1), (m2_floor, info["m2_shift"] == 2)):
                    if hit:
                        seen.add(shift)
        finally:
            rt.close()
        print(f"{h} x {w}: shifts {sorted(reached)}, mip_w == 1 at {sorted(whole_w)}, hm_w == 1 at {sorted(whole_hw)}, "
              f"m2_shift == 2 at {sorted(m2_floor)}")
        assert reached >= {4, 5, 6} and whole_w and whole_hw and m2_floor == {4}
        assert reached == set(range(4, 11))


def test_build_life_cycle(native_lib):
    """Null before the first marching call; the same step does not rebuild (the pointers stay), a changed step does; a new DEM
    drops the structures; an unknown id is refused."""
    h, w = 64, 129
    D, T = mm.spiked_dem(h, w), mm.noise_colour(5, 7)
    rt, s = context(D, T)
    try:
        assert all(rt.device_ptr(b) == (None, 0) for b in MIPS)
        assert all(rt.read_structure(b) is None for b in MIPS)
        assert set(rt.mip_info().values()) == {0}
        assert rt.device_ptr(_lib.BUF_DEM)[0] and rt.device_ptr(_lib.BUF_COLOR)[0]
        march(rt)
        first = [rt.device_ptr(b) for b in MIPS]
        assert all(p and n for p, n in first)
        info = check_structures(rt, s, D, T)
        march(rt)
        rt.set_params(marching_step=float(rt.params.marching_step) * 1.5)      # another step, the same cell size
        march(rt)
        assert [rt.device_ptr(b) for b in MIPS] == first and rt.mip_info() == info
        rt.set_params(marching_step=step_for(h, w, s.radius, 6))
        march(rt)
        again = check_structures(rt, s, D, T)
        assert again["mip_shift"] == 6 and again != info
        rt.upload_dem(D)
        assert all(rt.device_ptr(b) == (None, 0) for b in MIPS) and set(rt.mip_info().values()) == {0}
        for bad in (7, -1, 100):
            with pytest.raises(MoonRTError, match="unknown buffer id"):
                rt.device_ptr(bad)
    finally:
        rt.close()
