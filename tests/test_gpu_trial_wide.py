"""The trial segment of render_kernel<MODE 2> -- the first 16-step segment of every sample's continuation ray, marched in
the render wave -- on frames built to put its step loop under load: many pending steps per wave
(every skip off), one round's worth (skips on), rays that graze for many steps and then land, every wave packing with the
frame edge inside a wave, lanes without a path between lanes with long ones, and exact-fallback segments beside ordinary
ones.  Whether the steps of a wave's straggler rays are walked one iteration at a time or dealt out over the wave's lanes
(MRTX_TRIAL_WIDE), the frame is the oracle's: radiance, hit records and, in the counting build, every spec counter, through
the queue and through the in-wave path loop, production and counting instantiations alike."""
import numpy as np
import pytest

import fuzz_cases
import synth_np
from common import STAT_KEYS, assert_bit_equal, render_hip, render_oracle
from moonrtx_amd import _lib
from moonrtx_amd.scene import named_scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rough():
    return synth_np.corrugated_dem(720, 1440)      # steep relief: continuation rays really do hit terrain again


@pytest.fixture(scope="module")
def pitted():
    return fuzz_cases.dense_dem(np.random.default_rng(20240), 720)      # terraces, pits, spikes and one-texel walls


def paths(scene):
    scene.path_seg_min, scene.path_seg_max = 2, 4
    return scene


def three_way(scene, dem, extra_flags=0, tile=(32, 32)):
    """Queue, in-wave loop and oracle; production and counting instantiations.  Returns the oracle's counters."""
    lin_o, hits_o, st_o = render_oracle(scene, dem)
    for tag, fl in (("queue", 0), ("inwave", _lib.F_INWAVE_PATHS)):
        for count in (_lib.F_COUNT_STATS, 0):
            lin, hits, st, _ = render_hip(scene, dem, tile=tile, flags=fl | count | extra_flags)
            assert_bit_equal(lin, lin_o, f"{tag} (count={count}, flags={extra_flags}) radiance vs oracle")
            assert_bit_equal(hits, hits_o, f"{tag} (count={count}, flags={extra_flags}) hits vs oracle")
            if count:
                assert {k: st[k] for k in STAT_KEYS} == {k: st_o[k] for k in STAT_KEYS}, (tag, extra_flags)
            assert (st["paths_ms"] > 0.0) == (tag == "queue")
    return st_o


def test_every_step_pending_spans_many_rounds(native_lib, rough):
    """F_NO_SKIP: each continuing lane has all 16 steps of the trial pending, so a wave with five continuing lanes already
    holds more than 64 steps and most hold about a thousand -- rays straddle the rounds.  (Dealing steps out is not a skip:
    it stays on.)"""
    st = three_way(paths(named_scene("S1", 70, 50, spp_per_launch=64)), rough, extra_flags=_lib.F_NO_SKIP)
    assert st["bounce_rays"] >= st["primary_hits"] > 64 * 5


@pytest.mark.parametrize("flags", [0, _lib.F_FORCE_WIDE], ids=["narrow", "wide-addressing"])
def test_skips_on_one_round(native_lib, rough, flags):
    """The same frame with the skips on (what is left fits one round in most waves), 32- and 64-bit DEM addressing; the
    default scene_epsilon keeps the grazing rays that step many times and then land on the next ridge."""
    st = three_way(paths(named_scene("S1", 70, 50, spp_per_launch=64)), rough, extra_flags=flags)
    assert st["bounce_rays"] >= st["primary_hits"] > 0


@pytest.mark.parametrize("flags", [0, _lib.F_NO_SKIP], ids=["skip", "noskip"])
def test_pits_and_one_texel_walls(native_lib, pitted, flags):
    """A dense DEM with long march steps: rays climb out of pits and along one-texel walls, and land late in the segment."""
    s = paths(named_scene("S1", 48, 36, spp_per_launch=64))
    s.marching_step = 3e-2 * (s.radius / 10.0)
    s.marching_step_eps = 0.2 * s.marching_step
    st = three_way(s, pitted, extra_flags=flags)
    assert st["bounce_rays"] > 0


@pytest.mark.parametrize("spp", [1, 2, 4, 16, 64])
def test_every_packing_with_the_frame_edge_inside_a_wave(native_lib, rough, spp):
    """33 x 21: waves hold several pixels (S < 64) and the last pixel blocks hang over the frame's edge."""
    st = three_way(paths(named_scene("S1", 33, 21, spp_per_launch=spp)), rough)
    assert st["bounce_rays"] >= st["primary_hits"] > 0
    three_way(paths(named_scene("S1", 33, 21, spp_per_launch=spp)), rough, extra_flags=_lib.F_NO_SKIP)


def test_limb_heavy_view(native_lib, rough):
    """A crescent: along the limb and the terminator, lanes without any path sit between lanes with long ones."""
    st = three_way(paths(named_scene("S3", 64, 48, spp_per_launch=64)), rough)
    assert 0 < st["primary_hits"] < st["primary_rays"]
    three_way(paths(named_scene("S3", 64, 48, spp_per_launch=16)), rough, extra_flags=_lib.F_NO_SKIP)


@pytest.mark.parametrize("libration", [(179.5, 5.0), (0.0, 89.0)], ids=["seam", "pole"])
def test_exact_fallback_waves_beside_ordinary_ones(native_lib, rough, libration):
    """A view over the +-180 degree seam / the polar cap: waves with a lane in an exact-fallback segment keep the serial loop,
    their neighbours do not."""
    for flags in (0, _lib.F_NO_SKIP):
        st = three_way(paths(named_scene("S1", 48, 40, spp_per_launch=16, libration=libration)), rough, extra_flags=flags)
        assert st["bounce_rays"] > 0
