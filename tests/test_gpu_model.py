"""The HIP kernels against the float64 model of the full sample (oracle/numpy_paths.py) and the analytic known answers of
tests/test_oracle_model_paths.py, directly: production (flags 0) and counting (F_COUNT_STATS) instantiations, the path
queue and the in-wave path loop (F_INWAVE_PATHS), 1 to 64 samples per launch.  Bit-equality with the C oracle cannot
catch an error the two share through the spec; this can."""
import pytest

import model_cases as mc
from common import render_hip
from moonrtx_amd import _lib

pytestmark = pytest.mark.gpu

FLAGS = {"queue-count": _lib.F_COUNT_STATS, "queue-prod": 0,
         "inwave-count": _lib.F_INWAVE_PATHS | _lib.F_COUNT_STATS, "inwave-prod": _lib.F_INWAVE_PATHS}


def hip(flags):
    def render(scene, dem, color, bg, blocks):
        lin, hits, st, _ = render_hip(scene, dem, color, bg, blocks=(blocks,), flags=flags)
        return lin, hits, st
    return render


@pytest.mark.parametrize("mode", list(FLAGS))
@pytest.mark.parametrize("spp", [1, 16, 64])
def test_hip_paths_match_the_model_per_pixel(native_lib, mode, spp):
    fl = FLAGS[mode]
    s = mc.paths_scene((2, 4), spp=spp)
    blocks = {1: 16, 16: 2, 64: 1}[spp]                  # >= 16 samples per pixel (see check_per_pixel)
    mc.check_per_pixel(hip(fl), s, mc.crater_dem(), mc.colour(), mc.env_texture(), blocks=blocks,
                       counted=bool(fl & _lib.F_COUNT_STATS))


@pytest.mark.parametrize("mode", list(FLAGS))
@pytest.mark.parametrize("seg", [(1, 1), (1, 3), (4, 4)])
def test_hip_segment_ranges_match_the_model(native_lib, mode, seg):
    fl = FLAGS[mode]
    mc.check_per_pixel(hip(fl), mc.paths_scene(seg), mc.crater_dem(), mc.colour(), mc.env_texture(),
                       counted=bool(fl & _lib.F_COUNT_STATS))


@pytest.mark.parametrize("mode", ["queue-prod", "inwave-prod"])
def test_hip_steep_relief_matches_the_model(native_lib, mode):
    mc.check_per_pixel(hip(FLAGS[mode]), mc.paths_scene((2, 4)), mc.corrugated_dem(), mc.colour(), mc.env_texture(),
                       strict=False, counted=False)


@pytest.mark.parametrize("mode", ["queue-count", "inwave-count"])
def test_hip_sphere_in_a_uniform_environment(native_lib, mode):
    mc.sphere_in_uniform_environment(hip(FLAGS[mode]))


@pytest.mark.parametrize("mode", ["queue-count", "inwave-count"])
def test_hip_russian_roulette_is_unbiased(native_lib, mode):
    mc.roulette_is_unbiased(hip(FLAGS[mode]))


@pytest.mark.parametrize("mode", ["queue-count", "inwave-count"])
def test_hip_sun_disk_through_continuation_rays(native_lib, mode):
    mc.sun_disk_through_continuation_rays(hip(FLAGS[mode]))


def test_hip_colour_map_grid(native_lib):
    mc.colour_map_grid(hip(0))
