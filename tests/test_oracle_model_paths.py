"""The C oracle against the float64 model of the full sample (oracle/numpy_paths.py: colour map, path continuation with
Russian roulette, environment, Sun disk, coverage, hit buffer) and against analytic known answers (CPU only).

The HIP kernels are held bit-exact to the oracle; both follow one arithmetic spec, so an error in the
spec is invisible to those tests.  These compare the spec with the MODEL it states."""
import numpy as np
import pytest

import model_cases as mc
from common import render_oracle


def oracle(scene, dem, color, bg, blocks):
    return render_oracle(scene, dem, color, bg, blocks=(blocks,))


@pytest.mark.parametrize("seg", mc.SEGS)
def test_paths_match_the_model_per_pixel_on_craters(oracle_lib, seg):
    s = mc.paths_scene(seg)
    _, m = mc.check_per_pixel(oracle, s, mc.crater_dem(), mc.colour(), mc.env_texture())
    st = m["stats"]
    if seg[1] > 1:
        assert st["bounce_rays"] >= st["primary_hits"] * (seg[0] > 1) and st["bounce_sun_hits"] > 0


@pytest.mark.parametrize("seg", mc.SEGS)
def test_paths_match_the_model_per_pixel_on_steep_relief(oracle_lib, seg):
    s = mc.paths_scene(seg)
    _, m = mc.check_per_pixel(oracle, s, mc.corrugated_dem(), mc.colour(), mc.env_texture(), strict=False)
    if seg[1] > 2:
        assert m["stats"]["bounce_rays"] > m["stats"]["primary_hits"] * (seg[0] > 1)   # continuation rays hit terrain again


def test_sphere_in_a_uniform_environment(oracle_lib):
    mc.sphere_in_uniform_environment(oracle)


def test_russian_roulette_is_unbiased(oracle_lib):
    mc.roulette_is_unbiased(oracle)


def test_sun_disk_seen_by_continuation_rays_matches_its_solid_angle(oracle_lib):
    mc.sun_disk_through_continuation_rays(oracle)


def test_colour_map_lands_on_its_own_grid(oracle_lib):
    mc.colour_map_grid(oracle)


def test_model_own_rng_agrees_statistically(oracle_lib):
    """The model with numpy's RNG and another hemisphere basis: the same image up to Monte-Carlo noise (the spec RNG's
    dimensions and the Duff basis are not what makes the per-pixel agreement)."""
    from oracle import numpy_paths
    s = mc.paths_scene((2, 4), spp=64, width=32, height=16)
    lin, _, _ = oracle(s, mc.crater_dem(), mc.colour(), mc.env_texture(), 1)
    m = numpy_paths.render(s, mc.crater_dem(), mc.colour(), mc.env_texture(), blocks=1, spec_rng=False)
    x = (lin[..., :3].astype(np.float64) - m["linear"][..., :3]).ravel()
    sd = np.sqrt((2 * m["var"] / 64).ravel().mean())
    assert abs(x.mean()) < 4 * sd / np.sqrt(x.size) + 1e-6, (x.mean(), sd)
