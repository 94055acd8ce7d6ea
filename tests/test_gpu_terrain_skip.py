"""The skip identity of the terrain queries where the suite did not have it: illumination_at, illumination_series, horizon (ground
and mast top), view_hits and line_of_sight give the SAME BITS with the max-mip / medium-mip / horizon-mip skips (flags 0 and
F_COUNT_STATS), without them (F_NO_SKIP) and with 64-bit DEM addressing (F_FORCE_WIDE), on ragged DEMs (366 x 731 and
183 x 365: no w = 2h, no even size, a partial last mip cell in both directions), at the +-180 seam, next to both poles and at
interior controls.  The library is compared with itself: no model, no tolerance."""
import dataclasses
import math

import numpy as np
import pytest

import illum_model as im
from common import assert_bit_equal
from moonrtx_amd import _lib
from moonrtx_amd.renderer import MoonRT
from test_gpu_parity import seam_ridge_case

pytestmark = pytest.mark.gpu

N_SUN, N_AZ, N_BIS, K = 8, 16, 8, 16
WEST = 3 * N_AZ // 4                      # azimuth 270 degrees
FLAGS = {"skip": _lib.F_COUNT_STATS, "plain": 0, "noskip": _lib.F_COUNT_STATS | _lib.F_NO_SKIP,
         "wide": _lib.F_COUNT_STATS | _lib.F_FORCE_WIDE}
QUERIES = ("illumination_at", "illumination_series", "horizon", "horizon_mast", "view_hits", "line_of_sight")


def walled_dem():
    """183 x 365 (365 = 22 x 16 + 13, 183 = 11 x 16 + 7): one-texel walls along row 1 and row h - 2, and a meridian ridge on
    columns 357 .. 361, inside the last, partial mip cell west of the seam and outside every neighbour's two-texel border.
    The ridge stands above the walls: every horizon-mip cell of a map this small holds a wall, and walls as high as the ridge
    would stand in for it in a cell that missed the partial fine cell."""
    h, w = 183, 365
    rng = np.random.default_rng(12)
    dem = np.full((h, w), 0.98, np.float32) + rng.random((h, w)).astype(np.float32) * np.float32(2e-4)
    dem[1, :] = 0.99
    dem[h - 2, :] = 0.99
    dem[:, 357:362] = 1.0
    return dem


def flattened(name, dem):
    """The terrain without its seam ridge (as test_horizon_mip_sees_the_partial_cell_across_the_seam flattens it)."""
    flat = dem.copy()
    if name == "seam_ridge":
        flat[:, 723:728] = flat[:, 700:705]
    else:
        flat[:, 357:362] = flat[:, 330:335]
    return flat


def terrain(name):
    s, dem = seam_ridge_case()
    return s, (dem if name == "seam_ridge" else walled_dem())


def seam_columns(w):
    """Longitudes of the centres of columns 0 .. 3, just east of the seam."""
    return -180.0 + (np.arange(4) + 0.5) * 360.0 / w


def points(h, w):
    """About 40 points: columns 0 .. 3 east of the seam at two low latitudes, the same longitudes a turn further, the seam itself
    written three ways, the first three texel rows at each pole (centres and in between) with the poles themselves, and
    interior controls."""
    lon4 = seam_columns(w)
    pts = [(5.0, lo) for lo in lon4] + [(-3.0, lo) for lo in lon4] + [(5.0, lo + 360.0) for lo in lon4]
    pts += [(2.0, 180.0), (2.0, -180.0), (2.0, 540.0 - 1e-9)]
    for sign in (1.0, -1.0):
        pts.append((sign * 90.0, 0.0))
        for r in (0, 1, 2):
            for k, lo in enumerate((0.0, 120.0, -179.9)):
                pts.append((sign * (90.0 - (r + 0.5 + 0.2 * k) * 180.0 / h), lo))
    pts += [(0.0, 0.0), (30.0, 90.0), (-45.0, -120.0), (60.0, 179.0), (-20.0, 93.0)]
    a = np.array(pts, np.float64)
    return a[:, 0], a[:, 1]


def sun_at(s, lat_deg, lon_deg):
    """The scene with its light over the selenographic point (lat, lon)."""
    _, M = im.sun_dir_moon_frame(s)
    la, lo = math.radians(lat_deg), math.radians(lon_deg)
    d = float(np.linalg.norm(np.asarray(s.light_pos, float) - np.asarray(s.center, float)))
    body = d * np.array([math.cos(la) * math.sin(lo), math.cos(la) * math.cos(lo), math.sin(la)])
    out = dataclasses.replace(s, light_pos=tuple(np.asarray(s.center, float) + M.T @ body))
    assert np.allclose(im.subsolar_latlon(out), (lat_deg, lon_deg), atol=1e-9)
    return out


LOW_WEST = (0.0, 93.5)      # seen from columns 0 .. 3 (lon 180.25 .. 181.7): 3.2 .. 1.8 degrees above the western horizon


def epochs(s):
    """A dozen dates: the Sun between 6.7 degrees above and 4.3 below the western horizon of the seam points."""
    return [sun_at(s, 1.5 * (-1) ** k, 90.0 + k) for k in range(12)]


def observers(la, lo):
    """One observer per target, 30 km up and six degrees of longitude to its west: from the seam points the line runs back across
    the seam and the ridge, and every line climbs well clear of the ground on its way, which is where a skip has steps to prove
    empty (a line that dives into the terrain within a few steps gives the skip nothing to do: all of its steps are needed)."""
    return np.stack([la, lo - 6.0, np.full(la.size, 30000.0)], -1)


def run_queries(s, dem, flags):
    """name -> (list of output arrays, counters) of the six queries through one context."""
    h, w = dem.shape
    la, lo = points(h, w)
    rt = MoonRT(16, 16)
    out = {}
    try:
        rt.upload_dem(dem)
        rt.apply_scene(sun_at(s, *LOW_WEST))
        rt.set_params(flags=flags)
        st = {}
        out["illumination_at"] = ([rt.illumination_at(la, lo, n_sun=N_SUN, stats=st)], st)
        st = {}
        out["illumination_series"] = ([rt.illumination_series(la, lo, epochs(s), n_sun=N_SUN, stats=st)], st)
        st = {}
        out["horizon"] = ([rt.horizon(la, lo, n_az=N_AZ, n_bis=N_BIS, stats=st)], st)
        st = {}
        out["horizon_mast"] = ([rt.horizon(la, lo, n_az=N_AZ, n_bis=N_BIS, height_m=10.0, stats=st)], st)
        st = {}
        out["view_hits"] = (list(rt.view_hits(la, lo, k=K, stats=st)), st)
        st = {}
        out["line_of_sight"] = ([rt.line_of_sight(la, lo, observers(la, lo), target_height_m=2.0, mast_max_m=20000.0,
                                                  n_bis=N_BIS, stats=st)], st)
    finally:
        rt.close()
    return out


_cache = {}


def results(name):
    """The four runs of the six queries on one terrain, computed once for the module."""
    if name not in _cache:
        s, dem = terrain(name)
        _cache[name] = {tag: run_queries(s, dem, flags) for tag, flags in FLAGS.items()}
    return _cache[name]


@pytest.mark.parametrize("query", QUERIES)
@pytest.mark.parametrize("name", ["seam_ridge", "walled"])
def test_skip_identity(native_lib, name, query):
    runs = {tag: results(name)[tag][query] for tag in FLAGS}
    base, st_skip = runs["skip"]
    assert all(np.asarray(a).size > 0 for a in base)
    for tag in ("plain", "noskip", "wide"):
        for a, b in zip(runs[tag][0], base):
            assert a.shape == b.shape
            assert_bit_equal(a, b, f"{query} on {name}: {tag} against the counting skip run")
    rays = "bounce_rays" if query == "view_hits" else "shadow_rays"
    st_full, st_wide = runs["noskip"][1], runs["wide"][1]
    print(f"{name} {query}: {rays} {st_skip[rays]}, height_samples {st_skip['height_samples']}, dem_fetches "
          f"{st_skip['dem_fetches']} (skip) / {st_full['dem_fetches']} (no skip), mip_fetches {st_skip['mip_fetches']}")
    assert st_skip[rays] > 0 and st_skip["height_samples"] > 0
    for st in (st_full, st_wide):
        assert (st[rays], st["height_samples"]) == (st_skip[rays], st_skip["height_samples"])
    assert st_full["mip_fetches"] == 0
    assert st_skip["mip_fetches"] > 0 and st_skip["dem_fetches"] < st_full["dem_fetches"]
    assert (st_wide["mip_fetches"], st_wide["dem_fetches"]) == (st_skip["mip_fetches"], st_skip["dem_fetches"])


@pytest.mark.parametrize("name", ["seam_ridge", "walled"])
def test_the_case_is_what_it_claims(native_lib, name):
    """The ridge in the partial cell west of the seam is what the column 0 .. 3 points see in the west: without it their westward
    horizon drops by more than one bisection step, and under the low western Sun they are lit instead of dark.  So a
    horizon-mip or max-mip cell that missed the ridge would change these outputs."""
    s, dem = terrain(name)
    lo = seam_columns(dem.shape[1])
    la = np.full(4, 5.0)
    got = {}
    for tag, d in (("ridge", dem), ("flat", flattened(name, dem))):
        rt = MoonRT(16, 16)
        try:
            rt.upload_dem(d)
            rt.apply_scene(sun_at(s, *LOW_WEST))
            got[tag] = (rt.horizon(la, lo, n_az=N_AZ, n_bis=N_BIS)[:, WEST], rt.illumination_at(la, lo, n_sun=N_SUN)[:, 0])
        finally:
            rt.close()
    print(f"{name}: westward horizon {got['ridge'][0]} with the ridge, {got['flat'][0]} without; lit {got['ridge'][1]} / "
          f"{got['flat'][1]}")
    assert (got["ridge"][0] - got["flat"][0] > 180.0 / 2 ** N_BIS).all()
    assert (got["ridge"][1] == 0.0).all() and (got["flat"][1] > 0.0).all()
    # and the skip run of the identity above reports the same values for these points (the first four of its list)
    base = results(name)["skip"]
    assert_bit_equal(base["horizon"][0][0][:4, WEST], got["ridge"][0], "westward horizon of the seam points")
    assert_bit_equal(base["illumination_at"][0][0][:4, 0], got["ridge"][1], "lit of the seam points")
