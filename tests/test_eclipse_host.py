"""The Earth's occultation of the Sun on the host (DESIGN.md sections 3.18 and 4.20): known answers of the two-disc rule,
far_sun_epochs, the 2025-03-14 eclipse from the float64 model against its published contacts, a lunation and a year of the
prefilter, and the named defects of the restated SUMMARY walk.  No GPU."""
import json
import math
import os
from datetime import datetime, timedelta, timezone

import numpy as np
import pytest

import eclipse_model as em
import epoch_patterns as ep
from moonrtx_amd import ephemeris as E
from moonrtx_amd.scene import MOON_RADIUS, MOON_RADIUS_KM, named_scene

OBS = E.Observer(52.2, 21.0, 0.0)
UTC = timezone.utc
A_SUN = math.radians(0.266)
# Each contact against its published time: the largest difference measured when this test was written was 2.90 minutes
# (DESIGN.md section 4.20 lists all seven), rounded up to 3, plus 2.  Its sources: the published shadow is enlarged by about
# 2 % for the atmosphere (0.011 to 0.02 deg at 0.0075 deg per minute: 1.5 to 2.7 minutes, early ingress, late egress), the
# 1-minute step, and the series' own 10 arc seconds.
CONTACT_MARGIN_MIN = 5.0


def smooth_sphere():
    return named_scene("S1", 16, 16), np.ones((8, 16))


def sphere_points(seed, n):
    rng = np.random.default_rng(seed)
    return np.degrees(np.arcsin(rng.uniform(-1.0, 1.0, n))), rng.uniform(-180.0, 180.0, n)


@pytest.mark.parametrize("rule", [em.two_disc, em.vector_two_disc, E.two_disc_fraction], ids=["loops", "numpy", "package"])
def test_known_answers_of_the_rule(rule):
    a = A_SUN
    assert rule(0.0, a, 3.6 * a) == 0.0 and rule(2.6 * a - 1e-12, a, 3.6 * a) == 0.0          # concentric and larger; total
    assert rule(4.6 * a, a, 3.6 * a) == 1.0 and rule(9.0 * a, a, 3.6 * a) == 1.0              # tangent outside, and beyond
    assert rule(0.0, a, 0.4 * a) == pytest.approx(1.0 - 0.16, abs=1e-15)                      # annular
    assert rule(0.6 * a, a, 0.4 * a) == pytest.approx(1.0 - 0.16, abs=1e-15)
    # equal discs one radius apart: the lens is (2 pi / 3 - sqrt(3) / 2) r^2
    assert rule(a, a, a) == pytest.approx(1.0 - (2.0 * math.pi / 3.0 - math.sqrt(3.0) / 2.0) / math.pi, abs=1e-14)
    # a body much larger than the source with its limb through the source's centre: a half, less the limb's curvature,
    # which keeps a_s^3 / (3 a_b) of the disc's area uncovered to first order: a_s / (3 pi a_b) of it
    big = 500.0 * a
    assert rule(big, a, big) == pytest.approx(0.5 + a / (3.0 * math.pi * big), abs=1e-6)
    assert abs(float(rule(big, a, big)) - 0.5) < 1e-3
    # monotone in the separation
    sep = np.linspace(0.0, 5.0 * a, 2001)
    for a_b in (0.4 * a, a, 3.6 * a):
        g = np.asarray(rule(sep, a, a_b), float)
        assert np.all(np.diff(g) >= -1e-15), a_b
        assert g[-1] == 1.0
    if rule is not em.vector_two_disc:          # a point source: a step at the body's limb
        assert rule(0.999, 0.0, 1.0) == 0.0 and rule(1.0, 0.0, 1.0) == 0.0 and rule(1.001, 0.0, 1.0) == 1.0


def test_the_three_statements_of_the_rule_agree():
    rng = np.random.default_rng(4)
    sep, a_s, a_b = rng.uniform(0, 0.02, 4000), rng.uniform(1e-3, 6e-3, 4000), rng.uniform(1e-3, 2e-2, 4000)
    want = em.two_disc(sep, a_s, a_b)
    assert np.abs(em.vector_two_disc(sep, a_s, a_b) - want).max() < 1e-13
    assert np.abs(E.two_disc_fraction(sep, a_s, a_b) - want).max() < 1e-13
    assert ((want > 0) & (want < 1)).sum() > 500 and (want == 0).sum() > 100 and (want == 1).sum() > 100     # all cases met


def test_far_sun_epochs_keep_direction_and_angular_radius():
    times = [datetime(2025, 3, 14, 3, 40, tzinfo=UTC) + timedelta(hours=7 * k) for k in range(12)]
    sun = E.sun_epochs(times, OBS)
    far = E.far_sun_epochs(sun, times)
    assert far.shape == sun.shape and far is not sun
    near_ray, far_ray = sun[:, 0:3] - sun[:, 5:8], far[:, 0:3] - far[:, 5:8]
    d0, d1 = np.linalg.norm(near_ray, axis=1), np.linalg.norm(far_ray, axis=1)
    assert np.abs(near_ray / d0[:, None] - far_ray / d1[:, None]).max() < 1e-15
    assert np.abs((far[:, 3] / d1) / (sun[:, 3] / d0) - 1.0).max() < 1e-14
    assert np.array_equal(far[:, 4:], sun[:, 4:])               # radiance and Moon frame
    # the distance is the one sun_flux uses: S = 1361 (1 AU / r)^2
    r_km = d1 * (MOON_RADIUS_KM / MOON_RADIUS)
    assert np.abs(1361.0 / (r_km / E.AU_KM) ** 2 / E.sun_flux(times) - 1.0).max() < 1e-13
    assert np.all((r_km > 1.45e8) & (r_km < 1.53e8))
    with pytest.raises(ValueError):
        E.far_sun_epochs(sun, times[:-1])


@pytest.fixture(scope="module")
def march_eclipse():
    """The model's g over 3000 points of the smooth sphere, every minute from 03:40 to 10:19 UTC on 2025-03-14."""
    t0 = datetime(2025, 3, 14, 3, 40, tzinfo=UTC)
    times = [t0 + timedelta(minutes=k) for k in range(400)]
    sun, earth = E.sun_earth_epochs(times, OBS)
    s, dem = smooth_sphere()
    lat, lon = sphere_points(1, 3000)
    g, info = em.occult_g(s, dem, lat, lon, E.far_sun_epochs(sun, times), earth)
    return times, g, info


def test_the_eclipse_of_2025_03_14(march_eclipse):
    times, g, info = march_eclipse
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eclipse_2025_03_14.json")
    with open(here) as fh:
        pub = {k: datetime.strptime("2025-03-14 " + v, "%Y-%m-%d %H:%M:%S").replace(tzinfo=UTC)
               for k, v in json.load(fh)["contacts_utc"].items()}
    lit = info["mu"] > 0.0                                      # the points that see the Sun
    pen, umb = ((g < 1) & lit).any(0), ((g == 0) & lit).any(0)
    whole = np.array([lit[:, k].any() and bool((g[lit[:, k], k] == 0).all()) for k in range(len(times))])
    sep = [E._centre_geometry(t)[0] for t in times]
    at = {"P1": np.flatnonzero(pen)[0], "U1": np.flatnonzero(umb)[0], "U2": np.flatnonzero(whole)[0],
          "greatest": int(np.argmin(sep)), "U3": np.flatnonzero(whole)[-1], "U4": np.flatnonzero(umb)[-1],
          "P4": np.flatnonzero(pen)[-1]}
    got = {k: times[int(v)] for k, v in at.items()}
    order = ["P1", "U1", "U2", "greatest", "U3", "U4", "P4"]
    assert all(got[a] < got[b] for a, b in zip(order, order[1:])), got
    diff = {k: (got[k] - pub[k]).total_seconds() / 60.0 for k in order}
    print("contact, model, published, difference in minutes:")
    for k in order:
        print(f"  {k:9s} {got[k]:%H:%M} {pub[k]:%H:%M:%S} {diff[k]:+.2f}")
    # the geometric shadow is the smaller one: both spans lie inside the published ones
    assert got["P1"] >= pub["P1"] and got["P4"] <= pub["P4"], diff
    assert got["U1"] >= pub["U1"] and got["U4"] <= pub["U4"], diff
    assert max(abs(v) for v in diff.values()) <= CONTACT_MARGIN_MIN, diff
    assert math.degrees(min(sep)) == pytest.approx(0.316, abs=0.002)
    assert ((g > 0) & (g < 1)).sum() > 1000 and (g == 0).sum() > 1000


def test_a_lunation_without_an_eclipse():
    t0 = datetime(2025, 4, 1, tzinfo=UTC)
    times = [t0 + timedelta(hours=k) for k in range(709)]
    assert E.eclipse_candidates(times, OBS) == []
    assert np.all(E.eclipse_factor(times, OBS) == 1.0)
    sun, earth = E.sun_earth_epochs(times, OBS)
    s, dem = smooth_sphere()
    lat, lon = sphere_points(2, 200)
    g, _ = em.occult_g(s, dem, lat, lon, E.far_sun_epochs(sun, times), earth)
    assert np.all(g == 1.0)


def test_the_eclipses_of_2025():
    t0 = datetime(2025, 1, 1, tzinfo=UTC)
    times = [t0 + timedelta(hours=k) for k in range(8760)]
    ranges = E.eclipse_candidates(times, OBS)
    assert len(ranges) == 2, ranges
    (a0, a1), (b0, b1) = ranges
    assert times[a0].date() == times[a1 - 1].date() == datetime(2025, 3, 14).date()
    assert times[b0].date() == times[b1 - 1].date() == datetime(2025, 9, 7).date()
    assert 5 <= a1 - a0 <= 9 and 5 <= b1 - b0 <= 9
    g = E.eclipse_factor(times[a0:a1], OBS)
    assert g.min() == 0.0 and g[0] > 0.9                         # totality at the centre; the range opens near first contact
    # the prefilter contains every date at which the centre's factor is below 1
    assert np.all(E.eclipse_factor(times[a0 - 3:a0], OBS) == 1.0) and np.all(E.eclipse_factor(times[a1:a1 + 3], OBS) == 1.0)


def test_summary_loops_on_a_hand_made_row():
    g = np.array([[1, .5, 0, 0, 1, 1, .2, .3, 1, 0, 0, 0, .5]])
    want = [g.sum() / 13, 0.0, 9 / 13, 5 / 13, 4, 9, 3, 3]
    assert np.allclose(em.summarize(g)[0], want, rtol=0, atol=1e-15)
    assert np.array_equal(em.summarize(np.ones((1, 5)))[0], [1, 1, 0, 0, 0, -1, 0, 0])
    assert np.array_equal(em.summarize(np.zeros((1, 5)))[0], [0, 0, 1, 1, 5, 0, 5, 1])


@pytest.mark.parametrize("m", ep.M)
def test_the_restated_walk_equals_the_loops(m):
    for chunk in (64, 8):
        for name, codes in em.designed_codes(m):
            g = em.codes_as_g(codes)[None]
            assert np.array_equal(em.chunked_summary(g, chunk), em.summarize(g)), (m, chunk, name)


@pytest.mark.parametrize("mutant", em.MUTANTS)
def test_each_named_defect_is_told_from_the_correct_walk(mutant):
    """Over the epoch counts and the designed sequences the GPU test runs, the defective walk differs from the plain loops
    somewhere; which columns it spoils is printed."""
    cols, cases = set(), 0
    for m in ep.M:
        for name, codes in em.designed_codes(m):
            g = em.codes_as_g(codes)[None]
            bad = np.flatnonzero(em.chunked_summary(g, 64, mutant)[0] != em.summarize(g)[0])
            if bad.size:
                cases += 1
                cols.update(int(j) for j in bad)
    print(f"{mutant}: told apart in {cases} cases, columns {sorted(cols)}")
    assert cases > 0
    expected = {"count_forgets_carried_bit": {7}, "start_off_by_chunk": {5}, "tie_takes_later": {5},
                "inactive_lanes_partial": {2, 4, 5, 7}, "no_carry": {4, 5, 6}}[mutant]
    assert cols & expected, (mutant, cols)
