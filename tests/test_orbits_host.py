"""moonrtx_amd.orbits on the CPU: the Kepler propagator against closed forms and against an RK4
two-body integration written here, the J2 node rate, the frame conversions, and a satellite at a point's zenith."""
import math
from datetime import datetime, timedelta, timezone

import numpy as np

import horizon_model as hm
import model_cases as mc
import passes_model as pm
from moonrtx_amd import orbits as ob

T0 = datetime(2026, 1, 1, tzinfo=timezone.utc)


def test_period_of_a_100_km_circular_orbit():
    a = ob.R_EQ_MOON + 100e3
    want = 2.0 * math.pi * math.sqrt(a ** 3 / 4.9028e12)
    assert ob.period_s(a) == want or abs(ob.period_s(a) - want) <= 1e-12 * want
    assert 7050.0 < want < 7080.0                               # the familiar 118 minutes
    # the mean anomaly advances by one turn in one period: the position repeats
    el = ob.Elements(a, 0.0, 90.0, 0.0, 0.0, 0.0, T0)
    p, _ = ob.kepler_inertial(el, [0.0, want], j2=False)
    assert np.linalg.norm(p[1] - p[0]) <= 1e-9 * a


def test_inertial_position_repeats_after_one_period():
    for e, inc in ((0.0, 90.0), (0.3, 57.0), (0.6, 28.0)):
        a = 3.0e6
        el = ob.Elements(a, e, inc, 40.0, 70.0, 25.0, T0)
        t = np.array([0.0, 1234.5, 9000.0])
        p0, v0 = ob.kepler_inertial(el, t, j2=False)
        p1, v1 = ob.kepler_inertial(el, t + ob.period_s(a), j2=False)
        assert np.abs(p1 - p0).max() <= 1e-9 * a, (e, np.abs(p1 - p0).max())


def test_energy_and_angular_momentum_are_constant():
    a, e = 6.0e6, 0.6
    el = ob.Elements(a, e, 63.0, 10.0, 270.0, 0.0, T0)
    t = np.linspace(0.0, 2.0 * ob.period_s(a), 400)
    p, v = ob.kepler_inertial(el, t, j2=False)
    r = np.linalg.norm(p, axis=1)
    energy = 0.5 * (v * v).sum(1) - ob.GM_MOON / r
    h = np.cross(p, v)
    assert np.abs(energy / (-ob.GM_MOON / (2.0 * a)) - 1.0).max() < 1e-12
    want_h = math.sqrt(ob.GM_MOON * a * (1.0 - e * e))
    assert np.abs(np.linalg.norm(h, axis=1) / want_h - 1.0).max() < 1e-12
    assert np.abs(h / want_h - h[0] / want_h).max() < 1e-12
    assert abs(r.min() - a * (1 - e)) < 1e-3 * a and abs(r.max() - a * (1 + e)) < 1e-3 * a
    # Kepler's equation is solved to the stated residual
    M = np.linspace(-20.0, 20.0, 1001)
    for ecc in (0.0, 0.6, 0.95):
        E = ob.solve_kepler(M, ecc)
        Mw = np.remainder(M + math.pi, 2 * math.pi) - math.pi
        assert np.abs(E - ecc * np.sin(E) - Mw).max() <= 1e-14


def test_j2_node_rate():
    for inc in (30.0, 90.0, 120.0):
        el = ob.Elements(ob.R_EQ_MOON + 100e3, 0.1, inc, 0.0, 0.0, 0.0, T0)
        n = ob.mean_motion(el.a_m)
        p = el.a_m * (1 - el.e ** 2)
        want = -1.5 * n * 2.0323e-4 * (1737400.0 / p) ** 2 * math.cos(math.radians(inc))
        rate = ob.j2_rates(el)[0]
        assert abs(rate - want) <= 1e-15 * abs(n)
        assert (rate < 0) == (inc < 90.0) or inc == 90.0
    # the propagated orbit's node moves at that rate: the orbit normal's azimuth after a day
    el = ob.Elements(ob.R_EQ_MOON + 100e3, 0.0, 30.0, 0.0, 0.0, 0.0, T0)
    t = np.array([0.0, 86400.0])
    p, v = ob.kepler_inertial(el, t, j2=True)
    h = np.cross(p, v)
    node = np.arctan2(h[:, 0], -h[:, 1])                        # the ascending node's right ascension
    assert abs((node[1] - node[0]) - ob.j2_rates(el)[0] * 86400.0) < 1e-9
    assert node[1] < node[0]                                     # a prograde orbit's node regresses


def rk4(p, v, dt, steps):
    def acc(x):
        return -ob.GM_MOON * x / np.linalg.norm(x) ** 3
    for _ in range(steps):
        k1p, k1v = v, acc(p)
        k2p, k2v = v + 0.5 * dt * k1v, acc(p + 0.5 * dt * k1p)
        k3p, k3v = v + 0.5 * dt * k2v, acc(p + 0.5 * dt * k2p)
        k4p, k4v = v + dt * k3v, acc(p + dt * k3p)
        p = p + dt / 6.0 * (k1p + 2 * k2p + 2 * k3p + k4p)
        v = v + dt / 6.0 * (k1v + 2 * k2v + 2 * k3v + k4v)
    return p


def test_agrees_with_an_rk4_two_body_integration():
    """Half a period of an e = 0.3 orbit.  RK4's global error falls 16-fold when the step halves, so the finer run's own error
    is about (coarse - fine) / 15; the propagator has to lie within twice the whole step-halving difference of the finer run."""
    a = 2.5e6
    el = ob.Elements(a, 0.3, 75.0, 15.0, 40.0, 10.0, T0)
    T = 0.5 * ob.period_s(a)
    p, v = ob.kepler_inertial(el, [0.0, T], j2=False)
    coarse, fine = rk4(p[0], v[0], T / 2000, 2000), rk4(p[0], v[0], T / 4000, 4000)
    halving = float(np.linalg.norm(coarse - fine))
    err = float(np.linalg.norm(p[1] - fine))
    print(f"RK4 step-halving difference {halving:.3e} m, propagator against the finer run {err:.3e} m")
    assert halving < 1.0                                         # the integration itself has converged to under a metre
    assert err <= 2.0 * halving + 1e-6


def test_fixed_frame_round_trip_and_axes():
    rng = np.random.default_rng(3)
    lat, lon, r = rng.uniform(-90, 90, 200), rng.uniform(-179.9, 180, 200), rng.uniform(1.8e6, 9e6, 200)
    la, lo, rr = ob.latlon_from_fixed(ob.fixed_from_latlon(lat, lon, r))
    assert np.abs(la - lat).max() < 1e-10 and np.abs(lo - lon).max() < 1e-10 and np.abs(rr / r - 1).max() < 1e-14
    # the body axes: x toward 90 E, y toward the prime meridian, z north -- horizon_model.frame's U
    assert np.allclose(ob.fixed_from_latlon(0.0, 90.0, 1.0), [1, 0, 0], atol=1e-15)
    assert np.allclose(ob.fixed_from_latlon(0.0, 0.0, 1.0), [0, 1, 0], atol=1e-15)
    assert np.allclose(ob.fixed_from_latlon(90.0, 0.0, 1.0), [0, 0, 1], atol=1e-15)
    _, _, U, _, _ = hm.frame(pm.scene(), mc.crater_dem(), lat[:5], lon[:5])
    assert np.abs(ob.fixed_from_latlon(lat[:5], lon[:5], 1.0) - U).max() < 1e-15


def test_fixed_positions_follow_the_moons_spin():
    """An equatorial prograde orbit whose period is the Moon's spin period stays over one longitude; at the epoch the frames
    coincide; a polar orbit's ground track drifts west by the spin rate."""
    a = (ob.GM_MOON * (ob.SPIN_PERIOD_S / (2 * math.pi)) ** 2) ** (1.0 / 3.0)
    el = ob.Elements(a, 0.0, 0.0, 0.0, 0.0, 33.0, T0)
    pos = ob.kepler_fixed_positions(el, T0, 50, 3600.0, j2=False)
    la, lo, r = ob.latlon_from_fixed(pos)
    assert np.abs(la).max() < 1e-9 and np.abs(lo - 33.0).max() < 1e-6 and np.abs(r / a - 1).max() < 1e-12
    el = ob.Elements(2.0e6, 0.0, 90.0, 20.0, 0.0, 0.0, T0)
    pos = ob.kepler_fixed_positions(el, T0 + timedelta(seconds=ob.period_s(2.0e6)), 1, 60.0, j2=False)
    la, lo, _ = ob.latlon_from_fixed(pos)
    assert abs(la[0]) < 1e-6 and abs(lo[0] - (20.0 - math.degrees(ob.SPIN_RATE * ob.period_s(2.0e6)))) < 1e-6


def test_a_satellite_at_the_zenith_stands_at_90_degrees():
    s, dem = pm.scene(), mc.crater_dem()
    lat, lon = np.array([-85.0, 10.0, 60.0]), np.array([30.0, -120.0, 179.0])
    o, _, U, _, _ = hm.frame(s, dem, lat, lon)
    R = float(s.radius)
    hz = np.zeros((3, 8), np.float32)
    for p in range(3):
        X = (o[p] + 0.5 * R * U[p]) / R * pm.RADIUS_M            # 870 km straight up
        info = pm.look(s, dem, lat[p:p + 1], lon[p:p + 1], hz[p:p + 1], X[None, None, :])
        assert abs(info["es"][0, 0, 0] - 90.0) < 1e-5
        assert abs(info["range_m"][0, 0, 0] - 0.5 * pm.RADIUS_M) < 1e-3
        assert info["g"][0, 0, 0] > 89.9


def test_pass_times_place_aos_and_los_between_the_dates():
    from moonrtx_amd._lib import PASS_DTYPE
    recs = np.zeros(2, PASS_DTYPE)
    recs[0] = (0, 0, 10, 5, 12, 0, 0.25, 0.5, 40.0, 2.0e6)
    recs[1] = (0, 1, 0, 3, 1, 1, 0.0, 0.75, 10.0, 3.0e6)
    p = ob.pass_times(recs, T0, 30.0)
    assert p.aos[0] == T0 + timedelta(seconds=(10 - 0.25) * 30.0) and p.los[0] == T0 + timedelta(seconds=(14 + 0.5) * 30.0)
    assert p.aos[1] == T0 and p.los[1] == T0 + timedelta(seconds=2.75 * 30.0)
    assert np.allclose(p.duration_s, [4.75 * 30.0, 2.75 * 30.0])
