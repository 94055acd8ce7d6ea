"""The orbiter-pass model on the CPU: the float32 emulation of the kernel's operations against the
float64 model within the derived tolerance, the cap on the share of margins too close to zero to compare a sign, and the plain-loop
reductions on sequences whose answer is known."""
import numpy as np

import epoch_patterns as ep
import passes_model as pm
from moonrtx_amd._lib import PASS_DTYPE, PASS_OPEN_END, PASS_OPEN_START


def model_and_tolerance():
    c = pm.case()
    info = pm.look(c["scene"], c["dem"], c["lat"], c["lon"], c["hz"], c["pos"])
    return c, info, pm.tolerances(info, pm.N_AZ)


def test_few_margins_lie_within_the_tolerance_of_zero():
    """The cap condition of the GPU comparison, from the model alone: at most 1 % of the (point, satellite, epoch) entries have
    |g_model| <= tol_g.  Measured share: 0 of 36864 (the smallest |g| / tol_g is 3.65; the case holds 179 passes)."""
    c, info, (d_dir, d_az, tol_g) = model_and_tolerance()
    close = np.abs(info["g"]) <= tol_g
    print(f"{close.sum()} of {close.size} margins within the tolerance of zero; smallest |g| / tol_g "
          f"{(np.abs(info['g']) / tol_g).min():.2f}; tol_g {tol_g.min():.2e} .. {tol_g.max():.2e} deg")
    assert close.mean() <= 0.01
    view = info["g"] > 0
    assert 0.02 < view.mean() < 0.9                             # the case holds satellites above and below the horizon
    n_pass = len(pm.passes(info["g"], info["es"], info["range_m"]))
    print(f"{n_pass} passes")
    assert n_pass >= 100


def test_float32_emulation_stays_within_the_tolerance():
    """The kernel's operations in numpy float32 against the float64 model: es within d_dir, the azimuth within d_az on the
    circle (below 89.9 deg of elevation), the range within passes_model.range_tolerance, g within tol_g, and the same sign of g
    everywhere outside the tolerance."""
    c, info, (d_dir, d_az, tol_g) = model_and_tolerance()
    emu = pm.emulate32(c["scene"], c["dem"], c["lat"], c["lon"], c["hz"], c["pos"])
    e_es = np.abs(emu["es"] - info["es"])
    d = np.abs(emu["az"] - info["az"])
    e_az = np.minimum(d, 360.0 - d)
    low = info["es"] <= 89.9
    e_r = np.abs(emu["range_m"] - info["range_m"])
    e_g = np.abs(emu["g"] - info["g"])
    tol_r = pm.range_tolerance(info, c["scene"])
    print(f"worst error / tolerance: es {(e_es / d_dir).max():.3f}, azimuth {(e_az / d_az)[low].max():.3f}, "
          f"range {(e_r / tol_r).max():.3f}, g {(e_g / tol_g).max():.3f}")
    assert (e_es <= d_dir).all()
    assert (e_az <= d_az)[low].all()
    assert (e_r <= tol_r).all()
    assert (e_g <= tol_g).all()
    sure = np.abs(info["g"]) > tol_g
    assert ((emu["g"] > 0) == (info["g"] > 0))[sure].all()
    # and the records of the emulated table are those of the model's wherever nothing is close: the same passes
    a = pm.passes(emu["g"], emu["es"], emu["range_m"])
    b = pm.passes(info["g"], info["es"], info["range_m"])
    if sure.all():
        for k in ("point", "sat", "first", "count", "flags"):
            assert np.array_equal(a[k], b[k]), k


def table_of(bits, up=10.0, down=-60.0):
    return np.where(np.asarray(bits, bool), np.float32(up), np.float32(down)).astype(np.float32)


def test_reductions_on_designed_sequences():
    """summary and passes against epoch_patterns' own truth for single sequences, at every m of the chunk-edge list."""
    for m in ep.M:
        seqs = ep.structured(m, 0)
        for i, (name, seq) in enumerate(seqs):
            other = seqs[(i + 5) % len(seqs)][1]
            g = np.stack([table_of(seq), table_of(other)])[None]
            es = np.where(g > 0, np.float32(20.0), np.float32(-60.0)).astype(np.float32)
            rm = np.full(g.shape, 2.0e6, np.float32)
            got = pm.summary(g, es)[0]
            any_ = seq | other
            w = ep.expect_windows(any_, any_)[0]
            assert got[0] == w[4] and got[1] == w[7] and got[2] == w[5] and got[3] == w[6], (m, name)
            assert got[4] == np.count_nonzero(any_ & ~np.concatenate([[False], any_[:-1]])), (m, name)
            assert got[5] == (np.float32(20.0) if any_.any() else np.float32(-90.0))
            assert got[6] == np.float32((int(seq.sum()) + int(other.sum())) / float(m))
            assert got[7] == np.float32(int((seq & other).sum()) / float(m))
            recs = pm.passes(g, es, rm)
            for s, bits in enumerate((seq, other)):
                mine = recs[recs["sat"] == s]
                starts = np.flatnonzero(bits & ~np.concatenate([[False], bits[:-1]]))
                ends = np.flatnonzero(bits & ~np.concatenate([bits[1:], [False]]))
                assert np.array_equal(mine["first"], starts) and np.array_equal(mine["count"], ends - starts + 1), (m, name)
                assert np.array_equal(mine["flags"], (starts == 0) * PASS_OPEN_START + (ends == m - 1) * PASS_OPEN_END)
                assert np.array_equal(mine["max_at"], starts)    # equal elevations: the earliest epoch
    assert recs.dtype == PASS_DTYPE and PASS_DTYPE.itemsize == 40


def test_fractions_are_float32_operations():
    g = np.array([[[-0.3, 0.1, 0.7, -0.2, -1.0, 0.25]]], np.float32)
    es = np.array([[[1.0, 5.0, 9.0, 2.0, 0.0, 3.0]]], np.float32)
    rm = np.array([[[5e6, 4e6, 3e6, 3.5e6, 6e6, 7e6]]], np.float32)
    r = pm.passes(g, es, rm)
    assert len(r) == 2
    f = np.float32
    assert r[0]["rise_frac"] == f(0.1) / (f(0.1) - f(-0.3)) and r[0]["set_frac"] == f(0.7) / (f(0.7) - f(-0.2))
    assert r[0]["rise_frac"].dtype == np.float32
    assert (r[0]["first"], r[0]["count"], r[0]["max_at"], r[0]["flags"]) == (1, 2, 2, 0)
    assert r[0]["max_elev_deg"] == f(9.0) and r[0]["min_range_m"] == f(3e6)
    assert r[1]["rise_frac"] == f(0.25) / (f(0.25) - f(-1.0)) and r[1]["set_frac"] == 0 and r[1]["flags"] == PASS_OPEN_END
