"""Designed visibility sequences for the two epoch walkers (DESIGN.md sections 3.9 and 3.15), TEST INFRASTRUCTURE, numpy only.

horizon_sun_kernel (SUMMARY) and horizon_windows_kernel walk the epochs 64 at a time, one lane per epoch, and reduce ballots
across lanes and chunks.  The horizon table is an input, so any 0 / 1 visibility sequence can be forced per point: epoch k of
table A is a far light on the azimuth of horizon sample k at elevation +10 deg, epoch k of table B one on sample n_az / 2 + k,
and row p of the horizon table holds -45 deg where pattern p wants the body visible and +45 deg where it does not.  The
horizon stays 34.73 deg from the disc's edge, which float32 cannot bridge, so every fraction is exactly 0 or 1 and equals the
designed bit; the expected outputs are then plain loops over bits the test chose, with no tolerance and nothing left out.

lights / horizon_rows build the inputs, patterns names the sequences, expect_summary / expect_windows are the truth, and
chunked_windows restates the kernel's chunk-and-carry scheme with named deliberate defects, so that the CPU suite can show
that the patterns tell each of those mistakes from a correct walk (tests/test_epoch_patterns_host.py)."""
import functools
from datetime import datetime, timezone

import numpy as np

import horizon_model as hm

FAR = 2.0e4                     # the lights' distance from the point, in scene radii
UP, DOWN = -45.0, 45.0          # horizon elevation (degrees) where the body is to be visible / hidden
M = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 512)      # the epoch counts of the chunk-edge tests
MUTANTS = ("carry_from_lane_63", "no_carry", "tie_takes_later", "inactive_lanes_unset", "lane63_mask", "start_off_by_chunk")


@functools.lru_cache(maxsize=None)
def frame_row():
    """One row of ephemeris.sun_epochs: the Moon frame (centre, u, v) every designed epoch copies."""
    from moonrtx_amd import ephemeris as E
    return E.sun_epochs([datetime(2025, 3, 1, tzinfo=timezone.utc)], E.Observer(52.2, 21.0, 0.0))[0]


def lights(scene, dem, lat, lon, sectors, n_az, elev_deg=10.0, radius_deg=0.27):
    """(m, 14) float64 epochs (MrtxIllumEpoch rows): epoch k is a light FAR scene radii from the lifted origin of (lat, lon),
    on the azimuth of horizon sample sectors[k] (fractional values lie between samples) at elevation elev_deg (one value or
    one per epoch), of angular radius radius_deg (0: a point light).  Position: center + M^T (o + dist d), with d from
    horizon_model.frame's N, E, U and M the Moon frame of frame_row()."""
    o, _, U, N, E = hm.frame(scene, dem, [lat], [lon])
    o, U, N, E = o[0], U[0], N[0], E[0]
    sectors = np.atleast_1d(np.asarray(sectors, np.float64))
    phi = 2.0 * np.pi * sectors / float(n_az)
    e = np.radians(np.broadcast_to(np.asarray(elev_deg, np.float64), sectors.shape))
    d = np.cos(e)[:, None] * (np.cos(phi)[:, None] * N + np.sin(phi)[:, None] * E) + np.sin(e)[:, None] * U
    dist = FAR * float(scene.radius)
    row = frame_row()
    ez = row[8:11] / np.linalg.norm(row[8:11])
    v0 = row[11:14] - (row[11:14] @ ez) * ez
    v0 /= np.linalg.norm(v0)
    Mf = np.stack([np.cross(ez, v0), v0, ez])
    ep = np.tile(row, (sectors.size, 1))
    ep[:, 0:3] = row[5:8] + (o + dist * d) @ Mf            # rows of (o + dist d) times M = M^T applied to each
    ep[:, 3] = dist * np.sin(np.radians(float(radius_deg)))
    return ep


def horizon_rows(bits_a, bits_b, n_az):
    """The (P, n_az) float32 horizon table of P patterns of m <= n_az / 2 epochs: sample k carries bits_a[:, k] and sample
    n_az / 2 + k carries bits_b[:, k] (UP where the bit is set, DOWN elsewhere and at the samples no epoch looks at)."""
    a, b = np.atleast_2d(np.asarray(bits_a, bool)), np.atleast_2d(np.asarray(bits_b, bool))
    assert a.shape == b.shape and 2 * a.shape[1] <= n_az
    hz = np.full((a.shape[0], n_az), DOWN, np.float32)
    hz[:, :a.shape[1]] = np.where(a, UP, DOWN)
    hz[:, n_az // 2:n_az // 2 + a.shape[1]] = np.where(b, UP, DOWN)
    return hz


def sectors_of(m, n_az):
    """The horizon samples the epochs of table A and of table B look at."""
    return np.arange(m), n_az // 2 + np.arange(m)


# ---- the sequences -------------------------------------------------------------------------------------------------------------
def _run(m, *spans):
    """m bits with 1s over each [s, s + L) (clipped to m), or None if a span is empty or starts past m."""
    seq = np.zeros(m, bool)
    for s, L in spans:
        if L <= 0 or s < 0 or s >= m:
            return None
        seq[s:s + L] = True
    return seq


def _whole(m, *spans):
    """_run, dropped (None) unless every span fits: a tie clipped at m is no tie."""
    return _run(m, *spans) if all(L > 0 and 0 <= s and s + L <= m for s, L in spans) else None


def structured(m, seed):
    """The named structured sequences of m bits, identical ones (short m) listed once under their first name."""
    rng = np.random.default_rng([seed, m])
    seqs = [("all0", np.zeros(m, bool)), ("all1", np.ones(m, bool))]
    for k in (0, 62, 63, 64, 65, m - 1):
        seqs.append((f"one1@{k}", _run(m, (k, 1))))
        seqs.append((f"one0@{k}", None if k >= m else ~_run(m, (k, 1))))
    for s, L in ((0, 64), (64, 64), (1, 63), (1, 64), (63, 2), (60, 70), (0, m - 1), (1, m - 1)) + \
            tuple((m - L, L) for L in (1, 63, 64, 65)):
        seqs.append((f"run[{s},{s + L})", _run(m, (s, L))))
    # two equal longest runs a single 0 apart: both in chunk 0; the first across 63|64 and the second filling chunk 2 (a
    # single 0 apart, a second run inside a later chunk than the one the first ends in is 64 long); the first across 63|64
    # and the second in the chunk it ends in; the first in chunk 0 and the second across 63|64 (its part in chunk 0 is
    # shorter than the first run)
    seqs.append(("tie:chunk0", _whole(m, (2, 10), (13, 10))))
    seqs.append(("tie:straddle-then-later", _whole(m, (63, 64), (128, 64))))
    seqs.append(("tie:straddle-then-same", _whole(m, (59, 10), (70, 10))))
    seqs.append(("tie:chunk0-then-straddle", _whole(m, (40, 12), (53, 12))))
    seqs.append(("tie:short", _whole(m, (0, 1), (2, 1))))
    seqs.append(("L-then-L+1:chunk0", _whole(m, (3, 5), (20, 6))))
    seqs.append(("L-then-L+1:chunks", _whole(m, (10, 10), (100, 11))))
    seqs.append(("1010", np.arange(m) % 2 == 0))
    seqs.append(("0101", np.arange(m) % 2 == 1))
    seqs.append(("lane63", np.arange(m) % 64 == 63))
    seqs.append(("lane0", np.arange(m) % 64 == 0))
    for dens in (0.05, 0.5, 0.95):
        seqs.append((f"random{dens}", rng.random(m) < dens))
    out, seen = [], set()
    for name, seq in seqs:
        if seq is None or seq.tobytes() in seen:
            continue
        seen.add(seq.tobytes())
        out.append((name, seq))
    return out


def patterns(m, seed=0):
    """The named (bits_a, bits_b) pairs of m epochs: [(name, bits_a, bits_b)].  Each structured sequence appears as
    (A = seq, B = all 1), as (A = all 1, B = seq) and as (A = seq, B = another structured sequence)."""
    seqs = structured(m, seed)
    ones = np.ones(m, bool)
    out, seen = [], set()
    for i, (name, seq) in enumerate(seqs):
        other_name, other = seqs[(i + 5) % len(seqs)]
        for pair in ((f"A={name},B=all1", seq, ones), (f"A=all1,B={name}", ones, seq), (f"A={name},B={other_name}", seq, other)):
            key = pair[1].tobytes() + pair[2].tobytes()
            if key not in seen:                                 # a pair that a short m makes twice is listed once
                seen.add(key)
                out.append(pair)
    return out


def stack(pats):
    """(names, bits_a (P, m), bits_b (P, m)) of a patterns() list."""
    return [p[0] for p in pats], np.stack([p[1] for p in pats]), np.stack([p[2] for p in pats])


# ---- the truth: plain loops over bits ------------------------------------------------------------------------------------------
def _longest(bits):
    """(length, first index) of the earliest longest run of True; (0, -1) if there is none."""
    best, start, cur = 0, -1, 0
    for i, v in enumerate(bits):
        cur = cur + 1 if v else 0
        if cur > best:
            best, start = cur, i - cur + 1
    return best, start


def expect_summary(bits):
    """The (P, 4) float32 SUMMARY columns of DESIGN.md 3.9 for fractions that are exactly the bits: the mean and both shares
    are float32(count / m), the dark run is the longest run of 0."""
    bits = np.atleast_2d(np.asarray(bits, bool))
    m = bits.shape[1]
    out = np.empty((bits.shape[0], 4), np.float32)
    for p, row in enumerate(bits):
        share = np.float32(int(row.sum()) / m)
        out[p] = (share, share, share, _longest([not v for v in row])[0])
    return out


def expect_windows(bits_a, bits_b):
    """The (P, 8) float32 columns of DESIGN.md 3.15 for ok_a = bits_a, ok_b = bits_b."""
    a, b = np.atleast_2d(np.asarray(bits_a, bool)), np.atleast_2d(np.asarray(bits_b, bool))
    m = a.shape[1]
    out = np.empty((a.shape[0], 8), np.float32)
    for p in range(a.shape[0]):
        ra, rb = [bool(v) for v in a[p]], [bool(v) for v in b[p]]
        both = [x and y for x, y in zip(ra, rb)]
        run, first = _longest(both)
        out[p] = (np.float32(sum(ra) / float(m)), _longest([not v for v in ra])[0],
                  np.float32(sum(rb) / float(m)), _longest([not v for v in rb])[0],
                  np.float32(sum(both) / float(m)), run, first, _longest([not v for v in both])[0])
    return out


# ---- the kernel's scheme, restated, with named defects -------------------------------------------------------------------------
def _mask(flags):
    return sum(1 << i for i, v in enumerate(flags) if v)


def _run_ending_here(set_mask, lane, active, cur, chunk, mutant):
    """horizon_windows_kernel's run_ending_here: the run of set lanes ending at `lane`, back to the nearest unset lane at or
    below it, or through the chunk's start into the carried run `cur`; 0 for a lane past the last epoch."""
    below = (2 << lane) - 1
    if mutant == "lane63_mask" and lane == chunk - 1:
        below >>= 1                                             # the top lane's own bit is lost
    brk = ~set_mask & below
    run = lane - (brk.bit_length() - 1) if brk else lane + 1 + cur
    return run if active else 0


def chunked_windows(bits_a, bits_b, chunk=64, mutant=None, carries=False):
    """horizon_windows_kernel's walk in Python integers: per chunk of `chunk` epochs the masks of ok_a, ok_b and the valid
    lanes, their popcounts, per lane the four runs ending there, the carries taken at the last valid lane, the maxima, and the
    earliest longest `both` run kept unless a strictly longer one comes.  (P, 8) float32, as expect_windows.

    mutant names one deliberate defect (MUTANTS):
      carry_from_lane_63    the carries are read from the top lane, not from the last valid lane;
      no_carry              every chunk starts its runs at 0;
      tie_takes_later       a later chunk's `both` run of the same length replaces the kept one (>= for >);
      inactive_lanes_unset  lanes past m are walked as epochs that are "not ok": neither the valid mask nor the lane's own
                            guard keeps them out of the three complement runs (either one alone suffices, so a defect that
                            shows has lost both);
      lane63_mask           the top lane's `below` mask lacks its own bit;
      start_off_by_chunk    the kept start index lacks the chunk's first epoch k0.
    carries=True also returns the (P, 4) carries left after the last chunk, which no output reads."""
    assert mutant is None or mutant in MUTANTS
    a, b = np.atleast_2d(np.asarray(bits_a, bool)), np.atleast_2d(np.asarray(bits_b, bool))
    m = a.shape[1]
    out = np.empty((a.shape[0], 8), np.float32)
    left = np.empty((a.shape[0], 4), np.int64)
    for p in range(a.shape[0]):
        n_a = n_b = n_ab = 0
        cur = [0, 0, 0, 0]                                      # !ok_a, !ok_b, both, !both
        best = [0, 0, 0, 0]
        first_ab = -1
        for k0 in range(0, m, chunk):
            active = [k0 + lane < m for lane in range(chunk)]
            ok_a = [active[lane] and bool(a[p, k0 + lane]) for lane in range(chunk)]
            ok_b = [active[lane] and bool(b[p, k0 + lane]) for lane in range(chunk)]
            ma, mb, valid = _mask(ok_a), _mask(ok_b), _mask(active)
            if mutant == "inactive_lanes_unset":
                valid = (1 << chunk) - 1
            mab = ma & mb
            n_a += bin(ma).count("1"); n_b += bin(mb).count("1"); n_ab += bin(mab).count("1")
            last = (chunk if mutant == "carry_from_lane_63" else min(chunk, m - k0)) - 1
            if mutant == "no_carry":
                cur = [0, 0, 0, 0]
            sets = (valid & ~ma, valid & ~mb, mab, valid & ~mab)
            runs = []
            for j, s in enumerate(sets):
                guard = [True] * chunk if mutant == "inactive_lanes_unset" and j != 2 else active
                runs.append([_run_ending_here(s, lane, guard[lane], cur[j], chunk, mutant) for lane in range(chunk)])
            cur = [runs[j][last] for j in range(4)]
            for j in (0, 1, 3):
                best[j] = max(best[j], max(runs[j]))
            mx = max(runs[2])
            if mx >= best[2] if mutant == "tie_takes_later" else mx > best[2]:
                at = runs[2].index(mx)                           # the lowest lane that ends a run of mx
                best[2] = mx
                first_ab = (0 if mutant == "start_off_by_chunk" else k0) + at - mx + 1
        out[p] = (np.float32(n_a / float(m)), best[0], np.float32(n_b / float(m)), best[1], np.float32(n_ab / float(m)),
                  best[2], first_ab, best[3])
        left[p] = cur
    return (out, left) if carries else out
