"""Model of the site power budget (DESIGN.md sections 3.17 and 4.19), TEST INFRASTRUCTURE: numpy and Python ints, no GPU.

budget() is the reference of every SUMMARY column: plain loops over Python ints, straight from the formulas of 3.17.
panel_factor() is the float64 cosine factor of the three panels from horizon_model.frame; quantise() the host's float32
rounding of a table of watts to counts.  sequences() names the designed integer series e_k the GPU test forces through the
kernel, and chunked_budget() restates the kernel's chunk-and-carry walk (64 lanes per chunk) with named deliberate defects, so
that the CPU suite can show that the sequences tell each of those mistakes from a correct walk (tests/test_power_host.py)."""
import numpy as np

import horizon_model as hm
from moonrtx_amd.renderer import MoonRT

PANELS_BY_NAME = MoonRT.PANELS          # the header's MRTX_PANEL_* by name
TRACK, FIXED, AZIMUTH = (PANELS_BY_NAME[k] for k in ("track", "fixed", "azimuth"))
BIG = 1 << 28                   # the largest count a table entry may hold
# (capacity, initial) of the calls every designed sequence runs under: a small battery starting partly charged, one starting
# empty, none at all, the largest one the ABI takes, and one that the sequences of unit steps fill and empty
CONFIGS = ((37, 11), (1000, 0), (0, 0), (1 << 52, 1 << 52), (1000, 1000))
MUTANTS = ("no_S_carry", "no_peak_carry", "peak_tie_takes_earlier", "drawdown_tie_takes_later", "accumulate_32_bit",
           "clamp_order_swapped", "inactive_lanes_with_peak", "carry_from_lane_63")


# ---- the truth: plain loops over Python ints -----------------------------------------------------------------------------------
def budget(e, capacity, initial, g=None):
    """The eight SUMMARY columns of DESIGN.md 3.17 as Python ints for the integer series e (e_k = G_k - L_k), a battery of
    `capacity` counts holding `initial` before epoch 0.  g: the generated counts G_k of column [0] (default max(e_k, 0), the
    designed sequences' split of e into generation and load)."""
    e = [int(x) for x in e]
    g = [max(x, 0) for x in e] if g is None else [int(x) for x in g]
    capacity, initial = int(capacity), int(initial)
    S = 0
    peak, peak_at = 0, -1                                       # max_{-1 <= i < j} S_i and the latest i that attains it
    D, first, last = 0, -1, -1
    s = initial
    min_s, n_unmet, unmet = None, 0, 0
    for j, x in enumerate(e):
        S += x
        if peak - S > D:                                        # strictly: the smallest j that attains D
            D, first, last = peak - S, peak_at + 1, j
        if S >= peak:                                           # equal: the later index
            peak, peak_at = S, j
        t = s + x
        s = min(capacity, max(0, t))
        min_s = s if min_s is None else min(min_s, s)
        if t < 0:
            n_unmet += 1
            unmet += -t
    return [sum(g), S, D, first, last, min_s, n_unmet, unmet]


def budgets(e_rows, capacity, initial, g_rows=None):
    """budget() of every row, (P, 8) int64."""
    return np.array([budget(row, capacity, initial, None if g_rows is None else g_rows[p]) for p, row in enumerate(e_rows)],
                    np.int64).reshape(len(e_rows), 8)


# ---- float64 panel factors and the host's quantisation ---------------------------------------------------------------------------
def sun_direction(scene, dem, lat_deg, lon_deg, epochs):
    """(xe, xn, xu), each (P, m): the unit direction to the light centre from each point's lifted origin in its (E, N, U)."""
    o, _, U, N, E = hm.frame(scene, dem, lat_deg, lon_deg)
    ep = np.asarray(epochs, float).reshape(-1, 14)
    Lb = np.empty((ep.shape[0], 3))
    for k, row in enumerate(ep):
        ez = row[8:11] / np.linalg.norm(row[8:11])
        v0 = row[11:14] - (row[11:14] @ ez) * ez
        v0 /= np.linalg.norm(v0)
        Lb[k] = np.stack([np.cross(ez, v0), v0, ez]) @ (row[0:3] - row[5:8])
    t = Lb[None, :, :] - o[:, None, :]
    l = t / np.sqrt((t * t).sum(-1))[..., None]
    return (l * E[:, None, :]).sum(-1), (l * N[:, None, :]).sum(-1), (l * U[:, None, :]).sum(-1)


def panel_factor(scene, dem, lat_deg, lon_deg, epochs, panel, normal_enu=None):
    """(P, m) float64 cosine factor c of DESIGN.md 3.17: 1 (TRACK), max(0, n . l) (FIXED), min(1, |l's horizontal part|)
    (AZIMUTH)."""
    xe, xn, xu = sun_direction(scene, dem, lat_deg, lon_deg, epochs)
    if panel == TRACK:
        return np.ones_like(xe)
    if panel == FIXED:
        n = np.asarray(normal_enu, float)
        n = n / np.linalg.norm(n)
        return np.maximum(0.0, n[0] * xe + n[1] * xn + n[2] * xu)
    return np.minimum(1.0, np.hypot(xe, xn))


def quantise(watts, cpw_log2):
    """(int32)rintf((float)w * 2^cpw_log2) per entry: the host's L_k (round to nearest, ties to even)."""
    scaled = np.asarray(watts, np.float64).astype(np.float32) * np.float32(2.0 ** int(cpw_log2))
    return np.rint(scaled).astype(np.int64)


def split(e):
    """(gen_w, load_w) float64 tables that make e_k at cpw_log2 = 0, f = 1 and a tracking panel: max(e, 0) and max(-e, 0)."""
    e = np.asarray(e, np.int64)
    assert np.abs(e).max(initial=0) <= BIG
    assert np.array_equal(e.astype(np.float32).astype(np.int64), e), "an entry is not a float32: the call would round it"
    return np.maximum(e, 0).astype(np.float64), np.maximum(-e, 0).astype(np.float64)


# ---- the designed sequences --------------------------------------------------------------------------------------------------------
def _put(m, default, *items):
    """m entries of `default` with (index, value) items written over them; None if an index does not fit."""
    e = np.full(m, default, np.int64)
    for k, v in items:
        if not 0 <= k < m:
            return None
        e[k] = v
    return e


def sequences(m, seed=0):
    """The named designed series of m epochs, [(name, e (m,) int64)], |e_k| <= 2^28; a series that needs more epochs than m is
    left out, identical ones (short m) are listed once.  Every entry is exactly representable in float32, the format in which
    the call reads its tables of watts."""
    rng = np.random.default_rng([seed, m, 17])
    k = np.arange(m)
    out = [("zero", np.zeros(m, np.int64)), ("all+3", np.full(m, 3, np.int64)), ("all-3", np.full(m, -3, np.int64))]
    # the peak at lane 63, the trough at lane 64
    out.append(("peak@63,trough@64", None if m < 66 else np.where(k < 64, 5, np.where(k == 64, -400, 1))))
    # one drawdown over three chunks: up to epoch 9, down to epoch 149, up again
    out.append(("drawdown-3-chunks", None if m < 160 else np.where(k < 10, 10, np.where(k < 150, -1, 3))))
    # the two tie rules, within a chunk and across chunks
    out.append(("equal-drawdowns:chunk0", _put(m, 0, (2, 5), (3, -5), (6, 5), (7, -5))))
    out.append(("equal-drawdowns:chunks", _put(m, 0, (2, 5), (3, -5), (70, 5), (71, -5), (130, 5), (131, -5))))
    out.append(("equal-drawdowns:edge", _put(m, 0, (2, 5), (3, -5), (63, 5), (64, -5))))
    out.append(("equal-peaks:chunk0", _put(m, 0, (1, 5), (2, -2), (4, 2), (6, -4))))
    out.append(("equal-peaks:chunks", _put(m, 0, (1, 5), (2, -2), (70, 2), (80, -4))))
    out.append(("equal-peaks:edge", _put(m, 0, (1, 5), (62, -2), (63, 2), (64, -4))))
    out.append(("equal-peaks:start", _put(m, 0, (0, -1), (1, 1), (2, -3))))        # S_-1 = 0 against S_1 = 0
    out.append(("alternate+5-5", np.where(k % 2 == 0, 5, -5)))
    # the clamp at both bounds inside a chunk and across the edge 63 | 64
    out.append(("clamp:chunk0", _put(m, 0, (1, 2000), (2, -3000), (3, 7), (4, -2), (5, 2000), (6, -1990))))
    out.append(("clamp:edge", _put(m, 1, (62, 2000), (63, -3), (64, -3000), (65, 4))))
    out.append(("clamp:saw", np.where(k % 7 == 3, 30, -5)))
    # the largest entries: the sums pass 2^32 after 16 epochs
    out.append(("all-2^28", np.full(m, -BIG, np.int64)))
    out.append(("up-then-down-2^28", np.where(k < m // 2, BIG, -BIG)))
    out.append(("alternate-2^28", np.where(k % 2 == 0, -BIG, BIG)))
    # the drawdown that ends in the last epoch (a last chunk of one lane at m = 64 j + 1)
    out.append(("last-epoch-trough", _put(m, 2, (m - 1, -1000))))
    out.append(("last-epoch-peak", _put(m, -2, (m - 1, 1000))))
    for dens in (0.05, 0.5, 0.95):
        sign = np.where(rng.random(m) < dens, 1, -1)
        out.append((f"random{dens}", sign * rng.integers(0, 40, m)))
        # up to 2^28 in steps of 32: every value a float32, so that the tables of watts hold it exactly
        out.append((f"random{dens}:big", sign * (rng.integers(0, (BIG >> 5) + 1, m) << 5)))
    res, seen = [], set()
    for name, e in out:
        if e is None:
            continue
        e = np.ascontiguousarray(e, np.int64)
        assert e.shape == (m,) and np.abs(e).max() <= BIG, name
        if e.tobytes() not in seen:
            seen.add(e.tobytes())
            res.append((name, e))
    return res


def stack(seqs):
    """(names, e (P, m) int64) of a sequences() list."""
    return [s[0] for s in seqs], np.stack([s[1] for s in seqs])


# ---- the kernel's scheme, restated, with named defects -------------------------------------------------------------------------
def _wrap32(x):
    return (int(x) + (1 << 31)) % (1 << 32) - (1 << 31)


def _compose(f, g):
    """g after f for clamp functions (a, lo, hi): x -> min(hi, max(lo, x + a))."""
    fa, flo, fhi = f
    ga, glo, ghi = g
    return fa + ga, min(ghi, max(glo, flo + ga)), min(ghi, max(glo, fhi + ga))


def chunked_budget(e, capacity, initial, chunk=64, mutant=None, carries=False):
    """power_budget_kernel's walk in Python ints: per chunk of `chunk` epochs the inclusive add scan of e on the carried
    balance, the peak of the balance before each lane (value and index; equal values keep the later index) seeded with the
    carried peak, the chunk's largest drawdown at its lowest lane (kept only when strictly greater than the one held), the
    clamp functions composed lane by lane and applied to the carried state of charge, the sums, the count and the minimum,
    and the carries taken at the last valid lane.  Lanes past the last epoch hold e = 0, no peak, no drawdown and no count.
    Returns the eight columns of budget().

    mutant names one deliberate defect (MUTANTS):
      no_S_carry                 every chunk starts its balance at 0;
      no_peak_carry              every chunk starts its peak at the balance it starts from, forgetting the higher ones before;
      peak_tie_takes_earlier     of equal peaks the earlier index is kept;
      drawdown_tie_takes_later   an equal drawdown replaces the one held, and the highest lane of a chunk is taken (>= for >);
      accumulate_32_bit          the balance and the sums wrap at 32 bits;
      clamp_order_swapped        the clamp functions are composed earlier-after-later;
      inactive_lanes_with_peak   lanes past m are walked as epochs with e = 0: they take part in the peak, the drawdown, the
                                 minimum and the count;
      carry_from_lane_63         the carries are read from the top lane, not from the last valid lane.
    carries=True also returns the carries left after the last chunk (S, peak, peak index, s), which no output reads."""
    assert mutant is None or mutant in MUTANTS
    e = [int(x) for x in e]
    m = len(e)
    capacity = int(capacity)
    w = _wrap32 if mutant == "accumulate_32_bit" else int
    sum_g = unmet = n_unmet = 0
    min_s = None
    S_c, pk_c, pki_c, s_c = 0, 0, -1, int(initial)
    D, first, last_j = 0, -1, -1
    for k0 in range(0, m, chunk):
        if mutant == "no_S_carry":
            S_c = 0
        if mutant == "no_peak_carry":
            pk_c, pki_c = S_c, k0 - 1
        active = [k0 + lane < m for lane in range(chunk)]
        walked = [True] * chunk if mutant == "inactive_lanes_with_peak" else active
        ek = [e[k0 + lane] if active[lane] else 0 for lane in range(chunk)]
        # the inclusive add scan on the carried balance
        S, run = [], S_c
        for lane in range(chunk):
            run = w(run + ek[lane])
            S.append(run)
        # the peak up to and including each lane, then the one before each lane with the carry
        incl, best = [], None
        for lane in range(chunk):
            if walked[lane]:
                here = (S[lane], k0 + lane)
                if best is None or (here[0] > best[0] if mutant == "peak_tie_takes_earlier" else here[0] >= best[0]):
                    best = here
            incl.append(best)
        before = []
        for lane in range(chunk):
            x = incl[lane - 1] if lane > 0 else None
            keep_carry = x is None or (pk_c >= x[0] if mutant == "peak_tie_takes_earlier" else pk_c > x[0])
            before.append((pk_c, pki_c) if keep_carry else x)
        d = [before[lane][0] - S[lane] if walked[lane] else -1 for lane in range(chunk)]
        mx = max(d)
        if mx >= D if mutant == "drawdown_tie_takes_later" else mx > D:
            at = [lane for lane in range(chunk) if d[lane] == mx]
            jl = at[-1] if mutant == "drawdown_tie_takes_later" else at[0]
            D, last_j, first = mx, k0 + jl, before[jl][1] + 1
        # the clamps composed, each applied to the carried state of charge
        F, sk = None, []
        for lane in range(chunk):
            own = (ek[lane], 0, capacity)
            if F is None:
                F = own
            else:
                F = _compose(own, F) if mutant == "clamp_order_swapped" else _compose(F, own)
            sk.append(min(F[2], max(F[1], s_c + F[0])))
        for lane in range(chunk):
            t = (sk[lane - 1] if lane > 0 else s_c) + ek[lane]
            if walked[lane]:
                min_s = sk[lane] if min_s is None else min(min_s, sk[lane])
                if t < 0:
                    n_unmet += 1
                    unmet = w(unmet - t)
            if active[lane]:
                sum_g = w(sum_g + max(ek[lane], 0))
        last = (chunk if mutant == "carry_from_lane_63" else min(chunk, m - k0)) - 1
        S_c, s_c = S[last], sk[last]
        if incl[last] is not None and not (pk_c >= incl[last][0] if mutant == "peak_tie_takes_earlier" else pk_c > incl[last][0]):
            pk_c, pki_c = incl[last]
    cols = [sum_g, S_c, D, first, last_j, min_s, n_unmet, unmet]
    return (cols, (S_c, pk_c, pki_c, s_c)) if carries else cols
