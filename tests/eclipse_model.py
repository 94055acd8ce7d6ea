"""float64 model of the Earth's occultation of the Sun, TEST INFRASTRUCTURE, numpy only.

g: per (point, epoch) the directions from horizon_model.frame's lifted origin to the source and to the body of two (m, 14)
epoch tables, their angular radii asin(radius / distance), their separation atan2(|a x b|, a . b), and the planar two-disc
rule restated here from the section (not imported from the package).  summarize: the SUMMARY columns as plain loops.
g_tolerance / sure: what float32 may differ by, derived in g_tolerance's docstring.  designed_tables: epoch tables whose g
at one site is an exact 0, an exact 1 or a robust partial per epoch, as the test chooses.  chunked_summary restates
occultation_kernel's chunk-and-carry walk with named deliberate defects, so that the CPU suite can show that the designed
patterns tell each of those mistakes from a correct walk (tests/test_eclipse_host.py)."""
import math

import numpy as np

import epoch_patterns as ep
import horizon_model as hm

D_ANG = math.radians(5e-5)      # what float32 may move an angle seen from a vertex: horizon_model's f_tolerance figure
ULPS = 16 * 2.0 ** -24          # the rule's own float32 arithmetic on values <= 1
TOTAL, CLEAR, PARTIAL = 0, 1, 2
MUTANTS = ("count_forgets_carried_bit", "start_off_by_chunk", "tie_takes_later", "inactive_lanes_partial", "no_carry")


def two_disc(sep, a_s, a_b):
    """g of DESIGN.md section 3.18 in float64: the share of a disc of radius a_s left uncovered by a disc of radius a_b whose
    centre is sep away (radians; arrays broadcast)."""
    sep, a_s, a_b = np.broadcast_arrays(*(np.asarray(v, np.float64) for v in (sep, a_s, a_b)))
    g = np.empty(sep.shape)
    for i in np.ndindex(sep.shape):
        s, rs, rb = float(sep[i]), float(a_s[i]), float(a_b[i])
        if rs == 0.0:
            g[i] = 1.0 if s > rb else 0.0
        elif s >= rs + rb:
            g[i] = 1.0
        elif rb >= rs and s <= rb - rs:
            g[i] = 0.0
        elif rb < rs and s <= rs - rb:
            g[i] = 1.0 - (rb / rs) ** 2
        else:
            x = min(1.0, max(-1.0, (s * s + rs * rs - rb * rb) / (2.0 * s * rs)))
            y = min(1.0, max(-1.0, (s * s + rb * rb - rs * rs) / (2.0 * s * rb)))
            k2 = (-s + rs + rb) * (s + rs - rb) * (s - rs + rb) * (s + rs + rb)
            area = rs * rs * math.acos(x) + rb * rb * math.acos(y) - 0.5 * math.sqrt(max(0.0, k2))
            g[i] = min(1.0, max(0.0, 1.0 - area / (math.pi * rs * rs)))
    return g


def _moon_frame_points(epochs):
    """(m, 3) light centres relative to the Moon's centre in the Moon frame, and the (m,) radii, of an (m, 14) table."""
    e = np.asarray(epochs, float).reshape(-1, 14)
    L = np.empty((e.shape[0], 3))
    for k, row in enumerate(e):
        ez = row[8:11] / np.linalg.norm(row[8:11])
        v0 = row[11:14] - (row[11:14] @ ez) * ez
        v0 /= np.linalg.norm(v0)
        L[k] = np.stack([np.cross(ez, v0), v0, ez]) @ (row[0:3] - row[5:8])
    return L, e[:, 3].copy()


def geometry(o, src_epochs, body_epochs):
    """(sep, a_s, a_b), each (P, m) radians, from the origins o (P, 3), and a . n helpers: the unit directions a (P, m, 3)."""
    Ls, rs = _moon_frame_points(src_epochs)
    Lb, rb = _moon_frame_points(body_epochs)
    ts, tb = Ls[None] - o[:, None], Lb[None] - o[:, None]
    ds, db = np.sqrt((ts * ts).sum(-1)), np.sqrt((tb * tb).sum(-1))
    a, b = ts / ds[..., None], tb / db[..., None]
    c = np.cross(a, b)
    sep = np.arctan2(np.sqrt((c * c).sum(-1)), (a * b).sum(-1))
    return sep, np.arcsin(np.minimum(1.0, rs[None] / ds)), np.arcsin(np.minimum(1.0, rb[None] / db)), a


def occult_g(scene, dem, lat_deg, lon_deg, src_epochs, body_epochs):
    """(g (P, m) float64, info): the model's g at the points' lifted vertices; info holds sep, a_s, a_b (radians) and mu, the
    cosine of the source's direction against the vertex normal."""
    o, nrm, _, _, _ = hm.frame(scene, dem, lat_deg, lon_deg)
    sep, a_s, a_b, a = geometry(o, src_epochs, body_epochs)
    return vector_two_disc(sep, a_s, a_b), dict(sep=sep, a_s=a_s, a_b=a_b, mu=(a * nrm[:, None]).sum(-1))


def vector_two_disc(sep, a_s, a_b):
    """two_disc for large arrays with a_s > 0: the same cases through numpy (checked against two_disc in the host tests)."""
    sep, a_s, a_b = np.broadcast_arrays(*(np.asarray(v, np.float64) for v in (sep, a_s, a_b)))
    with np.errstate(divide="ignore", invalid="ignore"):
        x = np.clip((sep * sep + a_s * a_s - a_b * a_b) / (2.0 * sep * a_s), -1.0, 1.0)
        y = np.clip((sep * sep + a_b * a_b - a_s * a_s) / (2.0 * sep * a_b), -1.0, 1.0)
        k2 = (-sep + a_s + a_b) * (sep + a_s - a_b) * (sep - a_s + a_b) * (sep + a_s + a_b)
        area = a_s * a_s * np.arccos(x) + a_b * a_b * np.arccos(y) - 0.5 * np.sqrt(np.maximum(0.0, k2))
        g = np.clip(1.0 - area / (np.pi * a_s * a_s), 0.0, 1.0)
        g = np.where((a_b < a_s) & (sep <= a_s - a_b), 1.0 - (a_b / a_s) ** 2, g)
    g = np.where((a_b >= a_s) & (sep <= a_b - a_s), 0.0, g)
    return np.where(sep >= a_s + a_b, 1.0, g)


def g_tolerance(a_s):
    """What the kernel's float32 g may differ from the model's by, per entry, for a source of angular radius a_s (radians).

    The kernel and the model see the same three angles -- sep, a_s, a_b -- up to D_ANG = 5e-5 deg each: the figure the
    horizon stage's f_tolerance uses for an angle formed in float32 from a vertex (the vertex itself, the float32 light
    position and the reciprocal square root together stay well inside it).  g is 1 minus the lens area over pi a_s^2.  Moving
    the body's disc by d(sep) sweeps at most the chord it cuts in the source's disc, which is at most the diameter 2 a_s:
    |dg / d sep| <= 2 a_s / (pi a_s^2) = 2 / (pi a_s).  Growing the body's radius by d(a_b) sweeps the body's arc inside the
    source's disc, again at most a chord of it in width terms, so at most the same; rescaling the source by d(a_s) moves the
    edge it shares with the body by at most that much as well.  Hence 3 x 2 / (pi a_s) x D_ANG, plus ULPS for the rule's own
    float32 arithmetic (a few roundings of values <= 1)."""
    return 3.0 * 2.0 / (np.pi * np.asarray(a_s, float)) * D_ANG + ULPS


def sure(info):
    """(sure_one, sure_zero) masks: the model is farther than the three angle errors from the case boundary, on its g = 1
    side (sep > a_s + a_b) or its g = 0 side (sep < a_b - a_s): float32 must give exactly that value there."""
    sep, a_s, a_b = info["sep"], info["a_s"], info["a_b"]
    return sep - (a_s + a_b) > 3 * D_ANG, (a_b - a_s) - sep > 3 * D_ANG


# ---- SUMMARY as plain loops ----------------------------------------------------------------------------------------------------
def summarize(g):
    """The (P, 8) float64 SUMMARY columns of section 3.18 of FULL values g (P, m): mean, min, share g < 1, share g == 0,
    longest g < 1 run, its first epoch (earliest; -1), longest g == 0 run, number of maximal g < 1 runs."""
    g = np.atleast_2d(np.asarray(g))
    m = g.shape[1]
    out = np.empty((g.shape[0], 8))
    for p, row in enumerate(g):
        part, tot = [bool(v < 1) for v in row], [bool(v == 0) for v in row]
        run_p, first_p = ep._longest(part)
        runs = sum(1 for k in range(m) if part[k] and (k == 0 or not part[k - 1]))
        out[p] = (row.astype(np.float64).sum() / m, row.min(), sum(part) / float(m), sum(tot) / float(m), run_p, first_p,
                  ep._longest(tot)[0], runs)
    return out


# ---- designed tables -----------------------------------------------------------------------------------------------------------
NEAR = 60.0                     # the designed body's distance from the point, scene radii (the source stands at ep.FAR)
SRC_RADIUS_DEG = 0.27


def designed_tables(scene, dem, lat, lon, codes):
    """(source, body) (m, 14) tables for one site: the source stays due north at 40 deg elevation, 0.27 deg in radius, ep.FAR
    radii away; the body, NEAR radii away, is per epoch TOTAL (concentric with the source, 1 deg in radius: g is exactly 0,
    0.73 deg inside the boundary), CLEAR (due east on the horizon, 90 deg away: exactly 1, and unmarked by the host) or
    PARTIAL (5 deg in radius with its centre 5 deg above the source's: the limb crosses the source's centre, g = 0.5 less
    the limb's curvature)."""
    codes = np.asarray(codes)
    o, _, U, N, E = hm.frame(scene, dem, [lat], [lon])
    o, U, N, E = o[0], U[0], N[0], E[0]
    R = float(scene.radius)

    def direction(az_deg, el_deg):
        az, el = np.radians(az_deg), np.radians(el_deg)
        return np.cos(el)[:, None] * (np.cos(az)[:, None] * N + np.sin(az)[:, None] * E) + np.sin(el)[:, None] * U
    m = codes.size
    row = ep.frame_row()
    ez = row[8:11] / np.linalg.norm(row[8:11])
    v0 = row[11:14] - (row[11:14] @ ez) * ez
    v0 /= np.linalg.norm(v0)
    Mf = np.stack([np.cross(ez, v0), v0, ez])
    src, body = np.tile(row, (m, 1)), np.tile(row, (m, 1))
    src[:, 0:3] = row[5:8] + (o + ep.FAR * R * direction(np.zeros(m), np.full(m, 40.0))) @ Mf
    src[:, 3] = ep.FAR * R * math.sin(math.radians(SRC_RADIUS_DEG))
    az = np.where(codes == CLEAR, 90.0, 0.0)
    el = np.where(codes == CLEAR, 0.0, np.where(codes == PARTIAL, 45.0, 40.0))
    body[:, 0:3] = row[5:8] + (o + NEAR * R * direction(az, el)) @ Mf
    body[:, 3] = NEAR * R * np.sin(np.radians(np.where(codes == PARTIAL, 5.0, 1.0)))
    body[:, 4] = 0.0
    return src, body


def designed_codes(m, seed=0):
    """[(name, codes (m,))]: every structured sequence of epoch_patterns as the g < 1 mask, once with every set epoch TOTAL
    and once with TOTAL where the fifth-next structured sequence is set and PARTIAL elsewhere."""
    seqs = ep.structured(m, seed)
    out = []
    for i, (name, seq) in enumerate(seqs):
        other_name, other = seqs[(i + 5) % len(seqs)]
        out.append((f"{name}:total", np.where(seq, TOTAL, CLEAR)))
        if seq.any():
            out.append((f"{name}:total where {other_name}", np.where(seq, np.where(other, TOTAL, PARTIAL), CLEAR)))
    return out


def codes_as_g(codes, partial=0.5):
    """The designed g of a code sequence, PARTIAL epochs at `partial` (any value strictly between 0 and 1 gives the same
    counts, runs and indices)."""
    codes = np.asarray(codes)
    return np.where(codes == TOTAL, 0.0, np.where(codes == CLEAR, 1.0, partial))


# ---- the kernel's scheme, restated, with named defects -------------------------------------------------------------------------
def chunked_summary(g, chunk=64, mutant=None):
    """occultation_kernel's SUMMARY walk in Python integers over FULL values g (P, m): per chunk of `chunk` epochs the masks
    of g < 1 and g == 0 over the valid lanes, their popcounts, per lane the two runs ending there (epoch_patterns'
    _run_ending_here), the carries taken at the last valid lane, the earliest longest g < 1 run kept unless a strictly longer
    one comes, and the run starts: a set lane whose predecessor is unset, lane 0's predecessor being the carried last bit.
    (P, 8) float64 as summarize.

    mutant names one deliberate defect (MUTANTS):
      count_forgets_carried_bit  lane 0's predecessor counts as unset: a run crossing a chunk edge is counted twice;
      start_off_by_chunk         the kept start index lacks the chunk's first epoch k0;
      tie_takes_later            a later chunk's run of the same length replaces the kept one (>= for >);
      inactive_lanes_partial     lanes past m are walked as epochs with g < 1 (they hold g = 1 and must stay out);
      no_carry                   every chunk starts its runs at 0."""
    assert mutant is None or mutant in MUTANTS
    g = np.atleast_2d(np.asarray(g, np.float64))
    m = g.shape[1]
    out = np.empty((g.shape[0], 8))
    for p in range(g.shape[0]):
        total, lo = 0.0, 1.0
        n_p = n_t = n_runs = 0
        cur_p = cur_t = best_p = best_t = 0
        first_p, prev = -1, 0
        for k0 in range(0, m, chunk):
            active = [k0 + lane < m for lane in range(chunk)]
            val = [float(g[p, k0 + lane]) if active[lane] else 1.0 for lane in range(chunk)]
            guard = [True] * chunk if mutant == "inactive_lanes_partial" else active
            part = [guard[lane] and (val[lane] < 1.0 or not active[lane]) for lane in range(chunk)]
            tot = [active[lane] and val[lane] == 0.0 for lane in range(chunk)]
            total += sum(v for v, a in zip(val, active) if a)
            lo = min([lo] + val)
            mp, mt = ep._mask(part), ep._mask(tot)
            n_p += bin(mp).count("1"); n_t += bin(mt).count("1")
            last = min(chunk, m - k0) - 1
            if mutant == "no_carry":
                cur_p = cur_t = 0
            rp = [ep._run_ending_here(mp, lane, guard[lane], cur_p, chunk, None) for lane in range(chunk)]
            rt = [ep._run_ending_here(mt, lane, active[lane], cur_t, chunk, None) for lane in range(chunk)]
            cur_p, cur_t = rp[last], rt[last]
            best_t = max(best_t, max(rt))
            mx = max(rp)
            if mx >= best_p and mx > 0 if mutant == "tie_takes_later" else mx > best_p:
                best_p = mx
                first_p = (0 if mutant == "start_off_by_chunk" else k0) + rp.index(mx) - mx + 1
            before = (mp << 1) | (0 if mutant == "count_forgets_carried_bit" else prev)
            n_runs += bin(mp & ~before & ((1 << chunk) - 1)).count("1")
            prev = (mp >> last) & 1
        out[p] = (total / m, lo, n_p / float(m), n_t / float(m), best_p, first_p, best_t, n_runs)
    return out
