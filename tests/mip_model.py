"""Plain numpy builders of the five device structures every march trusts, written from their DEFINITIONS (DESIGN.md section
4.23), and the covering invariants their consumers rely on.

Everything is a copy or a maximum of float32 values (with zero, the neutral element the builders start from: D > 0), so a
device structure must equal its model bit for bit.  Windows are written in UNWRAPPED texel coordinates: a row index of any
sign clamps into [0, h-1], a column index of any sign wraps modulo w; nothing here knows about the seam.

    Dp(r, c) = D[clip(r, 0, h-1), c mod w]

The invariants (check_A, check_B, check_H) are derived from what the consumers INDEX (seg_anchors, first_/last_kept_step,
horizon_cell / horizon_kend), independently of how a builder loops: each returns the list of violated cells, empty = holds.
"""
import math

import numpy as np


# ---- the host-side shift rule (ensure_mip) -----------------------------------------------------------------------------
def shifts(h, w, radius, step):
    """(mip_shift, m2_shift, hm_shift) for a DEM of (h, w) texels on a sphere of `radius`, marched in steps of `step` (the
    float32 parameter, taken as a double): a 16-step segment plus its tap margins must fit one cell,
    cell = 2^shift >= 16 step / texel + 3.5, cells of 16 .. 1024 texels; the medium mip's cells are a quarter of that (never
    below 4 texels), the horizon mip's eight times."""
    texel = min(math.pi * float(radius) / h, 2.0 * math.pi * float(radius) / w)
    span = 16.0 * float(np.float32(step)) / texel + 3.5
    s = 4
    while (1 << s) < span and s < 10:
        s += 1
    return s, max(s - 2, 2), s + 3


def cdiv(a, b):
    return -(-a // b)


def mip_info(h, w, radius, step):
    """What mrtx_mip_info reports: (mip_shift, mip_h, mip_w, m2_shift, m2_h, m2_w, hm_shift, hm_h, hm_w)."""
    out = []
    for s in shifts(h, w, radius, step):
        out += [s, cdiv(h, 1 << s), cdiv(w, 1 << s)]
    return tuple(out)


# ---- unwrapped access --------------------------------------------------------------------------------------------------
def window(D, r0, r1, c0, c1):
    """D over the inclusive unwrapped window rows [r0, r1] x columns [c0, c1]: rows clamp, columns wrap."""
    rows = np.clip(np.arange(r0, r1 + 1), 0, D.shape[0] - 1)
    return np.take(np.take(D, rows, axis=0), np.arange(c0, c1 + 1), axis=1, mode="wrap")


# ---- 1, 2: the row-pair copies -----------------------------------------------------------------------------------------
def padded_dem(D):
    """(h+4, w+4, 2) float32: element (r+2, c+2) = (Dp(r, c), Dp(r+1, c)) for r in [-2, h+1], c in [-2, w+1]."""
    h, w = D.shape
    return np.stack([window(D, -2, h + 1, -2, w + 1), window(D, -1, h + 2, -2, w + 1)], -1)


def colour_pairs(T):
    """(h+1, w+4, 2) uint32 from the (h, w, 4) RGBA8 map (a texel = its four bytes as one little-endian word): element
    (r+1, c+2) = (Tp(r, c), Tp(r+1, c)) for r in [-1, h-1], c in [-2, w+1]."""
    t = np.ascontiguousarray(T, np.uint8).view("<u4")[..., 0]
    h, w = t.shape
    return np.stack([window(t, -1, h - 1, -2, w + 1), window(t, 0, h, -2, w + 1)], -1)


# ---- 3, 4: the max-mips ------------------------------------------------------------------------------------------------
def mip_cells(D, shift):
    """(mh, mw) float32, cells of C = 2^shift texels: cell (i, j) = max(0, Dp over rows [C i - 2, min(C i + C + 1, h + 1)] x
    columns [C j - 2, min(C j + C + 1, w + 1)]) -- the cell's own texels dilated by the two-texel tap border, and never
    beyond the padded DEM's last row and column."""
    h, w = D.shape
    C = 1 << shift
    mh, mw = cdiv(h, C), cdiv(w, C)
    rows = np.zeros((mh, w), np.float32)
    for i in range(mh):
        rows[i] = window(D, C * i - 2, min(C * i + C + 1, h + 1), 0, w - 1).max(0)
    out = np.zeros((mh, mw), np.float32)
    for j in range(mw):
        out[:, j] = np.take(rows, np.arange(C * j - 2, min(C * j + C + 1, w + 1) + 1), axis=1, mode="wrap").max(1)
    return np.maximum(out, np.float32(0.0))


def bordered(M):
    """(mh+2, mw+2): element (i+1, j+1) = M(clip(i), j mod mw) for i in [-1, mh], j in [-1, mw] -- the one-cell border clamps
    in the rows and wraps in the columns, like the DEM's."""
    return window(M, -1, M.shape[0], -1, M.shape[1])


def row_pairs(S):
    """(rows, pitch, 2): element (a, b) = (S[a, b], S[a+1, b]), the last row paired with itself."""
    return np.stack([S, window(S, 1, S.shape[0], 0, S.shape[1] - 1)], -1)


def max_mip(D, shift):
    """MRTX_BUF_MIP: the bordered max-mip in row pairs, (mh+2, mw+2, 2)."""
    return row_pairs(bordered(mip_cells(D, shift)))


def medium_mip(D, m2_shift):
    """MRTX_BUF_MIP2: the bordered medium max-mip, plain floats, (m2_h+2, m2_w+2)."""
    return bordered(mip_cells(D, m2_shift))


# ---- 5: the horizon mip ------------------------------------------------------------------------------------------------
def horizon_mip(D, shift, M=None, seam_bug=False):
    """MRTX_BUF_HMIP, (hh, hw) float32, cells of Cc = 2^(shift+3) texels: cell (i, j) = max(0, the max-mip cells (fi, fj) that
    the texels of rows [Cc i - Cc, Cc i + 2 Cc) (clamped) x columns [Cc j - Cc, Cc j + 2 Cc) (wrapped) lie in), fi = r >> shift
    and fj = c >> shift of the clamped / wrapped texel.  M = the max-mip cells to take (default: mip_cells(D, shift)).

    seam_bug = True restates the builder's former defect, for the regression test only: the columns were visited in steps of a
    fine cell from the window's first one, so across the seam the last, PARTIAL fine cell (w % C != 0) was never reached."""
    h, w = D.shape
    C, Cc = 1 << shift, 1 << (shift + 3)
    M = mip_cells(D, shift) if M is None else M
    hh, hw = cdiv(h, Cc), cdiv(w, Cc)
    out = np.zeros((hh, hw), np.float32)
    for i in range(hh):
        fi = np.unique(np.clip(np.arange(Cc * i - Cc, Cc * i + 2 * Cc), 0, h - 1) >> shift)
        for j in range(hw):
            cols = np.arange(Cc * j - Cc, Cc * j + 2 * Cc, C if seam_bug else 1)
            fj = np.unique(np.mod(cols, w) >> shift)
            out[i, j] = max(np.float32(0.0), M[np.ix_(fi, fj)].max())
    return out


def build_all(D, T, shift, m2_shift):
    """The five structures as read_structure returns them."""
    return {"dem": padded_dem(D), "color": colour_pairs(T), "mip": max_mip(D, shift), "mip2": medium_mip(D, m2_shift),
            "hmip": horizon_mip(D, shift)}


# ---- the consumers' invariants -----------------------------------------------------------------------------------------
def check_A(pairs, D, shift):
    """seg_anchors reads cell (i, j), i in [-1, mip_h], j in [-1, mip_w], for every padded texel (r, c), r in [-2, h+1],
    c in [-2, w+1], with r >> shift == i and c >> shift == j (the anchors' floors -1 / +2), through the row-pair element
    (i+1, j+1) or as the second component of (i, j+1): the cell must be >= Dp(r, c), the second component must be the cell one
    row below, the last row its own pair.  Returns the violations as (kind, i, j)."""
    h, w = D.shape
    bad = []
    r = np.arange(-2, h + 2)
    c = np.arange(-2, w + 2)
    need = np.full(pairs.shape[:2], -np.inf, np.float32)                # max of the texels that index each stored cell
    P = window(D, -2, h + 1, -2, w + 1)
    ii, jj = (r >> shift) + 1, (c >> shift) + 1
    if ii.min() < 0 or jj.min() < 0 or ii.max() >= pairs.shape[0] or jj.max() >= pairs.shape[1]:
        return [("shape", int(ii.max()), int(jj.max()))]
    np.maximum.at(need, (ii[:, None], jj[None, :]), P)
    for i, j in zip(*np.nonzero(pairs[..., 0] < need)):
        bad.append(("small", int(i) - 1, int(j) - 1))
    below = window(pairs[..., 0], 1, pairs.shape[0], 0, pairs.shape[1] - 1)
    for i, j in zip(*np.nonzero(pairs[..., 1].view(np.uint32) != below.view(np.uint32))):
        bad.append(("pair", int(i) - 1, int(j) - 1))
    return bad


def check_B(S2, D, m2_shift):
    """first_kept_step / last_kept_step read element (i+1, j+1), i = r >> m2_shift, j = c >> m2_shift, for a step whose position
    floors to texel (r, c), r in [-1, h), c in [-1, w): it must be >= the four bilinear taps Dp over (r, r+1) x (c, c+1)."""
    h, w = D.shape
    r = np.arange(-1, h)
    c = np.arange(-1, w)
    taps = np.maximum(np.maximum(window(D, -1, h - 1, -1, w - 1), window(D, 0, h, -1, w - 1)),
                      np.maximum(window(D, -1, h - 1, 0, w), window(D, 0, h, 0, w)))
    ii, jj = (r >> m2_shift) + 1, (c >> m2_shift) + 1
    if ii.max() >= S2.shape[0] or jj.max() >= S2.shape[1]:
        return [("shape", int(ii.max()), int(jj.max()))]
    need = np.full(S2.shape, -np.inf, np.float32)
    np.maximum.at(need, (ii[:, None], jj[None, :]), taps)
    return [("small", int(i) - 1, int(j) - 1) for i, j in zip(*np.nonzero(S2 < need))]


def check_H(Hm, D, hm_shift):
    """horizon_cell picks, for a march origin that floors to texel (r, c), r in [-1, h), c in [-1, w), the cell
    (clip(r >> hm_shift), clip(c >> hm_shift)); horizon_kend cuts the march with it whenever the ground track AND its taps
    (the +4 it budgets) stay within Cc = 2^hm_shift texels of the origin in both directions: the cell must be >= Dp over rows
    [r - Cc, r + Cc] x columns [c - Cc, c + Cc].  Returns the violations as ("small", i, j, r, c) with one origin each."""
    h, w = D.shape
    Cc = 1 << hm_shift
    hh, hw = Hm.shape
    # need[r + 1, c + 1] for the origin (r, c): the clamped rows [r - Cc, r + Cc] are the rows max(r - Cc, 0) .. min(r + Cc, h - 1);
    # 2 Cc + 1 wrapped columns are every column once they number w or more
    rows = np.stack([D[max(r - Cc, 0):min(r + Cc, h - 1) + 1].max(0) for r in range(-1, h)])
    if 2 * Cc + 1 >= w:
        need = np.repeat(rows.max(1)[:, None], w + 1, 1)
    else:
        extc = np.take(rows, np.arange(-1 - Cc, w + Cc), axis=1, mode="wrap")
        need = np.stack([extc[:, b:b + 2 * Cc + 1].max(1) for b in range(w + 1)], 1)
    i = np.clip(np.arange(-1, h) >> hm_shift, 0, hh - 1)
    j = np.clip(np.arange(-1, w) >> hm_shift, 0, hw - 1)
    have = Hm[i[:, None], j[None, :]]
    bad, seen = [], set()
    for a, b in zip(*np.nonzero(have < need)):
        key = (int(i[a]), int(j[b]))
        if key not in seen:
            seen.add(key)
            bad.append(("small",) + key + (int(a) - 1, int(b) - 1))
    return bad


# ---- test terrain ------------------------------------------------------------------------------------------------------
def spiked_dem(h, w, shift=4, seed=0, interior=False):
    """Seeded noise in [0.90, 0.95) plus single-texel spikes of distinct heights on row 0 and row h-1, column 0 and column w-1,
    and on the first and the last texel of the last (partial) cell of 2^shift texels in each direction.

    Those texels all lie within two texels of a neighbouring cell, whose dilated maximum therefore holds them as well: a
    structure built from the max-mip's cells (the horizon mip) can lose the last cell altogether without losing any of them.
    interior = True adds the map's two highest spikes in the MIDDLE of the last cell, one per direction, which only that
    cell holds when it is five texels wide or more."""
    rng = np.random.default_rng(1000 * h + w + seed)
    D = (np.float32(0.90) + rng.random((h, w), np.float32) * np.float32(0.05)).astype(np.float32)
    C = 1 << shift
    lr, lc = ((h - 1) // C) * C, ((w - 1) // C) * C           # the first texel of the last cell
    spots = [(0, w // 3), (h - 1, (2 * w) // 3), (h // 3, 0), ((2 * h) // 3, w - 1), (0, 0), (h - 1, w - 1),
             (lr, w // 2), (h - 1, w // 2 + 1), (h // 2, lc), (h // 2 + 1, w - 1), (lr, lc), (0, lc), (lr, 0)]
    for n, (r, c) in enumerate(spots):
        D[r % h, c % w] = np.float32(0.96 + 0.003 * n)
    if interior:
        D[lr + (h - lr) // 2, w // 4] = np.float32(0.9985)
        D[h // 2, lc + (w - lc) // 2] = np.float32(0.999)
    return D


def noise_colour(h, w, seed=0):
    return np.random.default_rng(77 * h + w + seed).integers(0, 256, (h, w, 4), dtype=np.uint8)
