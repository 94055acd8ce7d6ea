"""The float64 model of the regolith column, written from the spec alone: the grid, the absorbed
flux from (f, mu, S) and the explicit steps, vectorised over points.  It returns FULL, SUMMARY and the diagnostics the spec
names: Newton solves that reached the cap and the largest coefficient sum of an interior update (stable while <= 1), and
the range the column's temperatures took.  The grid and constants are the spec's, or those of any MrtxThermalModel, read
from the ctypes struct the kernel receives."""
import math
from typing import NamedTuple

import numpy as np

RHO_S, RHO_D, H_RHO = 1100.0, 1800.0, 0.06
K_S, K_D, CHI = 7.4e-4, 3.4e-3, 2.7
C_POLY = (-3.6125, 2.7431, 2.3616e-3, -1.2340e-5, 8.9093e-9)
EPS, SIGMA, Q_GEO = 0.95, 5.670374419e-8, 0.018
A0, A_A, A_B = 0.12, 0.06, 0.25
P_SYN = 29.530589 * 86400.0


def spec_grid():
    """(z, dz, rho, kc, zs, ref): the grid of the spec."""
    zs = math.sqrt(K_S / (RHO_S * 600.0) * P_SYN / math.pi)
    z, d = [0.0], zs / 10.0
    while z[-1] < 20.0 * zs:
        z.append(z[-1] + d)
        d *= 1.2
    z = np.array(z)
    rho = RHO_D - (RHO_D - RHO_S) * np.exp(-z / H_RHO)
    kc = K_D - (K_D - K_S) * (RHO_D - rho) / (RHO_D - RHO_S)
    return z, np.diff(z), rho, kc, zs, int(np.argmax(z >= 3.0 * zs))


class Consts(NamedTuple):
    """What the column needs besides the schedule: the grid and the constants of one MrtxThermalModel (or of the spec)."""
    dz: np.ndarray
    rho: np.ndarray
    kc: np.ndarray
    ref: int
    chi: float
    c: tuple
    eps: float
    sigma: float
    q_geo: float
    albedo: tuple


def spec_consts(grid=None):
    z, dz, rho, kc, zs, ref = spec_grid() if grid is None else grid
    return Consts(dz, rho, kc, ref, CHI, C_POLY, EPS, SIGMA, Q_GEO, (A0, A_A, A_B))


def model_consts(md):
    """The grid and constants straight from the ctypes MrtxThermalModel `md` the kernel receives."""
    n = int(md.n_nodes)
    return Consts(np.array(md.dz[:n - 1], np.float64), np.array(md.rho[:n], np.float64), np.array(md.kc[:n], np.float64),
                  int(md.ref_node), float(md.chi), tuple(md.c), float(md.emissivity), float(md.sigma), float(md.q_geo),
                  tuple(md.albedo))


def heat_capacity(T, c=C_POLY):
    c0, c1, c2, c3, c4 = c
    return c0 + T * (c1 + T * (c2 + T * (c3 + T * c4)))


def conductivity(kc, T, chi=CHI):
    return kc * (1.0 + chi * (T / 350.0) ** 3)


def absorbed(f, mu, S, model=None):
    """Q_abs = (1 - A(theta)) S f max(mu, 0), exactly 0 where f == 0 or mu <= 0; broadcasting float64.  The albedo law is
    the spec's, or that of the MrtxThermalModel `model`."""
    a0, a_a, a_b = (A0, A_A, A_B) if model is None else tuple(model.albedo)
    f, mu, S = np.broadcast_arrays(np.asarray(f, np.float64), np.asarray(mu, np.float64), np.asarray(S, np.float64))
    th = np.degrees(np.arccos(np.clip(mu, -1.0, 1.0)))
    A = a0 + a_a * (th / 45.0) ** 3 + a_b * (th / 90.0) ** 8
    q = (1.0 - A) * S * f * mu
    return np.where((f > 0.0) & (mu > 0.0), q, 0.0)


def max_step(model=None):
    """Delta_max, s.  Of the spec's grid (F = 0.5, the 1 K grid of [20, 450] K), or exactly as mrtx_thermal's checks form it
    for the MrtxThermalModel `model`: 1/2 min over T and the interior nodes of rho_i min(dz_{i-1}, dz_i)^2 c(T) / k_i(T)."""
    if model is None:
        _, dz, rho, kc, _, _ = spec_grid()
        T = np.arange(20.0, 451.0)
        d = np.minimum(dz[:-1], dz[1:])
        return 0.5 * float(np.min(rho[1:-1, None] * d[:, None] ** 2 * heat_capacity(T)[None, :] /
                                  conductivity(kc[1:-1, None], T[None, :])))
    n, (c0, c1, c2, c3, c4), chi = int(model.n_nodes), tuple(model.c), float(model.chi)
    best = math.inf
    for T in range(20, 451):
        t = float(T)
        cT, r = c0 + t * (c1 + t * (c2 + t * (c3 + t * c4))), t / 350.0
        for i in range(1, n - 1):
            d = min(model.dz[i - 1], model.dz[i])
            best = min(best, model.rho[i] * d * d * cT / (model.kc[i] * (1.0 + chi * r * r * r)))
    return 0.5 * best


def geotherm(T, i0, top, kc, dz, p=None):
    """Below node i0 (in place, every point): the steady profile carrying Q upward from temperature `top` at node i0 -- link
    by link k_{i+1/2} (T_{i+1} - T_i) / dz_i = Q (six fixed-point passes from T_{i+1} = T_i), the last link by the bottom
    rule from the new value above it (from `top` itself when i0 = N - 2).  Node i0 itself is left as it is."""
    chi, q = (CHI, Q_GEO) if p is None else (p.chi, p.q_geo)
    N = T.shape[1]
    prev = np.asarray(top, np.float64)
    for i in range(i0, N - 2):
        t = prev.copy()
        for _ in range(6):
            t = prev + q * dz[i] / (0.5 * (conductivity(kc[i], prev, chi) + conductivity(kc[i + 1], t, chi)))
        T[:, i + 1] = prev = t
    T[:, N - 1] = prev + q * dz[N - 2] / conductivity(kc[N - 2], prev, chi)


def surface_newton(T0, T1, k1, kc0, dz0, qa, p=None):
    """eps sigma T0^4 = qa + k_1/2(T0) (T1 - T0) / dz0 by Newton from T0 (|dT| < 1e-3 K, at most 30 iterations); returns
    (T0, cap hits)."""
    p = spec_consts() if p is None else p
    t = T0.copy()
    active = np.ones(t.shape, bool)
    for _ in range(30):
        kh = 0.5 * (conductivity(kc0, t, p.chi) + k1)
        d = T1 - t
        g = p.eps * p.sigma * t ** 4 - qa - kh * d / dz0
        gd = 4.0 * p.eps * p.sigma * t ** 3 + (kh - 0.5 * kc0 * 3.0 * p.chi * t ** 2 / 350.0 ** 3 * d) / dz0
        dt = np.where(active, g / gd, 0.0)
        t = t - dt
        active &= ~(np.abs(dt) < 1e-3)
        if not active.any():
            break
    return t, int(active.sum())


def run(qabs, spacing_s=None, n_sub=None, n_spin=None, block=None, n_reset=None, record_all=True, grid=None, probe=None,
        model=None):
    """Step the columns of P points through qabs (P, m) (section 3.10).  The schedule is (spacing_s, n_sub, n_spin, block,
    n_reset) on the spec's constants and grid (or `grid`), or, with `model`, everything -- schedule, grid and constants --
    read from that MrtxThermalModel.  Returns a dict: full (P, m - n_spin) surface temperatures after each recorded epoch,
    summary (P, 4) (max, min, mean, mean bottom), caps, coef_max (the largest coefficient sum of an interior update), t_lo
    and t_hi (the lowest and highest temperature of any node after any step; NaN if one was NaN), out_of_range (the
    (point, epoch)s after whose steps a node is non-finite or outside [20, 450] K), and with record_all the spin-up's surface
    series too (spin_surface (P, n_spin)) and the bottom node after each epoch (bottom (P, m)).  `probe`, if a callable, is
    called as probe(k, T) after every epoch's steps."""
    if model is None:
        p = spec_consts(grid)
    else:
        if grid is not None or any(a is not None for a in (spacing_s, n_sub, n_spin, block, n_reset)):
            raise ValueError("with a model the schedule and grid come from it")
        p = model_consts(model)
        spacing_s, n_sub, n_spin = float(model.spacing_s), int(model.n_sub), int(model.n_spin)
        block, n_reset = int(model.block), int(model.n_reset)
    dz, rho, kc, ref = p.dz, p.rho, p.kc, p.ref
    es = p.eps * p.sigma
    qabs = np.atleast_2d(np.asarray(qabs, np.float64))
    P, m = qabs.shape
    N = rho.size
    delta = spacing_s / n_sub
    qs = qabs[:, :n_spin].mean(1) if n_spin > 0 else np.zeros(P)
    T = np.repeat((((qs + p.q_geo) / es) ** 0.25)[:, None], N, 1)
    geotherm(T, 0, T[:, 0], kc, dz, p)
    surf = np.empty((P, m))
    bottom = np.empty((P, m))
    caps, coef_max, t_lo, t_hi, n_out = 0, 0.0, math.inf, -math.inf, 0
    ref_sum, in_block, blocks = np.zeros(P), 0, 0
    denom = rho[1:-1] * (dz[:-1] + dz[1:])
    with np.errstate(all="ignore"):       # a diverging column is a result here, reported through the diagnostics
        for k in range(m):
            qa = qabs[:, k]
            for _ in range(n_sub):
                kn = conductivity(kc, T, p.chi)
                kh = 0.5 * (kn[:, :-1] + kn[:, 1:])
                G = kh * (T[:, 1:] - T[:, :-1]) / dz
                cT = heat_capacity(T[:, 1:-1], p.c)
                coef = delta * 2.0 * (kh[:, 1:] / dz[1:] + kh[:, :-1] / dz[:-1]) / (cT * denom)
                coef_max = max(coef_max, float(coef.max()))
                T[:, 1:-1] = T[:, 1:-1] + delta * 2.0 * (G[:, 1:] - G[:, :-1]) / (cT * denom)
                k1 = conductivity(kc[1], T[:, 1], p.chi)
                T[:, 0], c = surface_newton(T[:, 0], T[:, 1], k1, kc[0], dz[0], qa, p)
                caps += c
                T[:, -1] = T[:, -2] + p.q_geo * dz[-1] / conductivity(kc[-2], T[:, -2], p.chi)
                t_lo, t_hi = min(t_lo, float(T.min())), max(t_hi, float(T.max()))
            n_out += int((~((T >= 20.0) & (T <= 450.0))).any(1).sum())
            surf[:, k] = T[:, 0]
            bottom[:, k] = T[:, -1]
            if probe is not None:
                probe(k, T)
            if k < n_spin and blocks < n_reset:
                ref_sum += T[:, ref]
                in_block += 1
                if in_block == block:
                    geotherm(T, ref, ref_sum / block, kc, dz, p)
                    ref_sum[:], in_block, blocks = 0.0, 0, blocks + 1
    full = surf[:, n_spin:]
    out = dict(full=full, caps=caps, coef_max=coef_max, t_lo=t_lo, t_hi=t_hi, out_of_range=n_out,
               summary=np.stack([full.max(1), full.min(1), full.mean(1), bottom[:, n_spin:].mean(1)], 1))
    if record_all:
        out["spin_surface"] = surf[:, :n_spin]
        out["bottom"] = bottom
    return out
