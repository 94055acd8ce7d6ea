"""Volatiles in the regolith column: the vapour-pressure law of a species, its free sublimation rate
and the depth at which buried ice survives, in float64 on the host.  The kernel receives the law folded into four
coefficients (MrtxVolatile); nothing here needs a GPU.

Water ice: Murphy & Koop 2005, "Review of the vapour pressures of ice and supercooled water for atmospheric applications",
Q. J. R. Meteorol. Soc. 131, eq. 7.  Other species are the caller's coefficients."""
import math
from typing import NamedTuple

import numpy as np

R_GAS = 8.314462618                    # J mol^-1 K^-1
RATE_MAX = 1e-3 / (1e9 * 365.25 * 86400.0)     # 1 mm per 10^9 years, m s^-1: the usual bar for "stable"
MM_PER_GYR = 1e3 * 1e9 * 365.25 * 86400.0      # m s^-1 -> mm per 10^9 years


class Species(NamedTuple):
    name: str
    a: tuple                # ln p[Pa] = a0 - a1 / T + a2 ln T + a3 T over the solid
    molar_mass: float       # kg mol^-1
    rho_solid: float        # kg m^-3


H2O = Species("H2O", (9.550426, 5723.265, 3.53068, -0.00728332), 0.01801528, 917.0)


def vapour_pressure(T, species=H2O):
    """p(T) over the solid, Pa (T in K).  The exponent is formed in numpy's long double (80-bit where the platform has it),
    so that the float64 result is a reference for the folded law of `law`, whose exponent is rounded in float64."""
    T = np.asarray(T, np.float64).astype(np.longdouble)
    a0, a1, a2, a3 = (np.longdouble(x) for x in species.a)
    return np.exp(a0 - a1 / T + a2 * np.log(T) + a3 * T)


def sublimation_rate(T, species=H2O):
    """E(T) = p(T) sqrt(M / (2 pi R T)), the free (Hertz-Knudsen) sublimation rate into vacuum, kg m^-2 s^-1."""
    T = np.asarray(T, np.float64)
    k = np.longdouble(species.molar_mass) / (2.0 * np.longdouble(math.pi) * np.longdouble(R_GAS) * T.astype(np.longdouble))
    return np.asarray(vapour_pressure(T, species) * np.sqrt(k), np.float64)


def law(species=H2O):
    """The MrtxVolatile of a species: ln E(T) = b0 - b1 / T + b2 ln T + b3 T with the Hertz-Knudsen factor folded in,
    b = (a0 + ln(M / (2 pi R)) / 2, a1, a2 - 1/2, a3).  A sequence of four numbers is taken as b itself."""
    from ._lib import MrtxVolatile
    if isinstance(species, Species):
        a0, a1, a2, a3 = species.a
        b = (a0 + 0.5 * math.log(species.molar_mass / (2.0 * math.pi * R_GAS)), a1, a2 - 0.5, a3)
    else:
        b = tuple(float(x) for x in species)
        if len(b) != 4:
            raise ValueError("a law has four coefficients")
    out = MrtxVolatile()
    out.b[:] = list(b)
    return out


def stability_depth(e_mean, z, species=H2O, rate_max=RATE_MAX, barrier_m=None):
    """The shallowest depth, m, at which ice of `species` retreats by at most rate_max (m s^-1).  e_mean: (..., n_nodes)
    time-mean free sublimation rates at the node depths z (n_nodes,), kg m^-2 s^-1.  The retreat rate of node i is
    r_i = e_mean_i / rho_solid; with barrier_m = l it is multiplied by l / (l + z_i), the attenuation of the vapour flux by
    Knudsen diffusion through a dry lag of thickness z_i with diffusion length l (after Schorghofer & Taylor 2007).  None:
    the exposed-ice criterion, the conservative one.  0 where r_0 <= rate_max; otherwise at the first node with
    r_i <= rate_max, ln r taken as linear in z between nodes i - 1 and i (z_i itself when r_i = 0); +inf where no node
    qualifies."""
    e = np.asarray(e_mean, np.float64)
    z = np.asarray(z, np.float64).ravel()
    if e.shape[-1] != z.size:
        raise ValueError("e_mean must hold one rate per node depth")
    r = e / float(species.rho_solid)
    if barrier_m is not None:
        l = float(barrier_m)
        if not l > 0.0:
            raise ValueError("barrier_m must be positive")
        r = r * (l / (l + z))
    ok = r <= rate_max
    i = np.argmax(ok, axis=-1)                        # the first qualifying node (0 where none does)
    j = np.maximum(i - 1, 0)
    r1 = np.take_along_axis(r, i[..., None], -1)[..., 0]
    r0 = np.take_along_axis(r, j[..., None], -1)[..., 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (math.log(rate_max) - np.log(r0)) / (np.log(r1) - np.log(r0))
        depth = np.where(r1 > 0.0, z[j] + t * (z[i] - z[j]), z[i])
    depth = np.where(i == 0, 0.0, depth)
    return np.where(ok.any(axis=-1), depth, np.inf)
