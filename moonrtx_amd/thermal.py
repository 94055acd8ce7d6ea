"""The regolith column of the surface-temperature stage: the constants, the layer grid and the
stable step, in float64 on the host.  The kernel receives the tables (MrtxThermalModel); nothing here needs a GPU.

Regolith properties: Hayne et al. 2017, "Global regolith thermophysical properties of the Moon from the Diviner Lunar
Radiometer Experiment", JGR Planets 122."""
import math
from typing import NamedTuple

import numpy as np

RHO_S, RHO_D = 1100.0, 1800.0          # surface / deep density, kg m^-3
H_RHO = 0.06                           # density e-folding depth, m
K_S, K_D = 7.4e-4, 3.4e-3              # contact conductivity, surface / deep, W m^-1 K^-1
CHI = 2.7                              # radiative conductivity: k(T) = kc (1 + CHI (T / 350)^3)
C_POLY = (-3.6125, 2.7431, 2.3616e-3, -1.2340e-5, 8.9093e-9)     # c(T) = c0 + c1 T + ... + c4 T^4, J kg^-1 K^-1
EMISSIVITY = 0.95
SIGMA = 5.670374419e-8
Q_GEO = 0.018                          # geothermal flux, W m^-2
ALBEDO = (0.12, 0.06, 0.25)            # A(theta) = A0 + a (theta / 45 deg)^3 + b (theta / 90 deg)^8
S0 = 1361.0                            # solar constant at 1 AU, W m^-2
LUNATION_S = 29.530589 * 86400.0       # synodic period, s
MAX_NODES = 32                         # MRTX_THERMAL_MAX_NODES

# defaults chosen with the float64 model
F_STEP = 0.5                           # Delta_max = F_STEP x the explicit bound
SPINUP_LUNATIONS = 10                  # spin-up epochs = this many lunations
RESETS = 8                             # deep-column resets: after each of the first RESETS spin-up lunations


class ThermalGrid(NamedTuple):
    z: np.ndarray           # node depths, m (z[0] = 0)
    dz: np.ndarray          # z[i+1] - z[i]
    rho: np.ndarray         # density per node
    kc: np.ndarray          # contact conductivity per node
    skin: float             # diurnal skin depth zs, m
    ref_node: int           # the first node with z >= 3 zs


def heat_capacity(T):
    c0, c1, c2, c3, c4 = C_POLY
    return c0 + T * (c1 + T * (c2 + T * (c3 + T * c4)))


def grid():
    """The layer grid: spacings zs/10 growing by 1.2 from the surface to the first node at >= 20 zs."""
    kappa = K_S / (RHO_S * 600.0)
    zs = math.sqrt(kappa * LUNATION_S / math.pi)
    z = [0.0]
    dz = zs / 10.0
    while z[-1] < 20.0 * zs:
        z.append(z[-1] + dz)
        dz *= 1.2
    z = np.array(z)
    rho = RHO_D - (RHO_D - RHO_S) * np.exp(-z / H_RHO)
    kc = K_D - (K_D - K_S) * (RHO_D - rho) / (RHO_D - RHO_S)
    ref = int(np.argmax(z >= 3.0 * zs))
    return ThermalGrid(z, np.diff(z), rho, kc, zs, ref)


def max_step(g=None, F=F_STEP):
    """Delta_max = F min_i rho_i min(dz_{i-1}, dz_i)^2 min_{T in [20, 450] K} c(T) / k_i(T) over the interior nodes, seconds."""
    g = grid() if g is None else g
    T = np.arange(20.0, 451.0)
    c = heat_capacity(T)
    k = g.kc[1:-1, None] * (1.0 + CHI * (T[None, :] / 350.0) ** 3)
    dz = np.minimum(g.dz[:-1], g.dz[1:])
    return F * float(np.min(g.rho[1:-1, None] * dz[:, None] ** 2 * c[None, :] / k))


def steps_per_epoch(spacing_s, g=None, F=F_STEP):
    return max(1, int(math.ceil(spacing_s / max_step(g, F))))


def block_epochs(spacing_s):
    """Epochs of one spin-up block: one lunation."""
    return max(1, int(round(LUNATION_S / spacing_s)))


def model(spacing_s=3600.0, spinup_lunations=SPINUP_LUNATIONS, resets=RESETS, F=F_STEP):
    """The MrtxThermalModel of the default regolith for evenly spaced epochs `spacing_s` apart, with `spinup_lunations`
    lunations of spin-up epochs and the deep column reset after each of the first `resets` of them."""
    from ._lib import MrtxThermalModel
    g = grid()
    n = g.z.size
    if n > MAX_NODES:
        raise ValueError(f"the grid has {n} nodes, more than {MAX_NODES}")
    md = MrtxThermalModel()
    md.n_nodes = n
    md.spacing_s = float(spacing_s)
    md.n_sub = steps_per_epoch(spacing_s, g, F)
    md.block = block_epochs(spacing_s)
    md.n_spin = int(spinup_lunations) * md.block
    md.n_reset = min(int(resets), int(spinup_lunations))
    md.ref_node = g.ref_node
    md.dz[:n - 1] = list(g.dz)
    md.rho[:n] = list(g.rho)
    md.kc[:n] = list(g.kc)
    md.chi = CHI
    md.c[:] = list(C_POLY)
    md.emissivity, md.sigma, md.q_geo = EMISSIVITY, SIGMA, Q_GEO
    md.albedo[:] = list(ALBEDO)
    return md


def albedo(theta_deg):
    """A(theta) of the default regolith, theta in degrees (float64)."""
    a0, a, b = ALBEDO
    t = np.asarray(theta_deg, np.float64)
    return a0 + a * (t / 45.0) ** 3 + b * (t / 90.0) ** 8


def albedo_hemispherical(n=64):
    """A_h, the albedo under diffuse incidence: the cosine-weighted hemispherical mean of A(theta),
    int_0^{pi/2} A(theta) 2 sin(theta) cos(theta) dtheta, by n-point Gauss-Legendre quadrature in float64."""
    x, w = np.polynomial.legendre.leggauss(int(n))
    th = (x + 1.0) * (math.pi / 4.0)
    return float(np.sum(w * albedo(np.degrees(th)) * 2.0 * np.sin(th) * np.cos(th)) * (math.pi / 4.0))
