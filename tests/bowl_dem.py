"""A spherical-bowl crater on the smooth sphere, TEST INFRASTRUCTURE (the analytic bowl check).

The rim is the circle at angular radius theta_c about the crater's centre on the unit sphere (the DEM's D is the radius in
units of R).  Inside it the surface is the lower cap of the sphere through the rim whose lowest point lies `depth` below the
rim's plane, so the crater is an exact spherical bowl in 3D and its interior sees itself with the view factor
f = 4 (d/D)^2 / (1 + 4 (d/D)^2) (Buhl et al. 1968; Ingersoll et al. 1992), D the rim's diameter.  Outside the rim the
sphere curves away below the rim's plane, so nothing else is in view from inside."""
import math

import numpy as np


def bowl_view_factor(d_over_D):
    x = 4.0 * d_over_D * d_over_D
    return x / (1.0 + x)


def bowl_geometry(theta_c_deg, d_over_D):
    """(a, d, Rs, c0): rim radius, depth, bowl-sphere radius and the distance of its centre from the Moon's centre along the
    crater axis, all in units of R."""
    th = math.radians(theta_c_deg)
    a = math.sin(th)
    d = d_over_D * 2.0 * a
    Rs = (a * a + d * d) / (2.0 * d)
    c0 = math.cos(th) - d + Rs
    return a, d, Rs, c0


def bowl_dem(h, w, lat0_deg=0.0, lon0_deg=0.0, theta_c_deg=6.0, d_over_D=0.2):
    """(h, w) float32 D on the DEM's lat/lon grid (texel centres, north row first, longitudes from -180): 1 outside the rim,
    the bowl's radial distance inside."""
    lat = math.pi / 2 - (np.arange(h) + 0.5) * (math.pi / h)
    lon = -math.pi + (np.arange(w) + 0.5) * (2 * math.pi / w)
    la, lo = np.meshgrid(lat, lon, indexing="ij")
    u = np.stack([np.cos(la) * np.sin(lo), np.cos(la) * np.cos(lo), np.sin(la)], -1)
    l0, m0 = math.radians(lat0_deg), math.radians(lon0_deg)
    e = np.array([math.cos(l0) * math.sin(m0), math.cos(l0) * math.cos(m0), math.sin(l0)])
    cos_t = np.clip(u @ e, -1.0, 1.0)
    sin2 = 1.0 - cos_t * cos_t
    _, _, Rs, c0 = bowl_geometry(theta_c_deg, d_over_D)
    t = c0 * cos_t - np.sqrt(np.maximum(Rs * Rs - c0 * c0 * sin2, 0.0))     # the nearer root along the radial ray
    inside = cos_t > math.cos(math.radians(theta_c_deg))
    return np.where(inside, t, 1.0).astype(np.float32)


def bowl_points(lat0_deg, lon0_deg, theta_c_deg, fractions, n_az=4):
    """Points at angular distance fraction x theta_c from the centre along n_az azimuths (the centre once): (lat, lon)."""
    lat, lon = [lat0_deg], [lon0_deg]
    for fr in fractions:
        for k in range(n_az):
            az = 2 * math.pi * (k + 0.5) / n_az
            r = fr * theta_c_deg
            lat.append(lat0_deg + r * math.cos(az))
            lon.append(lon0_deg + r * math.sin(az) / math.cos(math.radians(lat0_deg)))
    return np.array(lat), np.array(lon)
