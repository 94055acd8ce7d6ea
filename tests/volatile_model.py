"""The float64 model of the subsurface modes, written from the spec alone on top of
thermal_model.run's per-epoch probe: every node's temperature after each recorded epoch (COLUMN), and per node the mean free
sublimation rate and the highest temperature (VOLATILE).  The law is ln E(T) = b0 - b1 / T + b2 ln T + b3 T."""
import numpy as np

import thermal_model as tm


def ln_rate(T, b):
    """x(T) = b0 - b1 / T + b2 ln T + b3 T, float64, broadcasting."""
    T = np.asarray(T, np.float64)
    return b[0] - b[1] / T + b[2] * np.log(T) + b[3] * T


def rate(T, b):
    return np.exp(ln_rate(T, b))


def columns(qabs, model):
    """(P, m - n_spin, n_nodes) float64: the column of every point after each recorded epoch's steps, and run()'s dict."""
    qabs = np.atleast_2d(np.asarray(qabs, np.float64))
    n_spin, n = int(model.n_spin), int(model.n_nodes)
    col = np.empty((qabs.shape[0], qabs.shape[1] - n_spin, n))

    def probe(k, T):
        if k >= n_spin:
            col[:, k - n_spin, :] = T
    r = tm.run(qabs, model=model, probe=probe, record_all=False)
    return col, r


def fold(col, b):
    """The spec's reduction over a (P, m_rec, N) COLUMN: E at the float32-rounded temperature, a float64 left fold from 0 in
    epoch order divided by m_rec, and the float32 maximum.  Returns (e_mean (P, N) float64, t_max (P, N) float64)."""
    tf = np.asarray(col).astype(np.float32)
    td = tf.astype(np.float64)
    s = np.zeros((td.shape[0], td.shape[2]))
    for k in range(td.shape[1]):
        s = s + rate(td[:, k, :], b)
    return s / float(td.shape[1]), tf.max(axis=1).astype(np.float64)


def steady_geotherm(model):
    """The column a never-lit point settles on: the surface at (q_geo / (eps sigma))^(1/4) and below it the steady profile
    carrying q_geo upward (thermal_model.geotherm), (n_nodes,) float64."""
    p = tm.model_consts(model)
    T = np.full((1, p.rho.size), (p.q_geo / (p.eps * p.sigma)) ** 0.25)
    tm.geotherm(T, 0, T[:, 0].copy(), p.kc, p.dz, p)
    return T[0]
