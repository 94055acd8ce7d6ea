"""Built cases for the wave layouts of the illumination stage (DESIGN.md sections 4.8 and 4.9), TEST INFRASTRUCTURE, numpy only.

illum_kernel packs 64 / n_sun nodes, a PW x PH block in raster order, into one wave with the n_sun samples of a node in
adjacent lanes; illum_series_kernel does the same with points as rows and a window's epochs as columns, PW narrowed to the
window.  The layout is chosen at run time, so every n_sun, a one-row band and every window length is a layout of its own, and
a mistake in one of them shows only where the outputs of neighbouring nodes differ and where a grid is ragged against the
block.  This module holds

  the scene       S1 with the Sun's radius x 16 over the egg-crate relief, a window on the evening terminator: neighbouring
                  nodes differ in lit and a fifth of them see part of the disc (with the stock Sun, under 5 %);
  the cases       grid shapes ragged against every block, and series of every window length at which the narrowing rule takes
                  another branch, with point counts that are no multiple of any PH and per-point window starts;
  the models      the float64 model (tests/illum_model.py) of every case, run once over the seven sample tables side by side;
  the lane map    launch() / lanes() / report(): the mapping of sections 4.8 and 4.9 restated -- which (node, sample) each
                  lane of each wave holds, which lanes are past the edge, and the lit and shadow_rays a kernel with that
                  mapping reports from a per-sample visibility table -- with named deliberate defects (MUTANTS), so that the
                  CPU suite can show that the cases tell each of them from the true mapping
                  (tests/test_illum_layouts_host.py)."""
import functools
from datetime import datetime, timedelta, timezone

import numpy as np

import illum_model as im
import model_cases as mc
from moonrtx_amd.scene import named_scene

N_SUN = (1, 2, 4, 8, 16, 32, 64)
SUN_FACTOR = 16.0                                   # the light's radius: 0.27 deg x 16 = 4.3 deg
LAT, LON_OFF = (20.0, -20.0), (79.0, 93.0)          # the window: latitudes, and longitudes east of the subsolar point
SHAPES = ((9, 21), (13, 7), (5, 1), (1, 13), (3, 19))
THIN = ((5, 1), (1, 13), (3, 19))                   # under 90 nodes: held to "a dark, a lit and a partial node" only
COUNTS = (1, 2, 3, 5, 8, 9, 17, 33, 64, 65)         # the series' window lengths
POINTS = (1, 3, 7)                                  # ... and point counts
N_EPOCHS = 80
# the node block of section 4.8 per n_sun, PW x PH; a one-row band or a point list takes PW = 64 / n_sun, PH = 1
GRID_BLOCK = {1: (8, 8), 2: (8, 4), 4: (4, 4), 8: (4, 2), 16: (2, 2), 32: (2, 1), 64: (1, 1)}
MUTANTS = ("pw_too_wide", "pw_ph_swapped", "one_row_ignored", "group_sum_2n", "edge_lanes_not_zeroed", "sample_shifted",
           "series_pw_not_narrowed")


def scene():
    s = named_scene("S1", 16, 16)
    s.light_radius = s.light_radius * SUN_FACTOR
    return s


def dem():
    return mc.corrugated_dem()


def window():
    """(lat, lon) of the grid cases: the evening terminator of scene()."""
    _, lo0 = im.subsolar_latlon(scene())
    return LAT, (lo0 + LON_OFF[0], lo0 + LON_OFF[1])


def grid_nodes(lat, lon, shape):
    """DESIGN.md section 3.6's node centres (MoonRT.grid_nodes states the same expressions), as two (h w,) arrays."""
    h, w = shape
    la = lat[0] - (np.arange(h) + 0.5) * ((lat[0] - lat[1]) / h)
    lo = lon[0] + (np.arange(w) + 0.5) * ((lon[1] - lon[0]) / w)
    LA, LO = np.meshgrid(la, lo, indexing="ij")
    return LA.ravel(), LO.ravel()


def sun_table(n):
    """Section 3.6's (u2, u3) table of n samples, (n, 2) float32 (pinned against the library's by test_illumination_host)."""
    if n == 1:
        return np.zeros((1, 2), np.float32)
    i = np.arange(n)
    t = i * 0.6180339887498949
    return np.stack([(i + 0.5) / n, t - np.floor(t)], -1).astype(np.float32)


def _all_tables():
    return np.concatenate([sun_table(n) for n in N_SUN]).astype(np.float64), np.cumsum((0,) + N_SUN)


def _split(m):
    """One illuminate() over the seven tables side by side -> per n_sun what illuminate() over that table alone returns (a
    sample's march does not depend on the other samples)."""
    _, edge = _all_tables()
    out = {}
    for i, n in enumerate(N_SUN):
        c = slice(edge[i], edge[i + 1])
        V, cp = m["V"][:, c], m["cos_pos"][:, c]
        out[n] = dict(V=V, flagged=m["flagged"][:, c], cos_pos=cp, lit=V.mean(1),
                      irr=np.where(V, m["carried"][:, c], 0.0).mean(1), mu=m["mu"], D=m["D"], shadow_rays=int(cp.sum()))
    return out


@functools.lru_cache(maxsize=None)
def grid_model(shape):
    """{n_sun: illuminate()'s dict} at the nodes of a grid case."""
    lat, lon = window()
    la, lo = grid_nodes(lat, lon, shape)
    return _split(im.illuminate(scene(), dem(), la, lo, _all_tables()[0]))


# ---- the series ----------------------------------------------------------------------------------------------------------------
class Epoch:
    """An epoch row as the attributes illum_model reads (the light and Moon frame of one date)."""
    def __init__(self, row, base):
        self.light_pos, self.light_radius, self.light_radiance = row[0:3], row[3], row[4]
        self.center, self.u, self.v = row[5:8], row[8:11], row[11:14]
        self.radius, self.scene_epsilon, self.marching_step = base.radius, base.scene_epsilon, base.marching_step


@functools.lru_cache(maxsize=None)
def epochs():
    """N_EPOCHS dates ten minutes apart (the Sun moves a third of its true radius per step), the Sun's radius x SUN_FACTOR."""
    from moonrtx_amd import ephemeris as E
    t0 = datetime(2025, 3, 7, 21, 0, tzinfo=timezone.utc)
    ep = E.sun_epochs([t0 + timedelta(minutes=10 * k) for k in range(N_EPOCHS)], E.Observer(52.2, 21.0, 0.0))
    ep[:, 3] *= SUN_FACTOR
    ep.setflags(write=False)
    return ep


@functools.lru_cache(maxsize=None)
def series_points():
    """max(POINTS) points across the evening terminator of the middle epoch; a case of k points takes the first k."""
    _, lo0 = im.subsolar_latlon(Epoch(epochs()[N_EPOCHS // 2], scene()))
    lat = np.array([3.0, -11.5, 17.0, -4.0, 9.5, -17.5, 13.0])
    lon = lo0 + np.array([85.0, 83.5, 87.0, 88.5, 81.0, 86.0, 90.0])
    return lat, lon


def series_cases():
    """[(name, n_sun, points, first, count)]: every n_sun x every window length; the point count cycles through POINTS so
    that each n_sun meets each of them at several lengths; per-point window starts, except the full product at count 64."""
    out = []
    for a, n in enumerate(N_SUN):
        for b, count in enumerate(COUNTS):
            k = POINTS[(a + b) % len(POINTS)]
            rng = np.random.default_rng([n, count])
            first = None if count == 64 else rng.integers(0, N_EPOCHS - count + 1, k)
            out.append((f"n_sun {n}, {k} point(s) x {count} epochs", n, k, first, count))
    return out


@functools.lru_cache(maxsize=None)
def series_model():
    """{n_sun: dict} over series_points() x epochs(): V, flagged, cos_pos (P, m, n) and lit, irr, mu (P, m), D (P,)."""
    lat, lon = series_points()
    s, d, tab = scene(), dem(), _all_tables()[0]
    per = [_split(im.illuminate(Epoch(row, s), d, lat, lon, tab)) for row in epochs()]
    out = {}
    for n in N_SUN:
        out[n] = {k: np.stack([e[n][k] for e in per], 1) for k in ("V", "flagged", "cos_pos", "lit", "irr", "mu")}
        out[n]["D"] = per[0][n]["D"]
    return out


def series_window(table, k, first, count):
    """Rows [first[p], first[p] + count) of the first k points of a (P, m, ...) table: (k, count, ...)."""
    f = np.zeros(k, int) if first is None else np.asarray(first)
    return np.stack([table[p, f[p]:f[p] + count] for p in range(k)])


# ---- the lane map, restated, with named defects --------------------------------------------------------------------------------
def launch(rows, cols, n_sun, kind="grid"):
    """What the launcher decides: (PW, PH, waves_x, waves_y).  A grid band takes section 4.8's block, or 64 / n_sun nodes
    side by side when it has one row; a series (rows = points, cols = the window's epochs) takes 64 / n_sun epochs, narrowed
    to the least power of two >= cols."""
    P = 64 // n_sun
    if kind == "grid":
        PW = P if rows == 1 else GRID_BLOCK[n_sun][0]
    else:
        PW = 1
        while PW < min(cols, P):
            PW *= 2
    PH = P // PW
    return PW, PH, -(-cols // PW), -(-rows // PH)


def lanes(rows, cols, n_sun, kind="grid", mutant=None):
    """Every lane of every wave of a call: dict of (waves, 64) arrays row, col, sample, inside (row / col may lie past the
    edge where inside is False), and the launch's PW, PH.  Wave w is block (w // waves_x, w % waves_x) of the band; lane l
    holds sample l % n_sun of the block's node l // n_sun, nodes in raster order over the block's PW columns.

    mutant names one deliberate defect (MUTANTS); the four layout defects are a kernel decoding the block with another width
    than the launcher laid the waves out for -- a kernel and a launcher that agree on any layout report the same map:
      pw_too_wide             the kernel's block is 2 PW wide (pw_log2 one too large);
      pw_ph_swapped           the kernel's block is PH wide;
      one_row_ignored         a one-row band's waves are laid out for PW = 64 / n_sun, the kernel's block keeps the grid's PW
                              (the special case applied after pw_log2 was taken);
      series_pw_not_narrowed  a series' waves are laid out for the narrowed PW, the kernel's block is 64 / n_sun wide;
      sample_shifted          the Sun table is read at l // n_sun, the node's place in the block (taken modulo n_sun: the table
                              ends there), not at l % n_sun;
      group_sum_2n, edge_lanes_not_zeroed   defects of the reduction: see report()."""
    assert mutant is None or mutant in MUTANTS
    P = 64 // n_sun
    PW, PH, waves_x, waves_y = launch(rows, cols, n_sun, kind)
    kw = PW                                                     # the block width the kernel decodes with
    if mutant == "pw_too_wide":
        kw = 2 * PW
    elif mutant == "pw_ph_swapped":
        kw = PH
    elif mutant == "one_row_ignored" and kind == "grid" and rows == 1:
        kw = GRID_BLOCK[n_sun][0]
    elif mutant == "series_pw_not_narrowed" and kind == "series":
        kw = P
    kh = P // kw                                                # ... and its height (0 when the block is wider than P)
    lane = np.arange(64)
    node = lane // n_sun
    wave = np.arange(waves_x * waves_y)[:, None]
    row = (wave // waves_x) * kh + (node // kw)[None, :]
    col = (wave % waves_x) * kw + (node % kw)[None, :]
    sample = (node % n_sun if mutant == "sample_shifted" else lane % n_sun)[None, :] + 0 * wave
    return dict(row=row, col=col, sample=sample, inside=(row < rows) & (col < cols), rows=rows, cols=cols, n_sun=n_sun,
                PW=PW, PH=PH, mutant=mutant)


def coverage(L):
    """(rows cols, n_sun) counts: how many lanes inside the band hold each (node, sample)."""
    cnt = np.zeros((L["rows"] * L["cols"], L["n_sun"]), int)
    i = L["inside"]
    np.add.at(cnt, (L["row"][i] * L["cols"] + L["col"][i], L["sample"][i]), 1)
    return cnt


def report(L, V, cos_pos):
    """What a kernel with the lane map L reports from the per-sample tables V and cos_pos ((rows cols, n_sun) bool):
    (lit (rows cols,) float64, NaN where no lane stored; stores (rows cols,) int, how many lanes stored there; shadow_rays).
    Every lane inside the band takes V of its (node, sample), a lane past the edge 0; the n_sun lanes of a node are summed
    by an xor butterfly over lane distances 1, 2, ..., n_sun / 2; the node's first lane stores sum / n_sun if it is inside;
    shadow_rays is the wave's sum of the lanes' cos_pos, past-the-edge lanes counting 0.
      group_sum_2n            the butterfly goes one round further, to distance n_sun (a partner past lane 63 hands back the
                              lane's own value, as the cross-lane read of a 64-lane wave does);
      edge_lanes_not_zeroed   a lane past the edge works on the nearest node inside (row and column clamped) and feeds what
                              it finds into the sum and the counter."""
    rows, cols, n = L["rows"], L["cols"], L["n_sun"]
    inside = L["inside"]
    at = np.minimum(L["row"], rows - 1) * cols + np.minimum(L["col"], cols - 1)
    live = np.ones_like(inside) if L["mutant"] == "edge_lanes_not_zeroed" else inside
    val = np.where(live, V[at, L["sample"]], False).astype(np.float64)
    rays = int(np.where(live, cos_pos[at, L["sample"]], False).sum())
    lane = np.arange(64)
    d = 1
    while d < (2 * n if L["mutant"] == "group_sum_2n" else n):
        partner = lane ^ d
        val = val + val[:, np.where(partner < 64, partner, lane)]
        d *= 2
    store = inside & (lane % n == 0)[None, :]
    lit = np.full(rows * cols, np.nan)
    stores = np.zeros(rows * cols, int)
    lit[at[store]] = val[store] / n
    np.add.at(stores, at[store], 1)
    return lit, stores, rays
