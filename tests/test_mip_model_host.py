"""tests/mip_model.py on the CPU: the model of the march's skip structures satisfies the consumers' covering invariants on every
ragged shape, and each invariant REJECTS a model with one undersized cell.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import mip_model as mm

SHAPES = [(2, 2), (3, 5), (16, 32), (17, 33), (31, 47), (64, 129), (130, 257), (366, 731)]
LOW = np.float32(0.955)       # above spiked_dem's noise (< 0.95), below every spike (>= 0.96)


def test_shift_rule():
    """cell = 2^shift >= 16 step / texel + 3.5 within 16 .. 1024 texels; a quarter of it, never below 4; eight times it."""
    assert mm.shifts(64, 129, 10.0, 5e-3) == (4, 2, 7)
    texel = np.pi * 10.0 / 130          # the smaller of the row and the column pitch (2 pi 10 / 257)
    assert mm.shifts(130, 257, 10.0, texel * (16 - 3.5) / 16 * 0.999) == (4, 2, 7)
    assert mm.shifts(130, 257, 10.0, texel * (16 - 3.5) / 16 * 1.001) == (5, 3, 8)
    assert mm.shifts(130, 257, 10.0, texel * (512 - 3.5) / 16 * 1.001) == (10, 8, 13)
    assert mm.shifts(130, 257, 10.0, 1e6) == (10, 8, 13)
    assert mm.mip_info(366, 731, 10.0, 5e-3) == (4, 23, 46, 2, 92, 183, 7, 3, 6)


def test_row_pair_copies_against_np_pad():
    for h, w in SHAPES:
        D = mm.spiked_dem(h, w)
        P = np.pad(np.pad(D, ((2, 3), (0, 0)), mode="edge"), ((0, 0), (2, 2)), mode="wrap")
        got = mm.padded_dem(D)
        assert got.shape == (h + 4, w + 4, 2) and got.dtype == np.float32
        assert np.array_equal(got[..., 0], P[:-1]) and np.array_equal(got[..., 1], P[1:])
        T = mm.noise_colour(h + 1, w + 3)
        t = T.view("<u4")[..., 0]
        Q = np.pad(np.pad(t, ((1, 1), (0, 0)), mode="edge"), ((0, 0), (2, 2)), mode="wrap")
        cp = mm.colour_pairs(T)
        assert cp.shape == (h + 2, w + 7, 2) and cp.dtype == np.uint32
        assert np.array_equal(cp[..., 0], Q[:-1]) and np.array_equal(cp[..., 1], Q[1:])


@pytest.mark.parametrize("shift", [4, 5, 6, 9])
def test_the_model_satisfies_its_consumers(shift):
    """A, B and H on every shape, at the default shift, the next two, and one whose cells exceed every map here."""
    for h, w in SHAPES:
        for interior in (False, True):
            D = mm.spiked_dem(h, w, shift, interior=interior)
            m2 = max(shift - 2, 2)
            assert mm.check_A(mm.max_mip(D, shift), D, shift) == [], (h, w)
            assert mm.check_B(mm.medium_mip(D, m2), D, m2) == [], (h, w)
            assert mm.check_H(mm.horizon_mip(D, shift), D, shift + 3) == [], (h, w)


def own_columns_border(D, M, shift):
    """The sabotage "a border cell that is not wrapped": border column j = -1 built from the clamped neighbour's columns
    [0, C + 1] instead of the wrapped cell mw - 1."""
    C = 1 << shift
    S = mm.bordered(M).copy()
    for i in range(-1, M.shape[0] + 1):
        ic = min(max(i, 0), M.shape[0] - 1)
        S[i + 1, 0] = mm.window(D, C * ic - 2, min(C * ic + C + 1, D.shape[0] + 1), 0, C + 1).max()
    return S


@pytest.mark.parametrize("shape", [(130, 257), (366, 731)])
def test_invariant_A_rejects_an_undersized_cell(shape):
    h, w = shape
    s = 4
    D = mm.spiked_dem(h, w, s)
    M = mm.mip_cells(D, s)
    mh, mw = M.shape
    assert w % (1 << s) != 0 and h % (1 << s) != 0
    for i, j in ((((2 * h) // 3) >> s, mw - 1),        # the partial cell at the seam: the spike on column w - 1
                 (0, (w // 3) >> s),                    # a pole row: the spike on row 0
                 (mh - 1, (w // 2 + 1) >> s)):          # the partial last row: the spike on row h - 1
        bad = M.copy()
        bad[i, j] = LOW
        got = mm.check_A(mm.row_pairs(mm.bordered(bad)), D, s)
        assert ("small", i, j) in got, (i, j, got)
    # one ulp is enough where the cell's maximum is one of its own texels
    i, j = ((2 * h) // 3) >> s, mw - 1
    bad = M.copy()
    bad[i, j] = np.nextafter(bad[i, j], np.float32(0))
    assert ("small", i, j) in mm.check_A(mm.row_pairs(mm.bordered(bad)), D, s)
    # a border cell that is not wrapped
    got = mm.check_A(mm.row_pairs(own_columns_border(D, M, s)), D, s)
    assert ("small", ((2 * h) // 3) >> s, -1) in got and all(g[2] == -1 for g in got), got
    # ... whereas a border that CLAMPS to its dilated neighbour still covers: the two-texel dilation reaches across the seam,
    # so A cannot tell it from a wrapped one -- the bit-equality with the model does
    S = mm.bordered(M).copy()
    S[:, 0], S[:, -1] = S[:, 1], S[:, -2]
    assert mm.check_A(mm.row_pairs(S), D, s) == [] and not np.array_equal(S, mm.bordered(M))
    # the pairing: a last row paired with the wrong row (the row above it holds the same clamped cells, so: the first row),
    # a second component off by one cell
    P = mm.max_mip(D, s).copy()
    P[-1, :, 1] = P[0, :, 0]
    got = mm.check_A(P, D, s)
    assert got and all(g[:2] == ("pair", mh) for g in got), got
    P = mm.max_mip(D, s).copy()
    P[1, 2, 1] = P[1, 2, 0]
    assert mm.check_A(P, D, s) == [("pair", 0, 1)]


@pytest.mark.parametrize("shape", [(130, 257), (366, 731)])
def test_invariant_B_rejects_an_undersized_cell(shape):
    h, w = shape
    s = 2
    D = mm.spiked_dem(h, w, s)
    M = mm.mip_cells(D, s)
    mh, mw = M.shape
    for i, j in ((((2 * h) // 3) >> s, mw - 1), (0, (w // 3) >> s), (mh - 1, (w // 2 + 1) >> s)):
        bad = M.copy()
        bad[i, j] = LOW
        assert ("small", i, j) in mm.check_B(mm.bordered(bad), D, s), (i, j)
    got = mm.check_B(own_columns_border(D, M, s), D, s)
    assert ("small", ((2 * h) // 3) >> s, -1) in got and all(g[2] == -1 for g in got), got
    # the row border: the position row -1 reads border row -1, which must cover texel row 0
    S = mm.bordered(M).copy()
    S[0, :] = LOW
    assert ("small", -1, (w // 3) >> s) in mm.check_B(S, D, s)


@pytest.mark.parametrize("shape", [(130, 300), (366, 731)])
def test_invariant_H_rejects_an_undersized_cell(shape):
    h, w = shape
    s = 4
    hs, Cc = s + 3, 1 << (s + 3)
    D = mm.spiked_dem(h, w, s)
    Hm = mm.horizon_mip(D, s)
    hh, hw = Hm.shape
    assert hw > 1 and w % Cc != 0
    for i, j in ((((2 * h) // 3) >> hs, hw - 1), (0, (w // 3) >> hs), (hh - 1, (w // 2 + 1) >> hs)):
        bad = Hm.copy()
        bad[i, j] = LOW
        assert [g[:3] for g in mm.check_H(bad, D, hs)] == [("small", i, j)], (i, j)
    # a column window that is not wrapped: cell (i, 0) built from the clamped columns misses a spike on column w - 3, the
    # map's highest so that no other spike of the cell's window stands in for it (columns w - 2 and w - 1 would not do: the
    # first fine cell's own two-texel dilation reaches them across the seam)
    D = D.copy()
    D[(2 * h) // 3, w - 3] = np.float32(0.999)
    Hm = mm.horizon_mip(D, s)
    i = ((2 * h) // 3) >> hs
    M = mm.mip_cells(D, s)
    fi = np.unique(np.clip(np.arange(Cc * i - Cc, Cc * i + 2 * Cc), 0, h - 1) >> s)
    fj = np.unique(np.clip(np.arange(-Cc, 2 * Cc), 0, w - 1) >> s)
    bad = Hm.copy()
    bad[i, 0] = M[np.ix_(fi, fj)].max()
    assert [g[:3] for g in mm.check_H(bad, D, hs)] == [("small", i, 0)]


def seam_ridge(w):
    """The terrain of test_gpu_parity.seam_ridge_case at a width of choice: a meridian ridge on columns 723..727."""
    rng = np.random.default_rng(4)
    D = np.full((366, w), 0.992, np.float32) + rng.random((366, w)).astype(np.float32) * np.float32(2e-4)
    D[:, 723:728] = 1.0
    return D


def test_seam_regression_needs_the_partial_cell():
    """hmip_build_kernel's former defect, restated in the model (seam_bug): stepping the columns by a fine cell across the seam
    never reaches the last, partial fine cell.  H sees it at 731 columns (731 = 45 x 16 + 11: the ridge lies in the partial
    cell) in the cells (i, 0) that look west across the seam, and has nothing to see at 736 = 46 x 16."""
    D = seam_ridge(731)
    assert mm.check_H(mm.horizon_mip(D, 4), D, 7) == []
    got = mm.check_H(mm.horizon_mip(D, 4, seam_bug=True), D, 7)
    assert [g[:3] for g in got] == [("small", i, 0) for i in range(3)], got
    D = seam_ridge(736)
    assert np.array_equal(mm.horizon_mip(D, 4, seam_bug=True), mm.horizon_mip(D, 4))
    assert mm.check_H(mm.horizon_mip(D, 4, seam_bug=True), D, 7) == []
    # the GPU layout test's own terrain: spikes on the first and the last texel of the partial cell are held by the neighbouring
    # cells' two-texel borders as well, so the defect would go unseen there; the spike in the cell's middle shows it
    D = mm.spiked_dem(366, 731)
    assert np.array_equal(mm.horizon_mip(D, 4, seam_bug=True), mm.horizon_mip(D, 4))
    D = mm.spiked_dem(366, 731, interior=True)
    assert not np.array_equal(mm.horizon_mip(D, 4, seam_bug=True), mm.horizon_mip(D, 4))
    assert [g[:3] for g in mm.check_H(mm.horizon_mip(D, 4, seam_bug=True), D, 7)] == [("small", i, 0) for i in range(3)]


def test_mip_info_refuses_null_arguments(native_lib):
    out = (C.c_int32 * 9)()
    assert native_lib.mrtx_mip_info(None, out) == -1
