"""CPU: the band-packed lattice's layout (tests/band_ref.py) and the argument the band route of the loss rests on, in
float64: with lp_blank = lp_label = -inf written on every dead cell of the box, the lattice recursion gives the SAME
alpha and beta on the live cells and the same likelihood as the window-masked recursion of the box path - a dead cell
only ever contributed -inf there, through its alpha or its beta."""
import warnings

import numpy as np
import pytest
import torch

import arloss_ref as AR
import band_ref as BR
import test_arloss_gpu as TA
import test_fastemit_gpu as TF
from oracle.rnnt_loss_ref import lattice

P_B, P_T, P_U1, P_AL, P_LL = TF.P_B, TF.P_T, TF.P_U1, TF.P_AL, TF.P_LL
W_B, W_T, W_U1 = 3, 40, 80
W_AL, W_LL = [40, 31, 40], [79, 12, 30]


def p_windows(kind, V):
    """box set P: 'align00' / 'align21' around random_alignment(default_rng(V)), 'infeasible', 'cover'"""
    if kind in ("infeasible", "cover"):
        return TA._packed_windows(kind, V)
    frames = AR.random_alignment(np.random.default_rng(V), P_AL, P_LL, P_U1 - 1)
    left, right = (0, 0) if kind == "align00" else (2, 1)
    lo, hi = AR.windows_from_frames(frames, P_AL, P_LL, left, right, Tm=P_T)
    return lo.astype(np.int32), hi.astype(np.int32)


def w_windows(left, right):
    """shape W: windows around random_alignment(default_rng(1))"""
    frames = AR.random_alignment(np.random.default_rng(1), W_AL, W_LL, W_U1 - 1)
    lo, hi = AR.windows_from_frames(frames, W_AL, W_LL, left, right, Tm=W_T)
    return lo.astype(np.int32), hi.astype(np.int32)


P_KINDS = ("align00", "align21", "infeasible", "cover")
W_SLACKS = ((0, 0), (2, 1), (5, 5))


def all_cases():
    for V in (264, 1024):
        for kind in P_KINDS:
            yield "P-%s-%d" % (kind, V), P_AL, P_LL, P_T, P_U1, p_windows(kind, V)
    for slack in W_SLACKS:
        yield "W-%d%d" % slack, W_AL, W_LL, W_T, W_U1, w_windows(*slack)


def test_the_shapes_are_the_ones_the_gpu_tests_count_on():
    assert sum(t * (u + 1) for t, u in zip(P_AL, P_LL)) == 331
    assert sum(t * (u + 1) for t, u in zip(W_AL, W_LL)) == 4843
    for V in (264, 1024):
        band, cells = AR.band_table(*p_windows("align00", V), P_AL, P_LL, P_T)
        assert cells.sum() == 98 and (band[:, :, 1] - band[:, :, 0] + 1).max() <= 4
        band, cells = AR.band_table(*p_windows("align21", V), P_AL, P_LL, P_T)
        assert 148 <= cells.sum() <= 149 and (band[:, :, 1] - band[:, :, 0] + 1).max() <= 6
        band, cells = AR.band_table(*p_windows("infeasible", V), P_AL, P_LL, P_T)
        assert cells[2] == 0 and cells.sum() > 0
        band, cells = AR.band_table(*p_windows("cover", V), P_AL, P_LL, P_T)
        assert cells.sum() == 331
    want = {(0, 0): 232, (2, 1): 586, (5, 5): 1363}
    for slack in W_SLACKS:
        band, cells = AR.band_table(*w_windows(*slack), W_AL, W_LL, W_T)
        assert cells.sum() == want[slack], (slack, cells.sum())
        assert 90 <= ((band[:, :, 0] > 0) & (band[:, :, 1] >= band[:, :, 0])).sum() <= 111


def test_offsets_pack_and_unpack_round_trip():
    rng = np.random.default_rng(0)
    for name, al, ll, T, U1, (lo, hi) in all_cases():
        band, cells = AR.band_table(lo, hi, al, ll, T)
        row_off, rows = BR.band_offsets(band)
        assert rows == cells.sum() and row_off.shape == (len(al), T) and row_off.dtype == np.int64
        b, t, u = BR.band_cells(band)
        assert len(b) == rows
        assert (row_off[b, t] + (u - band[b, t, 0]) == np.arange(rows)).all(), name      # the layout's definition
        assert (np.diff(row_off.reshape(-1)) >= 0).all()
        live = AR.live_from_band(band, U1)
        assert live.sum() == rows and live[b, t, u].all()
        assert (BR.band_row_tu(band) == (t << 16 | u)).all()
        for x in (rng.normal(size=(len(al), T, U1, 3)), torch.tensor(rng.normal(size=(len(al), T, U1)))):
            y = BR.band_pack(x, band)
            assert y.shape[0] == rows
            back = BR.band_unpack(y, band, -7.0, U1)
            live_t = torch.tensor(live) if torch.is_tensor(x) else live
            assert (back[live_t] == x[live_t]).all() and (back[~live_t] == -7.0).all()
            y2 = BR.band_pack(back, band)
            assert (y2 == y).all()
    # an empty table
    band = np.zeros((2, 3, 2), np.int64)
    band[:, :, 1] = -1
    row_off, rows = BR.band_offsets(band)
    assert rows == 0 and not row_off.any() and BR.band_pack(np.zeros((2, 3, 4)), band).shape == (0,)


@pytest.mark.parametrize("name,al,ll,T,U1,windows", [c for c in all_cases() if c[0].endswith("264") or c[0][0] == "W"],
                         ids=lambda v: v if isinstance(v, str) else "")
def test_minus_inf_on_dead_cells_leaves_the_live_lattice_and_the_likelihood_unchanged(name, al, ll, T, U1, windows):
    lo, hi = windows
    rng = np.random.default_rng(len(name))
    V = 9
    band, cells = AR.band_table(lo, hi, al, ll, T)
    live_all = AR.live_from_band(band, U1)
    saw_infeasible = False
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                              # logaddexp(-inf, -inf)
        for b in range(len(al)):
            Tb, Ub = int(al[b]), int(ll[b])
            z = 2.0 * rng.normal(size=(Tb, Ub + 1, V))
            labels = rng.integers(1, V, size=Ub)
            _, lpm, alpha, beta, L = AR.ar_lattice(z, labels, Tb, Ub, lo[b], hi[b])
            live = live_all[b, :Tb, :Ub + 1]
            assert (live == (np.isfinite(alpha) & np.isfinite(beta))).all()
            dead = lpm.copy()
            for t in range(Tb):
                for u in range(Ub + 1):
                    if not live[t, u]:
                        dead[t, u, 0] = -np.inf
                        if u < Ub:
                            dead[t, u, labels[u]] = -np.inf
            alpha2, beta2, L2 = lattice(dead, labels, Tb, Ub, 0)
            assert L2 == L, (name, b)
            assert (alpha2[live] == alpha[live]).all() and (beta2[live] == beta[live]).all(), (name, b)
            assert not np.isnan(alpha2).any() and not np.isnan(beta2).any()
            # a dead cell stays dead
            assert (~(np.isfinite(alpha2) & np.isfinite(beta2)))[~live].all()
            if cells[b] == 0:
                saw_infeasible = True
                assert L == -np.inf and not live.any()
    assert saw_infeasible == ("infeasible" in name)
