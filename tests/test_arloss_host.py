"""CPU: the alignment-restricted RNN-T loss's host side.  The float64 restatement tests/arloss_ref.py that the GPU tests
compare against is pinned here - against the enumeration of every window-respecting alignment, against autograd of the
masked recursion, its band formula against isfinite(alpha) & isfinite(beta) - and every argument error is raised before
anything is launched."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import arloss_ref as AR
import fastemit_ref as FR


def _windows(rng, T, U, kind):
    if kind == 0:            # around a valid alignment: always feasible
        fr = np.sort(rng.integers(0, T, size=U))
        lo = np.maximum(0, fr - int(rng.integers(0, 3)))
        hi = np.minimum(T - 1, fr + int(rng.integers(0, 3)))
    elif kind == 1:          # independent windows: often infeasible
        lo = rng.integers(0, T, size=U)
        hi = np.minimum(T - 1, lo + rng.integers(0, 3, size=U))
    else:                    # unclipped values: lo < 0, hi >= T, now and then lo > hi
        lo = rng.integers(-2, T + 1, size=U)
        hi = lo + rng.integers(-1, T + 2, size=U)
    return lo, hi


def _cases(n, seed):
    rng = np.random.default_rng(seed)
    for trial in range(n):
        T, U, V = int(rng.integers(1, 7)), int(rng.integers(0, 5)), 5
        z = 2.0 * rng.normal(size=(T, U + 1, V))
        labels = rng.integers(1, V, size=U)
        lo, hi = _windows(rng, T, U, trial % 3)
        yield T, U, z, labels, lo, hi


def test_restatement_equals_the_enumeration_and_infeasible_iff_a_window_pair_crosses():
    """T <= 6, U <= 4: cost = -log sum over every window-respecting alignment; no alignment <=> elo_u > ehi_u for some
    u <=> cost +inf with an all-zero gradient; the band formula = isfinite(alpha) & isfinite(beta)."""
    infeasible = 0
    for T, U, z, labels, lo, hi in _cases(300, 0):
        lpb, lpl = FR.cell_logprobs(z, labels, T, U)
        total, best, arg, n = AR.ar_enumerate(lpb, lpl, lo, hi)
        cost, g, live = AR.ar_grad_one(z, labels, T, U, lo, hi)
        band_live, feasible, band = AR.band_one(T, U, lo, hi)
        assert feasible == (n > 0)
        assert (live == band_live).all(), (lo, hi)
        assert (AR.live_from_band(band[None], U + 1)[0] == live).all()
        score, frames = AR.ar_viterbi_one(lpb, lpl, lo, hi)
        if n == 0:
            infeasible += 1
            assert cost == np.inf and not g.any() and not live.any()
            assert score == -np.inf and (frames == -1).all()
            continue
        assert abs(-cost - total) <= 1e-10
        assert not np.isnan(g).any() and not g[~live].any()
        assert np.abs(g.sum(-1)).max() <= 1e-12                      # live rows still sum to zero
        assert score == pytest.approx(best, abs=1e-12) and AR.respects(frames, lo, hi)
        if len(arg) == 1:
            assert tuple(frames) == arg[0]
    assert 30 < infeasible < 200


@pytest.mark.parametrize("lam", [0.0, 0.5])
def test_gradient_formula_equals_autograd_of_the_masked_recursion(lam):
    seen = 0
    for T, U, z, labels, lo, hi in _cases(90, 1):
        ref = AR.ar_autograd_one(z, labels, T, U, lo, hi, lam)
        cost, g, _ = AR.ar_grad_one(z, labels, T, U, lo, hi, lam)
        if ref is None:
            assert cost == np.inf
            continue
        seen += 1
        assert abs(cost - ref[0]) <= 1e-12 * max(1.0, abs(ref[0]))
        assert np.abs(g - ref[1]).max() <= 1e-12
    assert seen > 30


def test_covering_windows_are_the_plain_loss_and_single_frame_windows_a_single_path():
    rng = np.random.default_rng(2)
    T, U, V = 6, 4, 7
    z = 2.0 * rng.normal(size=(T, U + 1, V))
    labels = rng.integers(1, V, size=U)
    for lam in (0.0, 0.5):
        cost, g, live = AR.ar_grad_one(z, labels, T, U, [0] * U, [T - 1] * U, lam)
        c0, g0 = FR.fastemit_grad_one(z, labels, T, U, lam)
        assert cost == c0 and np.abs(g - g0).max() <= 1e-15 and live.all()
    frames = np.sort(rng.integers(0, T, size=U))
    cost, _, live = AR.ar_grad_one(z, labels, T, U, frames, frames)
    lpb, lpl = FR.cell_logprobs(z, labels, T, U)
    assert cost == pytest.approx(-FR.path_score(lpb, lpl, frames), abs=1e-12)
    assert live.sum() == T + U                                       # the path's cells and no other


def test_window_helpers_match_their_definitions():
    lo, hi = AR.windows_from_frames(np.array([[0, 3, 3, -1], [1, -1, -1, -1]]), [5, 2], [3, 1], 2, 1, Tm=5)
    assert lo.tolist() == [[0, 1, 1, 0], [0, 0, 0, 0]] and hi.tolist() == [[1, 4, 4, 4], [1, 4, 4, 4]]
    band, cells = AR.band_table(lo, hi, [5, 2], [3, 1], 5)
    assert band[0].tolist() == [[0, 1], [0, 3], [1, 3], [1, 3], [1, 3]] and cells[0] == 2 + 4 + 3 + 3 + 3
    assert band[1].tolist() == [[0, 1], [0, 1], [0, -1], [0, -1], [0, -1]] and cells[1] == 4


def test_windows_are_validated_like_labels_and_keyword_only():
    from edgedict_amd import loss
    from edgedict_amd.models import Transducer
    from edgedict_amd.trainer import TrainEngine
    lo = torch.zeros(2, 3, dtype=torch.int32)
    assert loss.check_windows((lo, lo), 2, 3, lo.device) == (lo, lo)
    with pytest.raises(TypeError, match="int32"):
        loss.check_windows((lo.long(), lo), 2, 3, lo.device)
    with pytest.raises(ValueError, match=r"\[B,U\]"):
        loss.check_windows((lo, lo[:, :2]), 2, 3, lo.device)
    with pytest.raises(ValueError, match="contiguous"):
        loss.check_windows((lo.t().contiguous().t(), lo), 2, 3, lo.device)
    with pytest.raises(TypeError, match="pair"):
        loss.check_windows(lo, 2, 3, lo.device)
    with pytest.raises(ValueError, match=">= 0"):
        loss.alignment_windows(lo, torch.ones(2, dtype=torch.int32), torch.ones(2, dtype=torch.int32), -1, 0)
    for fn in (loss.RNNTLoss.forward, loss.rnnt_align, Transducer.forward, Transducer.align, TrainEngine.train_step):
        p = inspect.signature(fn).parameters["windows"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None, fn
    # the reference's positional call surface is unchanged
    assert list(inspect.signature(Transducer.forward).parameters)[:5] == ["self", "xs", "ys", "xlen", "ylen"]
    assert list(inspect.signature(loss.RNNTLoss.forward).parameters)[:5] == ["self", "acts", "labels", "act_lens",
                                                                              "label_lens"]
    assert list(inspect.signature(TrainEngine.train_step).parameters)[:6] == ["self", "wave", "wave_len", "ys", "ylen",
                                                                               "next_batch"]


def test_native_null_windows_and_bad_arguments_are_status_codes(hip_lib):
    """The *_ar entry points refuse null windows with ED_ERR_INVALID and a message before anything is launched (the
    device pointers below are never dereferenced); the backward family refuses a bad lambda as the *_fe one does."""
    fake = ctypes.c_void_p(256)
    f = ctypes.c_float
    dims = (2, 5, 3, 16, 0)
    fwd = {
        "loss_forward_ar": lambda lo, hi: (fake, 0, fake, fake, fake, lo, hi) + dims + (fake, fake, f(1.0), fake, None),
        "loss_forward_packed_ar": lambda lo, hi: (fake, 0, fake, fake, fake, lo, hi, fake) + dims + (fake, fake, f(1.0), fake, None),
        "loss_forward_packed_parts_ar": lambda lo, hi: (fake, fake, fake, fake, lo, hi, fake) + dims + (fake, fake, f(1.0), fake, fake, 1, None),
        "align_ar": lambda lo, hi: (fake, 0, fake, fake, fake, lo, hi) + dims + (fake, fake, fake, None),
        "align_packed_ar": lambda lo, hi: (fake, 0, fake, fake, fake, lo, hi, fake) + dims + (fake, fake, fake, None),
        "align_packed_parts_ar": lambda lo, hi: (fake, fake, fake, fake, lo, hi, fake) + dims + (fake, fake, fake, fake, 1, None),
    }
    for name, args in fwd.items():
        for lo, hi in ((None, fake), (fake, None), (None, None)):
            assert getattr(hip_lib, "edgedict_rnnt_" + name)(*args(lo, hi)) == -1, name
            assert b"null windows" in hip_lib.edgedict_last_error(), name
    head = (fake, 0, fake, fake, fake, fake)
    tail = (2, 5, 3, 16, 0, fake, f(1.0), None, 0)
    for bad in (-0.5, float("nan"), float("inf")):
        calls = {
            "backward_ar": head + tail + (f(bad), None),
            "backward_packed_ar": head + (fake,) + tail + (f(bad), None),
            "backward_packed_colsum_ar": head + (fake,) + tail + (fake, f(bad), None),
            "backward_packed_range_ar": head + (fake,) + tail + (0, 2, f(bad), None),
        }
        for name, args in calls.items():
            assert getattr(hip_lib, "edgedict_rnnt_loss_" + name)(*args) == -1, (name, bad)
            assert b"fastemit_lambda" in hip_lib.edgedict_last_error(), name
    assert hip_lib.edgedict_rnnt_alignment_windows(fake, fake, fake, 2, 5, 3, -1, 0, fake, fake, None) == -1
    assert hip_lib.edgedict_rnnt_band(fake, fake, fake, fake, 2, 5, 4096, fake, fake, None) == -1
    assert hip_lib.edgedict_rnnt_band(None, fake, fake, fake, 2, 5, 3, fake, fake, None) == -1


def test_new_symbols_are_declared_and_exported(hip_lib):
    from edgedict_amd import _lib
    want = {"edgedict_rnnt_loss_forward_ar", "edgedict_rnnt_loss_forward_packed_ar",
            "edgedict_rnnt_loss_forward_packed_parts_ar", "edgedict_rnnt_loss_backward_ar",
            "edgedict_rnnt_loss_backward_packed_ar", "edgedict_rnnt_loss_backward_packed_colsum_ar",
            "edgedict_rnnt_loss_backward_packed_range_ar", "edgedict_rnnt_align_ar", "edgedict_rnnt_align_packed_ar",
            "edgedict_rnnt_align_packed_parts_ar", "edgedict_rnnt_alignment_windows", "edgedict_rnnt_band"}
    assert want <= set(_lib.declared_symbols())
    for name in want:
        assert hasattr(hip_lib, name), name
    assert hip_lib.edgedict_abi_version() == 2
