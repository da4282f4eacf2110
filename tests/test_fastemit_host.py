"""CPU: FastEmit's and the forced aligner's host side - the float64 oracles the GPU tests compare against are pinned
here (the gradient formula against autograd, the Viterbi against the enumeration of every alignment), and every
argument error is raised before anything is launched (Python ValueError; native status codes)."""
import ctypes
import types

import numpy as np
import pytest
import torch

import fastemit_ref as FR

CFG = dict(vocab_embed_size=8, vocab_size=40, input_size=24, enc_hidden_size=32, enc_layers=2,
           enc_proj_size=24, dec_hidden_size=16, dec_layers=2, dec_proj_size=16, joint_size=32)


@pytest.mark.parametrize("T,U,V", [(1, 0, 3), (1, 3, 5), (4, 0, 4), (5, 3, 6), (7, 4, 9)])
@pytest.mark.parametrize("lam", [0.0, 0.01, 0.5, 3.0])
def test_fastemit_formula_equals_autograd_with_scaled_label_gradient(T, U, V, lam):
    rng = np.random.default_rng(100 * T + 10 * U + V)
    z = 2.0 * rng.normal(size=(T, U + 1, V))
    labels = rng.integers(1, V, size=U)
    cost, g = FR.fastemit_grad_one(z, labels, T, U, lam)
    cost_a, g_a = FR.fastemit_autograd_one(z, labels, T, U, lam)
    assert abs(cost - cost_a) <= 1e-12 * max(1.0, abs(cost_a))
    assert np.abs(g - g_a).max() <= 1e-12
    assert np.abs(g.sum(-1)).max() <= 1e-12              # every row still sums to zero
    if lam == 0.0:
        from oracle.rnnt_loss_ref import rnnt_loss
        _, g0 = rnnt_loss(z[None], labels[None], [T], [U])
        assert np.abs(g - g0[0]).max() <= 1e-14          # lambda = 0 is the plain gradient


@pytest.mark.parametrize("T,U", [(1, 0), (1, 4), (6, 0), (2, 2), (4, 3), (6, 4), (5, 1)])
def test_viterbi_equals_the_enumeration_of_every_alignment(T, U):
    for seed in range(4):
        rng = np.random.default_rng(1000 * T + 10 * U + seed)
        z = 2.0 * rng.normal(size=(T, U + 1, 5))
        labels = rng.integers(1, 5, size=U)
        lpb, lpl = FR.cell_logprobs(z, labels, T, U)
        score, frames = FR.viterbi_one(lpb, lpl)
        best, arg = FR.viterbi_bruteforce(lpb, lpl)
        assert score == pytest.approx(best, abs=1e-12)
        assert FR.path_score(lpb, lpl, frames) == pytest.approx(best, abs=1e-12)
        if len(arg) == 1:
            assert tuple(frames) == arg[0]


def test_viterbi_tie_takes_the_blank_predecessor():
    """All log-probabilities equal: every alignment scores the same, and the documented rule (come from t - 1 while
    there is one) emits every label on frame 0."""
    lpb = np.full((4, 3), -1.0)
    lpl = np.full((4, 2), -1.0)
    score, frames = FR.viterbi_one(lpb, lpl)
    assert score == -6.0 and frames.tolist() == [0, 0]


@pytest.mark.parametrize("bad", [-0.1, float("nan"), float("inf"), -float("inf")])
def test_bad_lambda_is_a_value_error(bad):
    from edgedict_amd.loss import RNNTLoss
    from edgedict_amd.models import Transducer
    with pytest.raises(ValueError, match="fastemit_lambda"):
        RNNTLoss(fastemit_lambda=bad)
    with pytest.raises(ValueError, match="fastemit_lambda"):
        Transducer(enc_dropout=0.0, dec_dropout=0.0, fastemit_lambda=bad, **CFG)


def test_lambda_is_a_plain_attribute_and_state_dict_keys_do_not_change():
    from edgedict_amd.loss import RNNTLoss
    from edgedict_amd.models import Transducer
    plain = Transducer(enc_dropout=0.0, dec_dropout=0.0, **CFG)
    fe = Transducer(enc_dropout=0.0, dec_dropout=0.0, fastemit_lambda=0.3, **CFG)
    assert plain.fastemit_lambda == 0.0 and fe.fastemit_lambda == 0.3
    assert list(plain.state_dict()) == list(fe.state_dict())
    assert [n for n, _ in fe.named_buffers()] == [n for n, _ in plain.named_buffers()]
    assert RNNTLoss().fastemit_lambda == 0.0 and RNNTLoss(fastemit_lambda=0.25).fastemit_lambda == 0.25
    with pytest.raises(TypeError):                       # keyword-only on the model: the reference's positions stay
        Transducer(8, 40, 24, 32, 2, 0.0, 24, 16, 2, 0.0, 16, 32, [1], 0, "LSTM", True, 0.3)


def test_emission_times_follow_the_frame_geometry():
    from edgedict_amd.decode import emission_times
    flags = types.SimpleNamespace(hop_length=200, downsample=3, sample_rate=16000)
    frames = torch.tensor([[0, 1, 4, -1]], dtype=torch.int32)
    sec = emission_times(frames, flags)                  # 200 * 3 * 2 / 16000 = 75 ms per encoder frame
    assert sec.shape == frames.shape
    assert sec[0, :3].tolist() == [0.0, 0.075, 0.3] and torch.isnan(sec[0, 3])
    assert emission_times(frames, flags, time_reduction=1)[0, 1].item() == 0.0375


def test_native_lambda_errors_are_status_codes(hip_lib):
    """The four *_fe entry points refuse a negative, NaN or infinite lambda with ED_ERR_INVALID and a message before
    anything is launched (the device pointers below are never dereferenced)."""
    fake = ctypes.c_void_p(256)
    f = ctypes.c_float
    head = (fake, 0, fake, fake, fake, fake)                                   # acts, dtype, grads, labels, lens
    dims = (2, 5, 3, 16, 0, fake, f(1.0), None, 0)                             # B T U1 V blank ws scale scale_dev stride
    for bad in (-0.5, float("nan"), float("inf")):
        calls = {
            "backward_fe": head + dims + (f(bad), None),
            "backward_packed_fe": head + (fake,) + dims + (f(bad), None),
            "backward_packed_colsum_fe": head + (fake,) + dims + (fake, f(bad), None),
            "backward_packed_range_fe": head + (fake,) + dims + (0, 2, f(bad), None),
        }
        for name, args in calls.items():
            assert getattr(hip_lib, "edgedict_rnnt_loss_" + name)(*args) == -1, (name, bad)
            assert b"fastemit_lambda" in hip_lib.edgedict_last_error(), name
    # the aligner's argument checks: shape and null pointers
    assert hip_lib.edgedict_rnnt_align(fake, 0, fake, fake, fake, 2, 5, 3, 16, 16, fake, fake, fake, None) == -1
    assert b"blank" in hip_lib.edgedict_last_error()
    assert hip_lib.edgedict_rnnt_align(fake, 0, fake, fake, fake, 2, 5, 3, 16, 0, fake, None, fake, None) == -1
    assert hip_lib.edgedict_rnnt_align_packed(fake, 0, fake, fake, fake, None, 2, 5, 3, 16, 0, fake, fake, fake, None) == -1


def test_new_symbols_are_declared_and_exported(hip_lib):
    from edgedict_amd import _lib
    want = {"edgedict_rnnt_loss_backward_fe", "edgedict_rnnt_loss_backward_packed_fe",
            "edgedict_rnnt_loss_backward_packed_colsum_fe", "edgedict_rnnt_loss_backward_packed_range_fe",
            "edgedict_rnnt_align", "edgedict_rnnt_align_packed", "edgedict_rnnt_align_packed_parts"}
    assert want <= set(_lib.declared_symbols())
    assert hip_lib.edgedict_abi_version() == 2
