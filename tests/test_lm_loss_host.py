"""CPU: the host side of LM training - the float64 oracle of the softmax NLL (tests/lm_loss_ref.py) pinned against
torch.nn.functional.cross_entropy in float64, the reference's collate restated, the checkpoint LMTrainer.save writes,
and the argument errors of SoftmaxNLLLoss raised before anything is launched."""
import ctypes

import numpy as np
import pytest
import torch

import lm_loss_ref as R
from test_lm_fusion_host import _ref_keyed_sd


def _case(M=11, V=13, ignore_index=0, seed=0):
    rng = np.random.default_rng(seed)
    z = 3.0 * rng.standard_normal((M, V))
    t = rng.integers(0, V, size=M)
    t[::3] = ignore_index
    z[1, t[1]] += 90.0
    z[2, (t[2] + 1) % V] += 90.0
    return z, t


@pytest.mark.parametrize("ignore_index", [0, -100, 5])
@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
def test_oracle_matches_torch_cross_entropy_in_float64(reduction, ignore_index):
    z, t = _case(ignore_index=ignore_index)
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    tt = torch.tensor(t, dtype=torch.long)
    want = torch.nn.functional.cross_entropy(zt, tt, ignore_index=ignore_index, reduction=reduction)
    rng = np.random.default_rng(1)
    go = rng.uniform(0.25, 1.0, size=len(t)) if reduction == "none" else 0.7
    want.backward(torch.tensor(go, dtype=torch.float64))
    loss, nll, lse, dz = R.softmax_nll(z, t, ignore_index, reduction, go)
    np.testing.assert_allclose(loss, want.detach().numpy(), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(dz, zt.grad.numpy(), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(lse, torch.logsumexp(zt.detach(), 1).numpy(), rtol=1e-13)
    ok = R.valid_rows(t, z.shape[1], ignore_index)
    assert (nll[~ok] == 0).all() and (dz[~ok] == 0).all() and ok.any() and (~ok).any()


def test_oracle_ignores_out_of_range_targets_and_zero_valid_rows_give_zero():
    z, t = _case()
    t2 = t.copy()
    t2[1], t2[4] = z.shape[1], -7             # out of range: ignored, as if they were ignore_index
    t3 = t.copy()
    t3[1] = t3[4] = 0
    for red in ("none", "sum", "mean"):
        a, b = R.softmax_nll(z, t2, 0, red), R.softmax_nll(z, t3, 0, red)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)
    for red in ("sum", "mean"):
        loss, nll, _, dz = R.softmax_nll(z, np.zeros(len(t), dtype=np.int64), 0, red, 0.7)
        assert loss == 0.0 and not nll.any() and not dz.any()


def test_oracle_log_softmax_backward_matches_autograd():
    rng = np.random.default_rng(2)
    x = torch.tensor(3.0 * rng.standard_normal((5, 9)), dtype=torch.float64, requires_grad=True)
    dy = rng.standard_normal((5, 9))
    y = torch.log_softmax(x, -1)
    y.backward(torch.tensor(dy))
    np.testing.assert_allclose(R.log_softmax(x.detach().numpy()), y.detach().numpy(), rtol=1e-13, atol=1e-14)
    np.testing.assert_allclose(R.log_softmax_bwd(y.detach().numpy(), dy), x.grad.numpy(), rtol=1e-12, atol=1e-14)


def test_seq_collate_is_the_reference_collate():
    from edgedict_amd.lm import seq_collate
    inputs, targets = seq_collate([torch.tensor([5, 6, 7]), torch.tensor([8]), torch.tensor([9, 3])])
    assert inputs.dtype == targets.dtype == torch.long
    assert targets.tolist() == [[5, 6, 7], [8, 0, 0], [9, 3, 0]]
    assert inputs.tolist() == [[1, 5, 6], [1, 8, 0], [1, 9, 3]]


@pytest.mark.parametrize("tied", [False, True])
def test_trainer_save_writes_the_reference_keyed_state_dict(tmp_path, tied):
    from edgedict_amd.lm import LMModel, LMTrainer
    ninp = 32 if tied else 16
    sd = _ref_keyed_sd(40, ninp, 32, 2)
    if tied:
        sd["decoder.weight"] = sd["encoder.weight"]
    lm = LMModel(40, ninp, 32, 2, tie_weights=tied)
    lm.load_state_dict(sd, strict=True)
    tr = LMTrainer(lm)
    path = str(tmp_path / "lm.pt")
    tr.save(path)
    got = torch.load(path)
    assert list(got) == list(lm.state_dict()) and set(got) == set(sd)
    for k, v in sd.items():
        assert got[k].shape == v.shape and got[k].dtype == torch.float32 and got[k].device.type == "cpu", k
        assert torch.equal(got[k], v), k
    fresh = LMModel(40, ninp, 32, 2, tie_weights=tied)
    fresh.load_state_dict(got, strict=True)
    tr2 = LMTrainer(fresh)
    tr2.load(path)
    assert all(torch.equal(a, b) for a, b in zip(fresh.state_dict().values(), lm.state_dict().values()))
    assert len(tr.optimizer.flat.params) == (8 + 2 if tied else 8 + 3)     # the tied weight is ONE parameter


def test_check_targets_raises_before_any_launch():
    """CPU tensors: anything that reached a launch would raise RuntimeError (no CPU fallback), not ValueError."""
    from edgedict_amd.loss import SoftmaxNLLLoss
    z = torch.zeros(4, 7)
    with pytest.raises(ValueError, match="outside"):
        SoftmaxNLLLoss(ignore_index=0, check_targets=True)(z, torch.tensor([1, 7, 0, 2]))
    with pytest.raises(ValueError, match="outside"):
        SoftmaxNLLLoss(ignore_index=0, check_targets=True)(z, torch.tensor([1, -1, 0, 2]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):      # -100 is the ignore_index: passes the check
        SoftmaxNLLLoss(check_targets=True)(z, torch.tensor([1, -100, 0, 2]))
    with pytest.raises(ValueError, match="shape"):
        SoftmaxNLLLoss()(z, torch.tensor([1, 2, 3]))
    with pytest.raises(TypeError):
        SoftmaxNLLLoss()(z.double(), torch.tensor([1, 2, 3, 4]))
    with pytest.raises(TypeError):
        SoftmaxNLLLoss()(z, torch.tensor([1., 2., 3., 4.]))
    with pytest.raises(ValueError, match="reduction"):
        SoftmaxNLLLoss(reduction="batchmean")


def test_cpu_tensors_raise_the_no_cpu_fallback_error():
    from edgedict_amd.lm import LMModel
    from edgedict_amd.loss import SoftmaxNLLLoss, softmax_nll_rows
    z, t = torch.zeros(4, 7), torch.tensor([1, 2, 0, 3])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SoftmaxNLLLoss(ignore_index=0)(z, t)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        softmax_nll_rows(z, t.int())
    lm = LMModel(40, 16, 32, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lm.loss(torch.zeros(1, 3, dtype=torch.long), torch.ones(1, 3, dtype=torch.long))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lm.score(torch.ones(1, 3, dtype=torch.long), torch.tensor([3]))


def test_native_argument_errors_are_status_codes(hip_lib):
    """The entry points validate before they touch the device: the pointers below are never dereferenced."""
    fake = ctypes.c_void_p(256)
    ll = ctypes.c_longlong
    fwd, bwd = hip_lib.edgedict_softmax_nll_forward, hip_lib.edgedict_softmax_nll_backward
    assert fwd(7, fake, ll(8), fake, 2, 8, 0, fake, fake, fake, fake, 1, None) == -1
    assert b"dtype" in hip_lib.edgedict_last_error()
    assert fwd(0, fake, ll(7), fake, 2, 8, 0, fake, fake, fake, fake, 1, None) == -1
    assert b"shape" in hip_lib.edgedict_last_error()
    assert fwd(0, fake, ll(8), fake, 2, 8, 0, fake, fake, None, fake, 1, None) == -1
    assert b"stats" in hip_lib.edgedict_last_error()
    assert fwd(0, None, ll(8), fake, 2, 8, 0, fake, fake, fake, fake, 1, None) == -1
    assert b"null" in hip_lib.edgedict_last_error()
    assert bwd(0, fake, ll(8), fake, 2, 8, 0, fake, fake, 2, fake, 1, None) == -1
    assert b"grad_stride" in hip_lib.edgedict_last_error()
    assert bwd(0, fake, ll(8), fake, 2, 8, 0, fake, fake, 0, None, 1, None) == -1
    assert b"mean" in hip_lib.edgedict_last_error()
    assert bwd(1, fake, ll(8), fake, 0, 8, 0, fake, fake, 0, fake, 1, None) == 0      # no rows: nothing to launch
    assert hip_lib.edgedict_log_softmax_rows_bwd(fake, fake, ll(4), 0, fake, 2, 8, None) == -1
    assert hip_lib.edgedict_abi_version() == 2
