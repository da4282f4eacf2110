"""GPU: the fused softmax-NLL kernels (csrc/lm_loss.hip, loss.SoftmaxNLLLoss) and the row log-softmax's autograd function
against the float64 oracle tests/lm_loss_ref.py (pinned on the CPU by test_lm_loss_host.py).  For bf16 the oracle sees
the bf16-rounded logits.  Every test prints its maximum error.

Bounds: those tests/test_ctc_gpu.py states for the same arithmetic, an fp32 log-sum-exp - fp32 nll rtol 1e-5 / atol 1e-4
and gradient 1e-3 |g| + 2e-5; bf16 nll rtol 1e-4 (no absolute term) and gradient 4e-3 absolute.  The row with a +90 spike
on its target has an nll of ~1e-36, below what 1 + x resolves in float64: the oracle's value there is exactly 0, and so
is the kernel's.  The incoming gradients have magnitude <= 1, so a bf16 gradient entry (|.| <= |g_m|) is rounded by at
most 2^-9 = 1.95e-3."""
import functools

import numpy as np
import pytest
import torch

import lm_loss_ref as R

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
IGN = -100
ROWS = 4      # rows (waves) per workgroup of both kernels: LM_ROWS in csrc/lm_loss.hip

# (M, V, slice): slice = None, or (buffer width, first column) - the logits are a column slice of a wider buffer
SHAPES = [(1, 2, None),            # smallest
          (3, 29, None),           # scalar path
          (5, 40, None),           # V % 8 == 0 but under one wave of 8-wide lanes
          (7, 512, None),          # one full sweep of 64 lanes x 8 (bf16); M just below 2 workgroups
          (4, 520, None),          # ... and one with a tail
          (9, 1024, None),         # the LM's V; M just above 2 workgroups
          (6, 1032, None),         # ... with a tail
          (2, 4096, None),         # the transducer's V
          (17, 64, None),          # M just above a multiple of ROWS
          (15, 64, None),          # M just below a multiple of ROWS
          (6, 40, (48, 3)),        # ldx > V, base pointer not 16-byte aligned: the scalar path
          (6, 40, (56, 8))]        # ldx > V, everything still aligned: the vector path with ldx != V
SHAPE_IDS = ["%dx%d%s" % (m, v, "" if s is None else "_in%d_at%d" % s) for m, v, s in SHAPES]


@functools.lru_cache(maxsize=None)
def _case(M, V):
    """Logits 3 * normal; row 0 targets V - 1, row 1 has +90 on its target, row 3 targets 0 and has +90 elsewhere, row 4
    is -1e4 everywhere but one entry (not its target), row 6's target is out of range, rows 2, 5, 8, ... are ignored."""
    rng = np.random.default_rng(100 * M + V)
    z = (3.0 * rng.standard_normal((M, V))).astype(np.float32)
    t = rng.integers(0, V, size=M).astype(np.int64)
    t[0] = V - 1
    if M >= 2:
        z[1, t[1]] += 90.0
    if M >= 4:
        t[3] = 0
        z[3, V // 2] += 90.0
    if M >= 5:
        keep = z[4, (t[4] + 1) % V]
        z[4, :] = -1e4
        z[4, (t[4] + 1) % V] = keep
    if M >= 7:
        t[6] = V + 3
    t[2::3] = IGN
    go = (rng.uniform(0.25, 1.0, size=M) * rng.choice([-1.0, 1.0], size=M)).astype(np.float32)
    z.setflags(write=False)
    t.setflags(write=False)
    go.setflags(write=False)
    return z, t, go


def _seen(z, dtype):
    return torch.tensor(z).to(dtype).double().numpy()


@functools.lru_cache(maxsize=None)
def _oracle(M, V, dtype, reduction):
    z, t, go = _case(M, V)
    return R.softmax_nll(_seen(z, dtype), t, IGN, reduction, go if reduction == "none" else 0.7)


def _logits(z, dtype, sl):
    """-> (leaf, logits view, untouched copy of the leaf)"""
    M, V = z.shape
    if sl is None:
        leaf = torch.tensor(z, device="cuda").to(dtype).requires_grad_(True)
        return leaf, leaf, leaf.detach().clone()
    width, at = sl
    buf = torch.full((M, width), 7.0, device="cuda", dtype=dtype)
    buf[:, at:at + V] = torch.tensor(z, device="cuda").to(dtype)
    buf.requires_grad_(True)
    return buf, buf[:, at:at + V], buf.detach().clone()


def _run(M, V, dtype, reduction, sl=None, ignore_index=IGN, targets=None):
    from edgedict_amd.loss import SoftmaxNLLLoss
    z, t, go = _case(M, V)
    if targets is not None:
        t = targets
    leaf, view, before = _logits(z, dtype, sl)
    tt = torch.tensor(t, device="cuda")
    loss = SoftmaxNLLLoss(ignore_index=ignore_index, reduction=reduction)(view, tt)
    out = loss.detach().clone()
    loss.backward(torch.tensor(go, device="cuda") if reduction == "none" else torch.tensor(0.7, device="cuda"))
    return out, leaf, before


def _assert_grad(got, ref, dtype, what):
    err = np.abs(got - ref)
    if dtype == F32:
        assert (err <= 1e-3 * np.abs(ref) + 2e-5).all(), (what, err.max())
    else:
        assert (err <= 4e-3).all(), (what, err.max())
    return err.max()


def _assert_nll(got, ref, dtype):
    np.testing.assert_allclose(got, ref, rtol=1e-5 if dtype == F32 else 1e-4, atol=1e-4 if dtype == F32 else 0.0)
    return np.abs(got - ref).max()


@pytest.mark.parametrize("M,V,sl", SHAPES, ids=SHAPE_IDS)
@DTYPES
def test_loss_and_gradient_against_the_oracle(hip_lib, M, V, sl, dtype):
    """All three reductions under a non-unit incoming gradient: nll / loss and gradient against the oracle, bit-zero nll
    and gradient on ignored rows, the gradient IS the logits buffer (written in place, in its dtype), the columns of a
    wider buffer around the slice untouched, and a second run bit-identical."""
    z, t, go = _case(M, V)
    ok = R.valid_rows(t, V, IGN)
    at = 0 if sl is None else sl[1]
    for reduction in ("none", "sum", "mean"):
        loss, nll, lse, dz = _oracle(M, V, dtype, reduction)
        out, leaf, before = _run(M, V, dtype, reduction, sl)
        g = leaf.grad
        assert g.dtype == dtype and out.dtype == F32 and torch.isfinite(out).all()
        gz = g[:, at:at + V]
        e_l = _assert_nll(out.double().cpu().numpy(), loss, dtype)
        e_g = _assert_grad(gz.double().cpu().numpy(), dz, dtype, reduction)
        print("softmax_nll", (M, V, sl), dtype, reduction, "max loss err %.3g, max grad err %.3g" % (e_l, e_g))
        if reduction == "none":
            assert out.shape == (M,)
            assert (out[torch.tensor(~ok, device="cuda")] == 0).all()          # bit zero: 0.0 == -0.0 is excluded below
            assert not torch.signbit(out[torch.tensor(~ok, device="cuda")]).any()
        else:
            assert out.dim() == 0
        zero_rows = gz[torch.tensor(~ok, device="cuda")]
        assert zero_rows.numel() == 0 or (zero_rows.view(torch.int16 if dtype == BF16 else torch.int32) == 0).all()
        # in place: the logits' storage now holds the gradient, what lies around a slice is as it was
        assert torch.equal(leaf.detach()[:, at:at + V], gz)
        if sl is not None:
            keep = torch.ones(sl[0], dtype=torch.bool, device="cuda")
            keep[at:at + V] = False
            assert torch.equal(leaf.detach()[:, keep], before[:, keep])
            assert (g[:, keep] == 0).all()
        out2, leaf2, _ = _run(M, V, dtype, reduction, sl)
        assert torch.equal(out2, out) and torch.equal(leaf2.grad, g)


@pytest.mark.parametrize("M,V,sl", [SHAPES[1], SHAPES[5], SHAPES[10]], ids=[SHAPE_IDS[1], SHAPE_IDS[5], SHAPE_IDS[10]])
@DTYPES
def test_forward_only_mode_and_lse(hip_lib, M, V, sl, dtype):
    """softmax_nll_rows (scoring): the per-row nll of the oracle, the logits untouched; the forward's lse through the C
    entry point, bit-identical in a second call."""
    from edgedict_amd import _lib
    from edgedict_amd.loss import softmax_nll_rows, _nll_ld
    z, t, _ = _case(M, V)
    _, nll, lse, _ = _oracle(M, V, dtype, "none")
    leaf, view, before = _logits(z, dtype, sl)
    tt = torch.tensor(t, device="cuda").int()
    got = softmax_nll_rows(view, tt, IGN)
    assert torch.equal(leaf.detach(), before)
    e_n = _assert_nll(got.double().cpu().numpy(), nll, dtype)
    got_lse = torch.empty(M, device="cuda")
    got_nll = torch.empty(M, device="cuda")
    v = view.detach()
    _lib.call("softmax_nll_forward", _lib.dtype_code(dtype), v, _nll_ld(v), tt, M, V, IGN, got_lse, got_nll, None, None, 0)
    e_s = _assert_nll(got_lse.double().cpu().numpy(), lse, dtype)
    assert torch.equal(got_nll, got)
    lse2 = torch.empty(M, device="cuda")
    nll2 = torch.empty(M, device="cuda")
    _lib.call("softmax_nll_forward", _lib.dtype_code(dtype), v, _nll_ld(v), tt, M, V, IGN, lse2, nll2, None, None, 0)
    assert torch.equal(lse2, got_lse) and torch.equal(nll2, got_nll)
    print("softmax_nll forward-only", (M, V, sl), dtype, "max nll err %.3g, max lse err %.3g" % (e_n, e_s))


@pytest.mark.parametrize("M,V", [(5, 40), (9, 1024), (3, 29)])
@DTYPES
def test_all_ignored_batch_gives_zero_loss_and_zero_gradient(hip_lib, M, V, dtype):
    """No valid row: every reduction gives 0 (torch's mean gives NaN), the gradient is bit zero, nothing is NaN."""
    targets = np.full(M, IGN, dtype=np.int64)
    targets[M // 2] = V            # out of range counts as ignored
    for reduction in ("none", "sum", "mean"):
        out, leaf, _ = _run(M, V, dtype, reduction, targets=targets)
        assert not torch.isnan(out).any() and not torch.isnan(leaf.grad).any()
        assert (out == 0).all() and not torch.signbit(out).any()
        assert (leaf.grad.view(torch.int16 if dtype == BF16 else torch.int32) == 0).all()
    print("softmax_nll all-ignored", (M, V), dtype, "max |loss| 0, max |grad| 0")


def test_ignore_index_inside_the_vocabulary(hip_lib):
    """ignore_index = 0, the LM's padding: rows with target 0 are ignored, the mean divides by the rest."""
    M, V = 9, 40
    z, t, _ = _case(M, V)
    t = np.where(t == IGN, 0, t)
    out, leaf, _ = _run(M, V, F32, "mean", ignore_index=0, targets=t)
    loss, _, _, dz = R.softmax_nll(z.astype(np.float64), t, 0, "mean", 0.7)
    e_l = _assert_nll(out.double().cpu().numpy(), loss, F32)
    e_g = _assert_grad(leaf.grad.double().cpu().numpy(), dz, F32, "mean")
    assert (leaf.grad[torch.tensor(t == 0, device="cuda")] == 0).all() and (t == 0).sum() >= 3
    print("softmax_nll ignore_index 0: max loss err %.3g, max grad err %.3g" % (e_l, e_g))


def test_second_backward_raises(hip_lib):
    from edgedict_amd.loss import SoftmaxNLLLoss
    z, t, _ = _case(5, 40)
    tz = torch.tensor(z, device="cuda").requires_grad_(True)
    loss = SoftmaxNLLLoss(ignore_index=IGN)(tz, torch.tensor(t, device="cuda"))
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="consumed by a previous backward"):
        loss.backward()


def test_check_targets_on_the_device(hip_lib):
    from edgedict_amd.loss import SoftmaxNLLLoss
    z, t, _ = _case(9, 40)
    tz = torch.tensor(z, device="cuda")
    with pytest.raises(ValueError, match="outside"):       # row 6's target is V + 3
        SoftmaxNLLLoss(ignore_index=IGN, check_targets=True)(tz, torch.tensor(t, device="cuda"))
    assert torch.equal(tz.cpu(), torch.tensor(z))


@pytest.mark.parametrize("M,N", [(3, 29), (5, 1024), (2, 1032)])
@DTYPES
def test_log_softmax_autograd_function(hip_lib, M, N, dtype):
    """lm._LogSoftmaxRowsFn against torch.log_softmax in float64 under a random dy: the output within the existing
    test_log_softmax_rows_kernel atol 1e-5, the gradient (in the logits' dtype) within the gradient bounds above."""
    from edgedict_amd.lm import _LogSoftmaxRowsFn
    rng = np.random.default_rng(7 * M + N)
    x = (3.0 * rng.standard_normal((M, N))).astype(np.float32)
    x[0, 3] += 40.0
    dy = rng.uniform(-1.0, 1.0, size=(M, N)).astype(np.float32) / 8.0
    dy[1] = 0.0
    dy[1, 5] = -0.5            # what NLLLoss sends: one entry per row
    tx = torch.tensor(x, device="cuda").to(dtype).requires_grad_(True)
    y = _LogSoftmaxRowsFn.apply(tx)
    y.backward(torch.tensor(dy, device="cuda"))
    ref = torch.tensor(x).to(dtype).double().requires_grad_(True)
    yr = torch.log_softmax(ref, -1)
    yr.backward(torch.tensor(dy).double())
    assert y.dtype == F32 and tx.grad.dtype == dtype
    e_y = (y.detach().double().cpu() - yr.detach()).abs().max().item()
    assert e_y <= 1e-5, e_y
    np.testing.assert_allclose(R.log_softmax_bwd(yr.detach().numpy(), dy), ref.grad.numpy(), rtol=1e-10, atol=1e-12)
    e_g = _assert_grad(tx.grad.double().cpu().numpy(), ref.grad.numpy(), dtype, "log_softmax bwd")
    print("log_softmax_rows autograd", (M, N), dtype, "max y err %.3g, max grad err %.3g" % (e_y, e_g))


def test_rows_behind_2_to_the_31_elements(hip_lib):
    """M * V > 2^31 (bf16, 4.3 GB): the row offsets are 64-bit.  The first and the last rows against the oracle, the
    fixed-order fp64 sum against a float64 sum of the kernel's own nll."""
    from edgedict_amd.loss import SoftmaxNLLLoss, softmax_nll_rows
    M, V = (1 << 21) + 3, 1024
    assert M * V > 2 ** 31
    g = torch.Generator(device="cuda").manual_seed(5)
    tz = torch.empty(M, V, device="cuda", dtype=BF16).normal_(0.0, 3.0, generator=g)
    tt = torch.randint(0, V, (M,), device="cuda", dtype=torch.int32, generator=g)
    tt[-2] = IGN
    rows = [0, 1, M - 3, M - 2, M - 1]
    seen = tz[rows].double().cpu().numpy()
    tsel = tt[rows].cpu().numpy()
    nll = softmax_nll_rows(tz, tt, IGN)
    _, ref_nll, _, ref_dz = R.softmax_nll(seen, tsel, IGN, "sum", 0.5)
    e_n = _assert_nll(nll[rows].double().cpu().numpy(), ref_nll, BF16)
    tz.requires_grad_(True)
    loss = SoftmaxNLLLoss(ignore_index=IGN, reduction="sum")(tz, tt)
    np.testing.assert_allclose(loss.item(), nll.double().sum().item(), rtol=1e-6)
    loss.backward(torch.tensor(0.5, device="cuda"))
    e_g = _assert_grad(tz.grad[rows].double().cpu().numpy(), ref_dz, BF16, "rows behind 2^31")
    assert (tz.grad[M - 2] == 0).all()
    print("softmax_nll M * V = %d: max nll err %.3g, max grad err %.3g" % (M * V, e_n, e_g))
