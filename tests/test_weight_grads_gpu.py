"""GPU: the weight gradients of the Functions whose backward goes through side.WeightGrads (Linear, the LSTM block, the
dense joint, the packed joint + loss) are the same whether they are returned to autograd (parameters without .grad) or
accumulated in place on the auxiliary stream (zeroed fp32 .grad views of one flat buffer, as FlatParams leaves them).
The in-place run reports its live parameters to the data-parallel exchange exactly once, the returned run not at all;
a frozen parameter's .grad stays zero in both."""
import pytest
import torch

pytestmark = pytest.mark.gpu

F32 = torch.float32


def _case(name):
    """(parameters - None for an absent bias -, a closure running forward and returning a scalar to backpropagate)"""
    from edgedict_amd.models import _JointFn, _JointLossFn, _LinearFn, _LSTMBlockFn
    g = torch.Generator(device="cpu").manual_seed(0)

    def rand(*shape, k=0.5):
        return (k * (torch.rand(*shape, generator=g) * 2 - 1)).cuda()

    def param(*shape, k=0.5):
        return rand(*shape, k=k).requires_grad_(True)

    if name.startswith("linear"):
        ps = [param(16, 24), param(16) if name == "linear" else None]
        x, dy = rand(3, 5, 24).requires_grad_(True), rand(3, 5, 16)
        return ps, lambda: (_LinearFn.apply(x, *ps, F32) * dy).sum()
    if name.startswith("lstm"):
        cd = torch.bfloat16 if name == "lstm_bf16" else F32
        B, T, I, H = 3, 5, 32, 32
        k = H ** -0.5
        ps = [param(4 * H, I, k=k), param(4 * H, H, k=k), param(4 * H, k=k), param(4 * H, k=k)]
        x = rand(B, T, I, k=1.0).to(cd).requires_grad_(True)
        h0, c0, dy = rand(B, H), rand(B, H), rand(B, T, H, k=1.0)

        def run():
            y = _LSTMBlockFn.apply(x, *ps, None, None, h0, c0, False, 1, cd)[0]
            return (y.float() * dy).sum()
        return ps, run
    B, T, U, P, P2, J, V = 2, 6, 3, 24, 16, 32, 40
    ps = [param(J, P + P2), param(J), param(V, J), param(V)]
    enc, dec = rand(B, T, P, k=1.0).requires_grad_(True), rand(B, U + 1, P2, k=1.0).requires_grad_(True)
    if name == "joint":
        dy = rand(B, T, U + 1, V)
        return ps, lambda: (_JointFn.apply(enc, dec, *ps, F32) * dy).sum()
    labels = torch.randint(1, V, (B, U), generator=g, dtype=torch.int32).cuda()
    act, ylen = torch.tensor([T, T - 2], dtype=torch.int32), torch.tensor([U - 1, U], dtype=torch.int32)
    return ps, lambda: _JointLossFn.apply(enc, dec, *ps, labels, act, ylen, 0, F32).sum()


NPARAMS = {"linear": 2, "linear_nobias": 1, "lstm_fp32": 4, "lstm_bf16": 4, "joint": 4, "joint_loss": 4}


@pytest.mark.parametrize("name,frozen", [(n, f) for n, k in NPARAMS.items() for f in [None] + list(range(k))])
def test_returned_and_in_place_weight_gradients_agree(hip_lib, name, frozen):
    from edgedict_amd import dp
    ps, run = _case(name)
    present = [p for p in ps if p is not None]
    if frozen is not None:
        present[frozen].requires_grad_(False)
    live = [p for p in present if p.requires_grad]
    reported = []
    saved, dp.READY_HOOK = dp.READY_HOOK, lambda params, stream: reported.append(sorted(id(p) for p in params))
    try:
        # returned to autograd: the live parameters own no .grad yet, a frozen one a zero buffer that must stay so
        for p in present:
            p.grad = None if p.requires_grad else torch.zeros_like(p)
        run().backward()
        torch.cuda.synchronize()
        assert reported == []
        returned = [p.grad.clone() for p in present]
        # accumulated in place: every parameter owns a zeroed fp32 view of one flat buffer
        flat = torch.zeros(sum(p.numel() for p in present), dtype=F32, device="cuda")
        views, off = [], 0
        for p in present:
            views.append(flat[off:off + p.numel()].view_as(p))
            p.grad = views[-1]
            off += p.numel()
        run().backward()
        torch.cuda.synchronize()
    finally:
        dp.READY_HOOK = saved
    # nothing live (the one parameter of a bias-less Linear frozen): nothing to accumulate, nothing to report
    assert reported == ([sorted(id(p) for p in live)] if live else []), (reported, len(live))
    for i, (p, r, v) in enumerate(zip(present, returned, views)):
        assert p.grad.data_ptr() == v.data_ptr(), i
        if not p.requires_grad:
            assert (r == 0).all() and (p.grad == 0).all(), i
            continue
        # the same products; only the order of fp32 accumulation (split-K, atomics) may differ
        scale = max(r.abs().max().item(), 1e-8)
        assert r.abs().max().item() > 0, i
        assert (p.grad - r).abs().max().item() <= 1e-5 * scale, (i, (p.grad - r).abs().max().item(), scale)
