"""GPU: the GRU recurrence kernels (csrc/gru.hip) and the autograd Function around them (_GRUBlockFn: input GEMM,
T step kernels, fused residual + LayerNorm + TimeReduction epilogue, BPTT, weight-gradient GEMMs and column sums)
against a float64 restatement (oracle.models_ref.gru_layer + autograd), in fp32 and bf16, at the shapes where the
kernels' tails live: batches past one 64-row forward tile and one 16-row backward tile, hidden sizes that leave a
partial 32-wide bf16 K fragment (40) and a partial 16-unit backward tile, a single step, with and without h0."""
import pytest
import torch

from oracle import models_ref as M

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16


def _close(got, ref, tol, what=""):
    """max |got - ref| <= tol * max |ref| (the test_lstm_gpu._close criterion, here in float64)."""
    ref = ref.detach().double().cpu()
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    assert torch.isfinite(got).all(), what
    err = (got - ref).abs().max().item()
    scale = max(ref.abs().max().item(), 1e-3)
    assert err <= tol * scale, (what, err, scale, tol)


# fp32: the recurrence's bound; bf16: test_lstm_gpu's bounds (h and the gates are stored in bf16 at every step)
OUT_TOL = {F32: 1e-4, BF16: 2e-2}
GRAD_TOL = {F32: 1e-4, BF16: 4e-2}


def _params(I, H, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    k = 1.0 / H ** 0.5
    w_ih = (torch.rand(3 * H, I, generator=g) * 2 - 1) * k
    w_hh = (torch.rand(3 * H, H, generator=g) * 2 - 1) * k
    b_ih = (torch.rand(3 * H, generator=g) * 2 - 1) * k
    b_hh = (torch.rand(3 * H, generator=g) * 2 - 1) * k
    ln_w = 1.0 + 0.2 * torch.randn(H, generator=g)
    ln_b = 0.2 * torch.randn(H, generator=g)
    return g, (w_ih, w_hh, b_ih, b_hh), (ln_w, ln_b)


# (H, B, T, I, with_h0, ln, residual, reduce): what ResLayerNormGRU passes - layer 0 (LN, no residual, I != H),
# layers > 0 (LN + residual, I == H), the reduction layer (reduce 2, odd T ends on a lone frame) - and the bare
# recurrence (no LN)
CASES = [(8, 3, 17, 12, True, False, False, 1),
         (40, 17, 17, 40, False, True, True, 2),
         (40, 130, 1, 24, True, True, False, 2),
         (64, 65, 17, 64, True, True, True, 2),
         (256, 130, 2, 96, False, True, False, 1),
         (1024, 17, 2, 256, True, False, False, 1),
         (256, 1, 17, 256, True, True, True, 1)]


@pytest.mark.parametrize("cd", [F32, BF16])
@pytest.mark.parametrize("H,B,T,I,with_h0,ln,residual,reduce", CASES)
def test_gru_block_matches_fp64(hip_lib, cd, H, B, T, I, with_h0, ln, residual, reduce):
    from edgedict_amd.models import _GRUBlockFn
    g, (w_ih, w_hh, b_ih, b_hh), (ln_w, ln_b) = _params(I, H, seed=H * 7 + B + T)
    x = torch.randn(B, T, I, generator=g).to(cd)
    h0 = 0.5 * torch.randn(B, H, generator=g) if with_h0 else None
    Tout = (T + reduce - 1) // reduce if ln else T
    dout = torch.randn(B, Tout, H, generator=g).to(cd)
    # float64 on the operands the kernels see: x and the weight matrices rounded to the compute dtype, fp32 biases
    x64 = x.double().requires_grad_(True)
    W = [w.to(cd).double().requires_grad_(True) for w in (w_ih, w_hh)]
    Bs = [b.double().requires_grad_(True) for b in (b_ih, b_hh)]
    L = [p.double().requires_grad_(True) for p in (ln_w, ln_b)]
    y64, h64 = M.gru_layer(x64, W[0], W[1], Bs[0], Bs[1], h0.double() if with_h0 else None)
    out64 = y64
    if ln:
        out64 = M.layer_norm(y64 + x64 if residual else y64, L[0], L[1])
        if reduce == 2:
            out64 = M.time_reduction(out64, 2)
    out64.backward(dout.double())

    dev = [t.cuda().requires_grad_(True) for t in (w_ih, w_hh, b_ih, b_hh, ln_w, ln_b)]
    xin = x.cuda().requires_grad_(True)
    out, hN = _GRUBlockFn.apply(xin, *dev[:4], dev[4] if ln else None, dev[5] if ln else None,
                                h0.cuda() if with_h0 else None, residual, reduce, cd)
    out.backward(dout.cuda())
    assert out.dtype == cd and hN.dtype == F32 and xin.grad.dtype == cd
    ot, gt = OUT_TOL[cd], GRAD_TOL[cd]
    _close(out, out64, ot, "out")
    _close(hN, h64, ot, "hN")
    _close(xin.grad, x64.grad, gt, "dx")
    for name, p, r in zip(("dw_ih", "dw_hh", "db_ih", "db_hh"), dev[:4], W + Bs):
        _close(p.grad, r.grad, gt, name)
    if ln:
        _close(dev[4].grad, L[0].grad, gt, "dln_w")
        _close(dev[5].grad, L[1].grad, gt, "dln_b")
    else:
        assert dev[4].grad is None and dev[5].grad is None
    # tails on their own: the last partial 64-row forward tile / 16-row backward tile, the last partial 16-unit
    # backward tile (its rows of dW_hh, one per gate), the lone last frame of the time reduction
    for tile in (64, 16):
        r0 = B - (B % tile or tile)
        _close(out[r0:], out64[r0:], ot, "out rows %d:" % r0)
        _close(hN[r0:], h64[r0:], ot, "hN rows %d:" % r0)
        _close(xin.grad[r0:], x64.grad[r0:], gt, "dx rows %d:" % r0)
    j0 = H - (H % 16 or 16)
    rows = torch.cat([torch.arange(gate * H + j0, gate * H + H) for gate in range(3)])
    _close(dev[1].grad[rows.cuda()], W[1].grad[rows], gt, "dw_hh last unit tile")
    _close(dev[3].grad[rows.cuda()], Bs[1].grad[rows], gt, "db_hh last unit tile")
    if ln and reduce == 2 and T % 2 == 1:
        _close(out[:, -1], out64[:, -1], ot, "out last frame")


def _ref_steps(G_in, w_hh, b_hh, h0, dY):
    """float64 recurrence on the input pre-activations G_in [B,T,3H] (leaf) with every hidden pre-activation
    gh_t = h_{t-1} W_hh^T + b_hh kept: returns (Y, Hprev, HN, hN, (r, z, n), dG_in, dGH) with dGH the gradients of
    the gh_t, the kernels' DH."""
    B, T, H3 = G_in.shape
    H = H3 // 3
    G_in = G_in.double().requires_grad_(True)
    h = torch.zeros(B, H, dtype=torch.float64) if h0 is None else h0.double()
    ys, hprev, hns, gates, ghs = [], [], [], [], []
    for t in range(T):
        hprev.append(h)
        gh = h @ w_hh.double().t() + b_hh.double()
        if gh.requires_grad:
            gh.retain_grad()
        else:                                           # the first step: a leaf of its own
            gh.requires_grad_(True)
        ghs.append(gh)
        ir, iz, inn = G_in[:, t].split(H, 1)
        hr, hz, hn = gh.split(H, 1)
        r = torch.sigmoid(ir + hr)
        z = torch.sigmoid(iz + hz)
        n = torch.tanh(inn + r * hn)
        h = (1 - z) * n + z * h
        ys.append(h)
        hns.append(hn)
        gates.append(torch.cat([r, z, n], 1))
    Y = torch.stack(ys, 1)
    (Y * dY.double()).sum().backward()
    st = lambda ts: torch.stack([t.detach() for t in ts], 1)     # noqa: E731
    return (Y.detach(), st(hprev), st(hns), h.detach(), st(gates), G_in.grad,
            torch.stack([gh.grad for gh in ghs], 1))


@pytest.mark.parametrize("with_h0", [True, False])
def test_gru_step_kernels_match_fp64(hip_lib, with_h0):
    """ops.gru_forward / ops.gru_backward directly, fp32: every buffer the step kernels leave - the gates written
    over G, h_{t-1}, W_hn h + b_hn, Y, the final state - and, from the BPTT, the input-side pre-activation gradients
    written over G and the hidden-side ones (DH)."""
    from edgedict_amd import ops
    B, T, H = 65, 9, 40
    g = torch.Generator(device="cpu").manual_seed(17 + with_h0)
    k = 1.0 / H ** 0.5
    w_hh = (torch.rand(3 * H, H, generator=g) * 2 - 1) * k
    b_hh = (torch.rand(3 * H, generator=g) * 2 - 1) * k
    G_in = torch.randn(B, T, 3 * H, generator=g)
    h0 = 0.5 * torch.randn(B, H, generator=g) if with_h0 else None
    dY = torch.randn(B, T, H, generator=g)
    Y64, Hp64, HN64, hN64, gates64, dG64, dGH64 = _ref_steps(G_in, w_hh, b_hh, h0, dY)
    G = G_in.cuda()
    Y, Hprev, HN, hN = ops.gru_forward(G, w_hh.cuda(), b_hh.cuda(), h0.cuda() if with_h0 else None)
    tol = 1e-4                                          # fp32 recurrence
    for name, a, b in (("Y", Y, Y64), ("Hprev", Hprev, Hp64), ("HN", HN, HN64), ("hN", hN, hN64),
                       ("gates", G, gates64)):
        _close(a, b, tol, name)
    DH = ops.gru_backward(G, dY.cuda(), Hprev, HN, w_hh.t().contiguous().cuda())
    _close(G, dG64, tol, "dG (input side)")
    _close(DH, dGH64, tol, "DH (hidden side)")
    # the first step's gradients are the end of the BPTT chain; the last batch row is alone in its forward tile
    _close(G[:, 0], dG64[:, 0], tol, "dG first step")
    _close(DH[64:], dGH64[64:], tol, "DH last row tile")
