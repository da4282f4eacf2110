"""CPU: pins tests/lstm_ref.py - the float64 step-by-step replay of the LSTM recurrence - before test_lstm_gpu.py judges
the kernels by it.

1. On G_in = x W_ih^T + b_ih + b_hh it reproduces oracle.models_ref.lstm_layer(explicit=True) + autograd in float64:
   outputs, final states, and - through dG, the gradient of every step's pre-activation - dx, dW_ih, dW_hh and the bias
   gradient, to 1e-12.  Without an initial state, and with a single step.
2. The saved buffers are consistent with each other (Hprev is Y shifted by one frame behind h0, Cst follows from the
   gates) and the hand-written BPTT over them equals the autograd dG.
3. With ``store`` every stored value is representable in that dtype and stays within its rounding of the exact replay.
4. The weight images' index arithmetic, element by element at hand-picked places.
"""
import pytest
import torch

import lstm_ref as R
from oracle import models_ref as M

F64 = torch.float64


def _rel(got, ref):
    return (got - ref).abs().max().item() / max(ref.abs().max().item(), 1e-3)


def _problem(B, T, I, H, state, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    k = 1.0 / H ** 0.5
    mk = lambda *s: ((torch.rand(*s, generator=g, dtype=F64) * 2 - 1) * k)     # noqa: E731
    w_ih, w_hh, b_ih, b_hh = mk(4 * H, I), mk(4 * H, H), mk(4 * H), mk(4 * H)
    x = torch.randn(B, T, I, generator=g, dtype=F64)
    h0 = 0.5 * torch.randn(B, H, generator=g, dtype=F64) if state else None
    c0 = 0.5 * torch.randn(B, H, generator=g, dtype=F64) if state else None
    dY = torch.randn(B, T, H, generator=g, dtype=F64)
    return x, (w_ih, w_hh, b_ih, b_hh), h0, c0, dY


# (B, T, I, H, initial state): no state over several steps; one step with a state; the plain case
SHAPES = [(5, 7, 12, 24, False), (3, 1, 10, 8, True), (4, 6, 16, 40, True)]


@pytest.mark.parametrize("B,T,I,H,state", SHAPES)
def test_replay_matches_the_oracle_layer_and_its_autograd(B, T, I, H, state):
    x, params, h0, c0, dY = _problem(B, T, I, H, state, seed=B * 100 + T)
    x = x.requires_grad_(True)
    w_ih, w_hh, b_ih, b_hh = [p.requires_grad_(True) for p in params]
    y, hN, cN = M.lstm_layer(x, w_ih, w_hh, b_ih, b_hh, h0, c0, explicit=True)
    (y * dY).sum().backward()

    G_in = (x.detach() @ w_ih.detach().t() + b_ih.detach() + b_hh.detach())
    r = R.lstm_steps64(G_in, w_hh.detach(), h0, c0, dY)
    assert r.gates.shape == (B, T, 4 * H) and r.dG.shape == (B, T, 4 * H)
    assert r.Y.shape == r.Hprev.shape == r.Cst.shape == (B, T, H) and r.hN.shape == r.cN.shape == (B, H)
    tol = 1e-12
    assert _rel(r.Y, y.detach()) <= tol
    assert _rel(r.hN, hN.detach()) <= tol and _rel(r.cN, cN.detach()) <= tol
    assert torch.equal(r.hN, r.hN_stored)
    dG = r.dG.reshape(B * T, 4 * H)
    assert _rel((dG @ w_ih.detach()).view(B, T, I), x.grad) <= tol
    assert _rel(dG.t() @ x.detach().reshape(B * T, I), w_ih.grad) <= tol
    assert _rel(dG.t() @ r.Hprev.reshape(B * T, H), w_hh.grad) <= tol
    assert _rel(dG.sum(0), b_ih.grad) <= tol and _rel(dG.sum(0), b_hh.grad) <= tol


@pytest.mark.parametrize("B,T,I,H,state", SHAPES)
def test_saved_buffers_are_consistent_and_the_hand_written_bptt_equals_autograd(B, T, I, H, state):
    x, (w_ih, w_hh, b_ih, b_hh), h0, c0, dY = _problem(B, T, I, H, state, seed=B + T)
    G_in = x @ w_ih.t() + b_ih + b_hh
    r = R.lstm_steps64(G_in, w_hh, h0, c0, dY)
    z = torch.zeros(B, H, dtype=F64)
    assert torch.equal(r.Hprev[:, 0], z if h0 is None else h0)
    assert torch.equal(r.Hprev[:, 1:], r.Y[:, :-1])
    assert torch.equal(r.Y[:, -1], r.hN) and torch.equal(r.Cst[:, -1], r.cN)
    i, f, g, o = r.gates.split(H, dim=2)
    cprev = torch.cat([(z if c0 is None else c0)[:, None], r.Cst[:, :-1]], 1)
    assert _rel(f * cprev + i * g, r.Cst) <= 1e-15
    assert _rel(o * torch.tanh(r.Cst), r.Y) <= 1e-15
    assert (i > 0).all() and (i < 1).all() and (g.abs() < 1).all()
    # pre-activations back from the gates: G_in + h_{t-1} W_hh^T
    pre_i = torch.log(i / (1 - i))
    assert _rel(pre_i, G_in[:, :, :H] + r.Hprev @ w_hh[:H].t()) <= 1e-10
    assert _rel(R.lstm_bwd64(r.gates, r.Cst, c0, dY, w_hh), r.dG) <= 1e-12
    # no dY: nothing to propagate
    assert R.lstm_steps64(G_in, w_hh, h0, c0).dG is None
    assert torch.equal(R.lstm_bwd64(r.gates, r.Cst, c0, None, w_hh), torch.zeros(B, T, 4 * H, dtype=F64))


def test_store_rounds_where_the_kernels_store_and_nowhere_else():
    BF16 = torch.bfloat16
    B, T, I, H = 4, 6, 16, 40
    x, (w_ih, w_hh, b_ih, b_hh), h0, c0, dY = _problem(B, T, I, H, True, seed=9)
    G_in = (x @ w_ih.t() + b_ih + b_hh).to(BF16)
    w = w_hh.to(BF16)
    exact = R.lstm_steps64(G_in, w, h0, c0, dY)
    r = R.lstm_steps64(G_in, w, h0, c0, store=BF16)
    for t in (r.gates, r.Y, r.Hprev, r.hN_stored):
        assert torch.equal(t, t.to(BF16).to(F64))
    assert not torch.equal(r.Cst, r.Cst.to(BF16).to(F64)) and not torch.equal(r.hN, r.hN_stored)
    assert torch.equal(r.Hprev[:, 0], h0.to(BF16).to(F64))
    # T steps of 2^-9 relative roundings on values below 1
    for a, b in zip(r[:6], exact[:6]):
        assert (a - b).abs().max().item() <= T * 2.0 ** -8
    with pytest.raises(AssertionError):
        R.lstm_steps64(G_in, w, h0, c0, dY, store=BF16)
    d = R.lstm_bwd64(r.gates, r.Cst, c0, dY, w, store=BF16)
    assert torch.equal(d, d.to(BF16).to(F64))
    assert _rel(d, exact.dG) <= T * 2.0 ** -6


def test_pack_images_by_hand():
    H = 64
    W = torch.arange(4 * H * H, dtype=torch.float32).view(4 * H, H) % 251       # integers below 256: exact in bf16
    fwd, bwd = R.pack_images(W)
    assert fwd.dtype == bwd.dtype == torch.bfloat16
    assert fwd.shape == (4, 4, 2, 64, 8) and bwd.shape == (4, 8, 64, 8)
    # fwd (ub 2, gate 3, ks 1, lane 37 = row 5 of the tile, k quarter 2, e 6): W row 3H + 32 + 5, column 32 + 16 + 6
    assert fwd[2, 3, 1, 37, 6].item() == W[3 * H + 37, 54].item()
    assert fwd[0, 0, 0, 0, 0].item() == W[0, 0].item() and fwd[3, 3, 1, 63, 7].item() == W[4 * H - 1, H - 1].item()
    # bwd (ub 1, ks 5, lane 50 = unit 2 of the tile, k quarter 3, e 1): W row 160 + 24 + 1, column 16 + 2
    assert bwd[1, 5, 50, 1].item() == W[185, 18].item()
    assert bwd[3, 7, 63, 7].item() == W[4 * H - 1, H - 1].item()
    # both are permutations of W
    key = lambda t: torch.sort(t.float().flatten()).values                      # noqa: E731
    assert torch.equal(key(fwd), key(W)) and torch.equal(key(bwd), key(W))
    # rounding is to nearest even: 1 + 2^-8 is a tie between 1 and 1 + 2^-7 and goes to the even mantissa
    W2 = torch.full((128, 32), 1.0 + 2.0 ** -8)
    W2[0, 0] = 1.0 + 3 * 2.0 ** -8                                              # tie between 1 + 2^-7 and 1 + 2^-6
    f2, _ = R.pack_images(W2)
    assert f2[0, 0, 0, 1, 0].item() == 1.0 and f2[0, 0, 0, 0, 0].item() == 1.0 + 2.0 ** -6
