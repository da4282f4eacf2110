"""CPU: the float64 restatement of the encoder stack (tests/stack_ref.py) is the oracle's encoder
(oracle.models_ref.encoder_forward, pinned to the reference's goldens), its one-layer replay chains to the whole, its
column permutation is the kernels' (ed_gate_col, csrc/stack_kernels.hpp) and its weight-gradient products are
autograd's."""
import pytest
import torch

import lstm_ref as R
import stack_ref as S
from oracle import models_ref as M

F64 = torch.float64

# (B, T0, I0, H, L, reductions, initial states): one layer and three, odd T under a reduction, two reductions in a row
CASES = [
    (3, 5, 8, 16, 1, [1], False),
    (2, 5, 8, 16, 1, [2], True),
    (3, 7, 24, 32, 3, [1, 2, 1], True),
    (2, 7, 16, 16, 3, [2, 2, 1], False),
    (2, 9, 8, 16, 3, [1, 2, 2], True),
]


def _problem(B, T0, I0, H, L, reductions, states, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed + 100 * H + T0)
    k = 1.0 / H ** 0.5
    u = lambda *s: (torch.rand(*s, generator=g, dtype=F64) * 2 - 1) * k            # noqa: E731
    n = lambda *s: torch.randn(*s, generator=g, dtype=F64)                         # noqa: E731
    layers = []
    for l in range(L):
        I = I0 if l == 0 else H
        layers.append((u(4 * H, I), u(4 * H, H), u(4 * H), u(4 * H), 1 + 0.3 * n(H), 0.3 * n(H)))
    in_g, in_b = 1 + 0.3 * n(I0), 0.3 * n(I0)
    x = n(B, T0, I0)
    h0 = 0.5 * n(L, B, H) if states else None
    c0 = 0.5 * n(L, B, H) if states else None
    T = T0
    for r in reductions:
        T = (T + r - 1) // r
    return x, in_g, in_b, layers, h0, c0, n(B, T, H)


def _state_dict(in_g, in_b, layers, H):
    """The reference's key names; the projection is the identity, so encoder_forward returns the stack's raw output."""
    sd = {"encoder.norm.weight": in_g, "encoder.norm.bias": in_b,
          "encoder.proj.weight": torch.eye(H, dtype=F64), "encoder.proj.bias": torch.zeros(H, dtype=F64)}
    for l, lay in enumerate(layers):
        p = "encoder.lstm.lstms.%d." % l
        sd[p + "weight_ih_l0"], sd[p + "weight_hh_l0"], sd[p + "bias_ih_l0"], sd[p + "bias_hh_l0"] = lay[:4]
        sd["encoder.lstm.projs.%d.0.weight" % l], sd["encoder.lstm.projs.%d.0.bias" % l] = lay[4:]
    return sd


def _rel(a, b):
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-300)


@pytest.mark.parametrize("B,T0,I0,H,L,reductions,states", CASES)
def test_stack_forward64_is_the_oracles_encoder(B, T0, I0, H, L, reductions, states):
    x, in_g, in_b, layers, h0, c0, dout = _problem(B, T0, I0, H, L, reductions, states)
    res = S.stack_forward64(x, in_g, in_b, layers, reductions, h0, c0)
    grads = S.stack_grads64(res, dout)

    sd = {k: v.clone().requires_grad_(True) for k, v in _state_dict(in_g, in_b, layers, H).items()}
    xr = x.clone().requires_grad_(True)
    hid = None
    if states:
        hid = (h0.clone().requires_grad_(True), c0.clone().requires_grad_(True))
    # layers listed in time_reductions halve the frame rate (encoder_forward: x = y if i == 0 else x + y, then the norm)
    red = tuple(l for l, r in enumerate(reductions) if r == 2)
    y, (hs, cs) = M.encoder_forward(sd, xr, hid, time_reductions=red, explicit=True)
    (y * dout).sum().backward()

    assert res.out.shape == y.shape
    assert _rel(res.out.detach(), y.detach()) <= 1e-12
    assert _rel(res.hN.detach(), hs.detach()) <= 1e-12 and _rel(res.cN.detach(), cs.detach()) <= 1e-12
    assert _rel(grads["dx"], xr.grad) <= 1e-12
    assert _rel(grads["in_gamma"], sd["encoder.norm.weight"].grad) <= 1e-12
    assert _rel(grads["in_beta"], sd["encoder.norm.bias"].grad) <= 1e-12
    for l in range(L):
        p = "encoder.lstm.lstms.%d." % l
        names = [p + "weight_ih_l0", p + "weight_hh_l0", p + "bias_ih_l0", p + "bias_hh_l0",
                 "encoder.lstm.projs.%d.0.weight" % l, "encoder.lstm.projs.%d.0.bias" % l]
        for got, name in zip(grads["layers"][l], names):
            assert _rel(got, sd[name].grad) <= 1e-12, name
    if states:
        assert _rel(res.leaves["h0"].grad, hid[0].grad) <= 1e-12
        assert _rel(res.leaves["c0"].grad, hid[1].grad) <= 1e-12
    # the frame arithmetic: every reduction rounds up
    T = T0
    for l, r in enumerate(reductions):
        assert res.layers[l].Y.shape == (B, T, H) and res.layers[l].mean.shape == (B, T)
        T = (T + r - 1) // r
        assert res.layers[l].out.shape == (B, T, H)


@pytest.mark.parametrize("B,T0,I0,H,L,reductions,states", CASES)
def test_layer_forward64_chained_reproduces_the_stack_and_the_lstm_replay(B, T0, I0, H, L, reductions, states):
    x, in_g, in_b, layers, h0, c0, dout = _problem(B, T0, I0, H, L, reductions, states)
    res = S.stack_forward64(x, in_g, in_b, layers, reductions, h0, c0)
    grads = S.stack_grads64(res, dout)
    mean, rstd = S.ln_stats(x)
    assert torch.equal(mean, res.in_mean) and torch.equal(rstd, res.in_rstd)
    X = M.layer_norm(x, in_g, in_b)
    assert _rel(X, res.X0.detach()) <= 1e-14
    for l in range(L):
        want = res.layers[l]
        got = S.layer_forward64(X, layers[l], reductions[l], l > 0, h0[l] if states else None, c0[l] if states else None)
        for name in ("X", "G_in", "gates", "Y", "Hprev", "C", "Z", "mean", "rstd", "out", "hN", "cN"):
            a, b = getattr(got, name), getattr(want, name).detach()
            assert a.shape == b.shape, name
            assert _rel(a, b) <= 1e-13, (l, name)
        # the statistics are those of Z, and Z's LayerNorm (+ pair mean with zeros behind a lone frame) is the output
        zn = (got.Z - got.mean[..., None]) * got.rstd[..., None] * layers[l][4] + layers[l][5]
        if reductions[l] == 2:
            if zn.shape[1] % 2:
                zn = torch.cat([zn, torch.zeros(B, 1, H, dtype=F64)], 1)
            zn = 0.5 * (zn[:, 0::2] + zn[:, 1::2])
        assert _rel(zn, got.out) <= 1e-13
        # the differentiable recurrence of stack_forward64 is lstm_ref's loop
        rep = R.lstm_steps64(got.G_in, layers[l][1], h0[l] if states else None, c0[l] if states else None)
        assert _rel(rep.gates, want.gates.detach()) <= 1e-13
        X = got.out
    assert _rel(X, res.out.detach()) <= 1e-13
    assert all(g.shape == rec.gates.shape for g, rec in zip(grads["dG"], res.layers))


@pytest.mark.parametrize("H", [16, 32, 96, 1024])
def test_gate_cols_inverts_ed_gate_col(H):
    """``row_of`` is the formula tests/test_encoder_stack_gpu.py::test_weight_images_match_their_documented_layouts
    checks the packed W_ih image against: the W row (= plain gate column) of interleaved column kap."""
    perm = S.gate_cols(H)
    assert sorted(perm.tolist()) == list(range(4 * H))
    kap = torch.arange(4 * H)
    row_of = ((kap >> 4) & 3) * H + (kap >> 6) * 16 + (kap & 15)
    assert torch.equal(row_of[perm], kap)                       # plain -> interleaved -> plain
    assert torch.equal(perm[row_of], kap)
    assert torch.equal(perm.argsort(), row_of)
    for gate in range(4):                                        # ed_gate_col spelled out
        for j in (0, 1, 15, H // 2, H - 1):
            assert perm[gate * H + j].item() == (j >> 4) * 64 + gate * 16 + (j & 15)
    g = torch.Generator(device="cpu").manual_seed(H)
    plain = torch.randn(3, 2, 4 * H, generator=g)                # [B, T, 4H]
    inter = S.interleaved_gates(plain, H)                        # [T, B, 4H]
    assert inter.shape == (2, 3, 4 * H)
    assert torch.equal(inter[1, 2, kap], plain[2, 1, row_of])
    assert torch.equal(S.plain_gates(inter, H), plain)
    assert torch.equal(S.batch_first(inter)[2, 1], inter[1, 2])


@pytest.mark.parametrize("B,T0,I0,H,L,reductions,states", CASES[2:])
def test_weight_grads_from_buffers_are_autograds(B, T0, I0, H, L, reductions, states):
    x, in_g, in_b, layers, h0, c0, dout = _problem(B, T0, I0, H, L, reductions, states)
    res = S.stack_forward64(x, in_g, in_b, layers, reductions, h0, c0)
    grads = S.stack_grads64(res, dout)
    for l, rec in enumerate(res.layers):
        (dw_ih, dw_hh, db), (m_ih, m_hh, m_b) = S.weight_grads_from_buffers(grads["dG"][l], rec.X, rec.Hprev)
        want = grads["layers"][l]
        assert _rel(dw_ih, want[0]) <= 1e-12 and _rel(dw_hh, want[1]) <= 1e-12
        assert _rel(db, want[2]) <= 1e-12 and _rel(db, want[3]) <= 1e-12
        assert (dw_ih.abs() <= m_ih * (1 + 1e-12)).all() and (dw_hh.abs() <= m_hh * (1 + 1e-12)).all()
        assert (db.abs() <= m_b * (1 + 1e-12)).all()
        assert m_ih.shape == (4 * H, rec.X.shape[-1]) and m_hh.shape == (4 * H, H) and m_b.shape == (4 * H,)
