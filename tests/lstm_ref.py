"""float64 replay of the LSTM recurrence as csrc/lstm.hip and csrc/lstm_fast.hip split it: the input product is done
(G_in [B,T,4H] holds x W_ih^T + b_ih + b_hh), what remains is the serial part, one step at a time.  Gate order i, f, g, o
in the 4H columns; i, f, o = sigmoid, g = tanh; c' = f c + i g, h' = o tanh(c').

``lstm_steps64`` returns every buffer the step kernels leave - the post-activation gates written over G, Y, the h_{t-1}
image Hprev, the cell states Cst, the final states - and, by autograd of (Y * dY).sum(), the gradient of every step's
pre-activation: what the BPTT writes over G.

``lstm_bwd64`` is the BPTT spelled out by hand on SAVED buffers (gates, Cst), the cell backward of lstm_step_bwd formula
for formula.  On the replay's own buffers it equals the autograd result (tests/test_lstm_ref_host.py); on a kernel's
buffers it says what that kernel's backward should have made of them, which separates a backward error from an
inherited forward one.

Both take ``store``: a dtype the kernels round to where they store - h_t (Y, Hprev and the operand of the next step's
product; h0 too: Hprev's frame 0 is in the compute dtype), the saved gates, dG_t (the operand of step t-1's product).
With it a difference beyond a few ulps of that dtype is no rounding.  Cst, hN and cN stay unrounded, as in the kernels
(the fragment-order forward alone takes hN from the rounded h; see ``hN_stored``).
"""
import collections

import torch

F64 = torch.float64

Replay = collections.namedtuple("Replay", "gates Y Hprev Cst hN cN dG hN_stored")


def _rt(x, store):
    """x rounded to ``store`` (round-to-nearest-even, torch's cast), back in float64."""
    return x if store is None else x.to(store).to(F64)


def lstm_steps64(G_in, w_hh, h0=None, c0=None, dY=None, store=None):
    """G_in [B,T,4H], w_hh [4H,H], h0/c0 [B,H] or None (zeros), dY [B,T,H] or None (no gradient wanted).
    Returns Replay(gates [B,T,4H], Y, Hprev [B,T,H], Cst [B,T,H], hN, cN [B,H], dG [B,T,4H] or None, hN_stored)."""
    B, T, H4 = G_in.shape
    H = H4 // 4
    assert H4 == 4 * H and tuple(w_hh.shape) == (H4, H)
    assert store is None or dY is None, "rounded replay: take the gradients from lstm_bwd64"
    W = w_hh.detach().to(F64)
    G = G_in.detach().to(F64).clone().requires_grad_(dY is not None)
    h = torch.zeros(B, H, dtype=F64) if h0 is None else _rt(h0.detach().to(F64), store)
    c = torch.zeros(B, H, dtype=F64) if c0 is None else c0.detach().to(F64)
    gates, ys, hprev, cs = [], [], [], []
    h_exact = h
    for t in range(T):
        hprev.append(h)
        pre = G[:, t] + h @ W.t()
        i, f, g, o = pre.split(H, dim=1)
        i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
        c = f * c + i * g
        h_exact = o * torch.tanh(c)
        h = _rt(h_exact, store)
        gates.append(_rt(torch.cat([i, f, g, o], 1), store))
        ys.append(h)
        cs.append(c)
    Y = torch.stack(ys, 1)
    dG = None
    if dY is not None:
        (Y * dY.detach().to(F64)).sum().backward()
        dG = G.grad
    st = lambda ts: torch.stack([x.detach() for x in ts], 1)     # noqa: E731
    return Replay(st(gates), Y.detach(), st(hprev), st(cs), h_exact.detach(), c.detach(), dG, h.detach())


def lstm_bwd64(gates, Cst, c0, dY, w_hh, store=None):
    """BPTT over saved buffers: gates [B,T,4H] (post-activation), Cst [B,T,H], c0 [B,H] or None, dY [B,T,H] or None.
    dh_t = dY_t + dG_{t+1} W_hh; dc_t = dc_carry + dh_t o (1 - tanh(c_t)^2); the four pre-activation gradients; the
    carry dc_t f.  Returns dG [B,T,4H]."""
    B, T, H4 = gates.shape
    H = H4 // 4
    W = w_hh.detach().to(F64)
    gates, Cst = gates.detach().to(F64), Cst.detach().to(F64)
    dC = torch.zeros(B, H, dtype=F64)
    out = [None] * T
    nxt = None
    for t in range(T - 1, -1, -1):
        dh = torch.zeros(B, H, dtype=F64) if dY is None else dY[:, t].detach().to(F64)
        if nxt is not None:
            dh = dh + nxt @ W
        i, f, g, o = gates[:, t].split(H, dim=1)
        c = Cst[:, t]
        cprev = Cst[:, t - 1] if t > 0 else (torch.zeros(B, H, dtype=F64) if c0 is None else c0.detach().to(F64))
        tc = torch.tanh(c)
        dct = dC + dh * o * (1 - tc * tc)
        d = torch.cat([dct * g * i * (1 - i), dct * cprev * f * (1 - f), dct * i * (1 - g * g), dh * tc * o * (1 - o)], 1)
        nxt = out[t] = _rt(d, store)
        dC = dct * f
    return torch.stack(out, 1)


def pack_images(w_hh):
    """The two fragment-order bf16 images of W_hh [4H,H] by the formulas in the header of csrc/lstm_fast.hip, as index
    arithmetic: fwd [H/16][4][H/32][64][8] with element (ub, gate, ks, lane, e) = W[gate H + 16 ub + (lane & 15),
    32 ks + 8 (lane >> 4) + e]; bwd [H/16][4H/32][64][8] with (ub, ks, lane, e) = W[32 ks + 8 (lane >> 4) + e,
    16 ub + (lane & 15)].  bf16 by round-to-nearest-even."""
    H4, H = w_hh.shape
    assert H4 == 4 * H and H % 32 == 0
    Wb = w_hh.detach().cpu().to(torch.bfloat16)
    ar = torch.arange
    lane, e = ar(64).view(1, 1, 1, 64, 1), ar(8).view(1, 1, 1, 1, 8)
    ub, gate, ks = ar(H // 16).view(-1, 1, 1, 1, 1), ar(4).view(1, 4, 1, 1, 1), ar(H // 32).view(1, 1, -1, 1, 1)
    fwd = Wb[gate * H + ub * 16 + (lane & 15), ks * 32 + (lane >> 4) * 8 + e]
    ksb = ar(4 * H // 32).view(1, 1, -1, 1, 1)
    bwd = Wb[ksb * 32 + (lane >> 4) * 8 + e, ub * 16 + (lane & 15)][:, 0]
    assert fwd.shape == (H // 16, 4, H // 32, 64, 8) and bwd.shape == (H // 16, 4 * H // 32, 64, 8)
    return fwd.contiguous(), bwd.contiguous()
