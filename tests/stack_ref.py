"""float64 restatement of the bf16 encoder stack (csrc/encoder_stack.hip, csrc/stack_kernels.hip): input LayerNorm, then
per layer the input product plus both biases, the LSTM recurrence, the residual for l > 0, the LayerNorm and - where
``reductions[l] == 2`` - the mean of frame pairs (a lone last frame is averaged with zeros).  Plain torch on the CPU, no
rounding anywhere, built from ``oracle.models_ref.layer_norm`` / ``time_reduction`` and ``tests/lstm_ref.lstm_steps64``.

Everything here is batch-first ([B, T, ...]) with the gates in plain order (column ``gate * H + j``, gates i, f, g, o).
The kernels keep their buffers time-major with the gate columns interleaved (``ed_gate_col`` in
csrc/stack_kernels.hpp); ``gate_cols`` / ``plain_gates`` translate.

``stack_forward64`` is the whole stack with every operand a leaf, so ``stack_grads64`` gets every parameter gradient and
every layer's pre-activation gradient dG_l from autograd.  ``layer_forward64`` is the same arithmetic for ONE layer fed a
given input (the forward buffers through ``lstm_ref.lstm_steps64``): on a kernel's own stored X_l it says what that layer
should have made of it, whatever happened below.  ``weight_grads_from_buffers`` are the three weight-gradient products
of a layer from given dG, X and h_{t-1} buffers, with the magnitude sums an fp32 error bound needs.

Dropout (``drop=``, default None: none): mask * scale behind every layer's norm role, the mask restated by
tests/dropout_ref.py over the layer's REDUCED batch-first output, element index (b T_out + tau) H + j.
"""
import collections

import numpy as np
import torch

import dropout_ref as D
import lstm_ref as R
from oracle import models_ref as M

F64 = torch.float64
EPS = 1e-5

Layer64 = collections.namedtuple("Layer64", "X G_in gates Y Hprev C Z mean rstd out hN cN")
Stack64 = collections.namedtuple("Stack64", "out hN cN X0 in_mean in_rstd layers leaves")


def gate_cols(H):
    """perm [4H] with perm[gate * H + j] = ed_gate_col(gate, j) = (j >> 4) * 64 + gate * 16 + (j & 15): 64-column groups
    of 16 units x (i, f, g, o).  ``interleaved[..., perm]`` is the plain order, ``plain[..., perm.argsort()]`` the
    interleaved one."""
    assert H % 16 == 0
    j = torch.arange(H)
    return torch.cat([(j >> 4) * 64 + gate * 16 + (j & 15) for gate in range(4)])


def plain_gates(G_tb, H):
    """A kernel's G buffer [T, B, 4H] (interleaved columns, time-major) as [B, T, 4H] in plain gate order."""
    assert G_tb.shape[-1] == 4 * H
    return G_tb[..., gate_cols(H)].transpose(0, 1).contiguous()


def interleaved_gates(G_bt, H):
    """The inverse of ``plain_gates``: [B, T, 4H] plain -> [T, B, 4H] interleaved."""
    return G_bt[..., gate_cols(H).argsort()].transpose(0, 1).contiguous()


def batch_first(t_tb):
    """A time-major buffer [T, B, ...] as [B, T, ...]."""
    return t_tb.transpose(0, 1).contiguous()


def ln_stats(z, eps=EPS):
    """mean and 1 / sqrt(var + eps) over the last dimension (biased variance, as LayerNorm)."""
    mean = z.mean(-1)
    var = ((z - mean[..., None]) ** 2).mean(-1)
    return mean, 1.0 / torch.sqrt(var + eps)


def drop_mask64(shape, p, seed, frame_shift=0):
    """mask * scale of a layer's batch-first [B, T_out, H] output as float64: element (b, tau, j) has index
    (b T_out + tau) H + j (tests/dropout_ref.py restates the hash; the scale is the kernels' float32 1 / (1 - p)).
    ``frame_shift``: a deliberately WRONG mask for negative controls - the index of frame tau + frame_shift."""
    B, T, H = shape
    keep = D.mask((B, T, H), p, seed, first=frame_shift * H)
    return torch.from_numpy(keep.astype(np.float64) * float(D.scale(p)))


def layer_drop(drop, l):
    """``drop`` = (p, seeds) or (p, seeds, frame_shifts), one seed (and shift) per layer -> layer l's (p, seed, shift)."""
    if drop is None:
        return None
    return (drop[0], drop[1][l], drop[2][l] if len(drop) > 2 else 0)


def norm_role(Z, gamma, beta, reduce, drop=None):
    """LayerNorm of every frame of Z [B, T, H], then the pair mean where reduce == 2; with ``drop`` = (p, seed) or
    (p, seed, frame_shift) of THIS layer, times mask * scale over the REDUCED output.  The kernel rounds the LayerNorm
    (+ pair mean) to bf16 BEFORE it masks and scales (the reference's Dropout sees a bf16 tensor) and rounds the product
    again at its store; float64 rounds nowhere, so a kept element of the kernel is within two bf16 roundings of this
    value and a dropped one is exactly 0."""
    out = M.layer_norm(Z, gamma, beta, EPS)
    out = M.time_reduction(out, 2) if reduce == 2 else out
    if drop is not None:
        out = out * drop_mask64(out.shape, *drop)
    return out


def _recurrence(G_in, w_hh, h, c):
    """The serial part, differentiable: lstm_ref.lstm_steps64's loop with the graph kept."""
    B, T, H4 = G_in.shape
    H = H4 // 4
    gates, ys, hprev, cs = [], [], [], []
    for t in range(T):
        hprev.append(h)
        pre = G_in[:, t] + h @ w_hh.t()
        i, f, g, o = pre.split(H, dim=1)
        i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
        c = f * c + i * g
        h = o * torch.tanh(c)
        gates.append(torch.cat([i, f, g, o], 1))
        ys.append(h)
        cs.append(c)
    return torch.stack(gates, 1), torch.stack(ys, 1), torch.stack(hprev, 1), torch.stack(cs, 1), h, c


def _leaf(t):
    return t.detach().to(F64).cpu().clone().requires_grad_(True)


def stack_forward64(x, in_gamma, in_beta, layers, reductions, h0=None, c0=None, drop=None):
    """x [B, T0, I0]; layers: per layer (w_ih, w_hh, b_ih, b_hh, ln_gamma, ln_beta); reductions: 1 or 2 per layer; h0 / c0
    [L, B, H] or None (zeros); ``drop`` = (p, seeds) - one seed per layer, as EncoderStackFn takes them - puts
    mask * scale behind every layer's norm role (``norm_role``), and a third item, per-layer frame shifts, makes the mask
    deliberately wrong.  Returns Stack64: out [B, T', H], hN / cN [L, B, H], X0, the input norm's statistics
    [B, T0], per layer a Layer64 (X the normalised input, G_in the pre-activations' input part - the leaf of dG -, the
    gates, Y, h_{t-1}, the cell states, Z = Y (+ X) with its statistics [B, T], the layer's output) and ``leaves``:
    x, in_gamma, in_beta, h0, c0 and the per-layer parameter lists as float64 leaves of the graph."""
    L = len(layers)
    assert len(reductions) == L and all(r in (1, 2) for r in reductions)
    lv = dict(x=_leaf(x), in_gamma=_leaf(in_gamma), in_beta=_leaf(in_beta),
              h0=None if h0 is None else _leaf(h0), c0=None if c0 is None else _leaf(c0),
              layers=[[_leaf(p) for p in lay] for lay in layers])
    B = x.shape[0]
    H = layers[0][1].shape[1]
    in_mean, in_rstd = ln_stats(lv["x"].detach())
    X = X0 = M.layer_norm(lv["x"], lv["in_gamma"], lv["in_beta"], EPS)
    recs, hs, cs = [], [], []
    for l, (w_ih, w_hh, b_ih, b_hh, ln_g, ln_b) in enumerate(lv["layers"]):
        G_in = X @ w_ih.t() + b_ih + b_hh
        G_in.retain_grad()
        h = torch.zeros(B, H, dtype=F64) if lv["h0"] is None else lv["h0"][l]
        c = torch.zeros(B, H, dtype=F64) if lv["c0"] is None else lv["c0"][l]
        gates, Y, Hprev, C, hN, cN = _recurrence(G_in, w_hh, h, c)
        Z = Y if l == 0 else X + Y
        mean, rstd = ln_stats(Z.detach())
        out = norm_role(Z, ln_g, ln_b, reductions[l], layer_drop(drop, l))
        recs.append(Layer64(X, G_in, gates, Y, Hprev, C, Z, mean, rstd, out, hN, cN))
        hs.append(hN)
        cs.append(cN)
        X = out
    return Stack64(X, torch.stack(hs), torch.stack(cs), X0, in_mean, in_rstd, recs, lv)


def stack_grads64(res, dout, drop=None):
    """Autograd of (out * dout).sum() through a ``stack_forward64`` result (once per result; ``drop`` is the one the
    result was built with - its masks are part of the graph, so nothing is left to apply here).  Returns a dict: ``dx``,
    ``in_gamma``, ``in_beta``, ``layers`` (per layer [dW_ih, dW_hh, db_ih, db_hh, dln_gamma, dln_beta]) and ``dG`` (per
    layer [B, T, 4H], the gradient of every step's pre-activation, plain gate order)."""
    (res.out * dout.detach().to(F64).cpu()).sum().backward()
    lv = res.leaves
    return dict(dx=lv["x"].grad, in_gamma=lv["in_gamma"].grad, in_beta=lv["in_beta"].grad,
                layers=[[p.grad for p in lay] for lay in lv["layers"]],
                dG=[rec.G_in.grad for rec in res.layers])


def layer_forward64(X, layer, reduce, residual, h0=None, c0=None, drop=None):
    """One layer on a given input X [B, T, I]: (w_ih, w_hh, b_ih, b_hh, ln_gamma, ln_beta), h0 / c0 [B, H] or None;
    ``drop`` = this layer's (p, seed), as ``norm_role`` takes it (only ``out`` depends on it).
    No gradient.  Returns a Layer64 (G_in: the input product plus both biases)."""
    w_ih, w_hh, b_ih, b_hh, ln_g, ln_b = [p.detach().to(F64).cpu() for p in layer]
    X = X.detach().to(F64).cpu()
    G_in = X @ w_ih.t() + b_ih + b_hh
    r = R.lstm_steps64(G_in, w_hh, h0, c0)
    Z = X + r.Y if residual else r.Y
    mean, rstd = ln_stats(Z)
    return Layer64(X, G_in, r.gates, r.Y, r.Hprev, r.Cst, Z, mean, rstd, norm_role(Z, ln_g, ln_b, reduce, drop), r.hN,
                   r.cN)


def weight_grads_from_buffers(dG, X, Hprev):
    """dG [B, T, 4H] (plain gate order), X [B, T, I], Hprev [B, T, H] -> ((dW_ih, dW_hh, db), (|dG|^T |X|, |dG|^T |Hprev|,
    column sums of |dG|)), all float64: the products the side stream makes of a layer's buffers, and the sums of the
    magnitudes of their terms (the scale of an fp32 summation error, whatever the order of the sum)."""
    B, T, H4 = dG.shape
    d = dG.detach().to(F64).cpu().reshape(B * T, H4)
    x = X.detach().to(F64).cpu().reshape(B * T, -1)
    h = Hprev.detach().to(F64).cpu().reshape(B * T, -1)
    return ((d.t() @ x, d.t() @ h, d.sum(0)),
            (d.abs().t() @ x.abs(), d.abs().t() @ h.abs(), d.abs().sum(0)))
