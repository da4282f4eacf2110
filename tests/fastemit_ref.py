"""float64 restatements shared by test_fastemit_host.py, test_fastemit_gpu.py and test_rnnt_align_gpu.py (test-local
code; the lattice recursion and the log-softmax are oracle/rnnt_loss_ref.py's, unmodified).

FastEmit gradient (Yu et al. 2021), per utterance, cell (t, u), a = alpha, L = log-likelihood, y = labels[u]:

    wb(t,u) = exp(a(t,u) + lpb(t,u) + beta(t+1,u) - L)      (last frame: only at u = U, without the beta term)
    wl(t,u) = exp(a(t,u) + lpl(t,u) + beta(t,u+1) - L)      (u < U, else 0)
    grad(t,u,k) = softmax_k (wb + (1 + lambda) wl) - [k == blank] wb - [k == y] (1 + lambda) wl

Viterbi:  v(t,u) = max(v(t-1,u) + lpb(t-1,u), v(t,u-1) + lpl(t,u-1)),  score = v(T-1,U) + lpb(T-1,U); where both
predecessors score equal the path comes from the blank one (t - 1)."""
import itertools

import numpy as np
import torch

from oracle.rnnt_loss_ref import lattice, log_softmax


def fastemit_grad_one(z, labels, T, U, lam, blank=0):
    """(cost, grad [T, U+1, V]) of ONE utterance from its float64 logits block z [>=T, >=U+1, V]."""
    lp = log_softmax(np.asarray(z, dtype=np.float64)[:T, :U + 1])
    alpha, beta, ll = lattice(lp, labels, T, U, blank)
    wb = np.zeros((T, U + 1))
    wl = np.zeros((T, U + 1))
    for t in range(T):
        for u in range(U + 1):
            if t < T - 1:
                wb[t, u] = np.exp(alpha[t, u] + lp[t, u, blank] + beta[t + 1, u] - ll)
            elif u == U:
                wb[t, u] = np.exp(alpha[t, u] + lp[t, u, blank] - ll)
            if u < U:
                wl[t, u] = np.exp(alpha[t, u] + lp[t, u, labels[u]] + beta[t, u + 1] - ll)
    g = np.exp(lp) * (wb + (1.0 + lam) * wl)[:, :, None]
    for t in range(T):
        for u in range(U + 1):
            g[t, u, blank] -= wb[t, u]
            if u < U:
                g[t, u, labels[u]] -= (1.0 + lam) * wl[t, u]
    return -ll, g


def fastemit_loss(acts, labels, act_lens, label_lens, lam, blank=0):
    """costs [B] (the PLAIN negative log-likelihoods) and the FastEmit gradient [B, T, U1, V], zeros outside the boxes."""
    acts = np.asarray(acts, dtype=np.float64)
    costs = np.zeros(acts.shape[0])
    grads = np.zeros_like(acts)
    for b in range(acts.shape[0]):
        T, U = int(act_lens[b]), int(label_lens[b])
        costs[b], grads[b, :T, :U + 1] = fastemit_grad_one(acts[b], np.asarray(labels[b]), T, U, lam, blank)
    return costs, grads


class _ScaleGrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, s):
        ctx.s = s
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.s, None


def fastemit_autograd_one(z, labels, T, U, lam, blank=0):
    """The same gradient by autograd: -log-likelihood through a float64 alpha recursion in which the gradient of the
    label log-probabilities is scaled by 1 + lambda (the definition of FastEmit)."""
    zt = torch.tensor(np.asarray(z, dtype=np.float64)[:T, :U + 1], requires_grad=True)
    lp = torch.log_softmax(zt, dim=-1)
    lpb = lp[:, :, blank]
    neg = torch.tensor(float("-inf"), dtype=torch.float64)
    alpha = [[None] * (U + 1) for _ in range(T)]
    for t in range(T):
        for u in range(U + 1):
            if t == 0 and u == 0:
                alpha[t][u] = torch.zeros((), dtype=torch.float64)
                continue
            stay = alpha[t - 1][u] + lpb[t - 1, u] if t > 0 else neg
            emit = alpha[t][u - 1] + _ScaleGrad.apply(lp[t, u - 1, int(labels[u - 1])], 1.0 + lam) if u > 0 else neg
            alpha[t][u] = torch.logsumexp(torch.stack([stay, emit]), 0)
    cost = -(alpha[T - 1][U] + lpb[T - 1, U])
    cost.backward()
    return cost.item(), zt.grad.numpy()


def cell_logprobs(z, labels, T, U, blank=0):
    """(lpb [T, U+1], lpl [T, U]) of one utterance in float64."""
    lp = log_softmax(np.asarray(z, dtype=np.float64)[:T, :U + 1])
    lpb = lp[:, :, blank]
    lpl = np.stack([lp[:, u, int(labels[u])] for u in range(U)], axis=1) if U > 0 else np.zeros((T, 0))
    return lpb, lpl


def viterbi_one(lpb, lpl):
    """(score, frames [U]) of the best alignment; ties come from the blank predecessor."""
    T, U1 = lpb.shape
    U = U1 - 1
    v = np.full((T, U1), -np.inf)
    v[0, 0] = 0.0
    for t in range(T):
        for u in range(U1):
            if t == 0 and u == 0:
                continue
            stay = v[t - 1, u] + lpb[t - 1, u] if t > 0 else -np.inf
            emit = v[t, u - 1] + lpl[t, u - 1] if u > 0 else -np.inf
            v[t, u] = max(stay, emit)
    frames = np.zeros(U, dtype=np.int64)
    t, u = T - 1, U
    while u > 0:
        stay = v[t - 1, u] + lpb[t - 1, u] if t > 0 else -np.inf
        emit = v[t, u - 1] + lpl[t, u - 1]
        if emit > stay:
            frames[u - 1] = t
            u -= 1
        else:
            t -= 1
    return v[T - 1, U] + lpb[T - 1, U], frames


def path_score(lpb, lpl, frames):
    """log-probability of the alignment that emits label u on frame frames[u] (non-decreasing, inside [0, T))."""
    T, U1 = lpb.shape
    frames = [int(f) for f in frames]
    assert len(frames) == U1 - 1
    s, t = 0.0, 0
    for u, f in enumerate(frames):
        assert t <= f < T
        while t < f:
            s += lpb[t, u]
            t += 1
        s += lpl[t, u]
    while t < T:
        s += lpb[t, U1 - 1]
        t += 1
    return s


def viterbi_bruteforce(lpb, lpl):
    """Every alignment enumerated: (best score, list of the frames tuples that reach it)."""
    T, U1 = lpb.shape
    best, arg = -np.inf, []
    for frames in itertools.combinations_with_replacement(range(T), U1 - 1):
        s = path_score(lpb, lpl, frames)
        if s > best:
            best, arg = s, [frames]
        elif s == best:
            arg.append(frames)
    return best, arg
