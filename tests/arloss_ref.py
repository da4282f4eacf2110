"""float64 restatements of the alignment-restricted RNN-T loss (per-label emission windows; Mahadeokar et al. 2021)
shared by test_arloss_host.py and test_arloss_gpu.py (test-local code; the lattice recursion and the log-softmax are
oracle/rnnt_loss_ref.py's, unmodified: the windows reach them as a copy of the log-probabilities in which the label
entry of every masked cell is -inf).

Label u (0-based) may be emitted - the step (t,u) -> (t,u+1) - on the frames lo[u] <= t <= hi[u] only; blanks are never
restricted.  With the restricted alpha, beta and L (cost = -L; +inf where no alignment respects the windows):

    wb(t,u) = exp(a(t,u) + lpb(t,u) + beta(t+1,u) - L)      (last frame: only at u = U, without the beta term)
    wl(t,u) = exp(a(t,u) + lpl(t,u) + beta(t,u+1) - L)      (u < U and lo[u] <= t <= hi[u], else 0)
    grad(t,u,k) = softmax_k (wb + (1 + lambda) wl) - [k == blank] wb - [k == y_u] (1 + lambda) wl

and an all-zero row wherever a(t,u) = -inf or beta(t,u) = -inf.  Band: elo_u = max(lo_0..lo_u),
ehi_u = min(hi_u..hi_{U-1}, T-1); column u is alive on the frames [elo_{u-1}, ehi_u] (column 0 from frame 0, column U
up to T-1); no alignment exists iff elo_u > ehi_u for some u."""
import itertools

import numpy as np
import torch

import fastemit_ref as FR
from oracle.rnnt_loss_ref import lattice, log_softmax


def masked_lp(lp, labels, T, U, lo, hi, blank=0):
    """Copy of lp [T, U+1, V] with the label entry of every cell outside its window set to -inf."""
    out = np.array(lp[:T, :U + 1], dtype=np.float64, copy=True)
    for u in range(U):
        y = int(labels[u])
        assert y != blank
        for t in range(T):
            if not (int(lo[u]) <= t <= int(hi[u])):
                out[t, u, y] = -np.inf
    return out


def ar_lattice(z, labels, T, U, lo, hi, blank=0):
    """(lp, lp_masked, alpha, beta, ll) of ONE utterance from its float64 logits block z [>=T, >=U+1, V]."""
    lp = log_softmax(np.asarray(z, dtype=np.float64)[:T, :U + 1])
    lpm = masked_lp(lp, labels, T, U, lo, hi, blank)
    alpha, beta, ll = lattice(lpm, labels, T, U, blank)
    return lp, lpm, alpha, beta, ll


def ar_grad_one(z, labels, T, U, lo, hi, lam=0.0, blank=0):
    """(cost, grad [T, U+1, V], live [T, U+1] bool) of one utterance; cost +inf and grad 0 without an alignment."""
    lp, lpm, alpha, beta, ll = ar_lattice(z, labels, T, U, lo, hi, blank)
    live = np.isfinite(alpha) & np.isfinite(beta)
    g = np.zeros_like(lp)
    if not np.isfinite(ll):
        assert not live.any()
        return np.inf, g, live
    for t in range(T):
        for u in range(U + 1):
            if not live[t, u]:
                continue
            a = alpha[t, u]
            wb = wl = 0.0
            if t < T - 1:
                wb = np.exp(a + lp[t, u, blank] + beta[t + 1, u] - ll)
            elif u == U:
                wb = np.exp(a + lp[t, u, blank] - ll)
            if u < U and np.isfinite(lpm[t, u, labels[u]]):
                wl = np.exp(a + lp[t, u, labels[u]] + beta[t, u + 1] - ll)
            g[t, u] = np.exp(lp[t, u]) * (wb + (1.0 + lam) * wl)
            g[t, u, blank] -= wb
            if u < U:
                g[t, u, labels[u]] -= (1.0 + lam) * wl
    return -ll, g, live


def ar_loss(acts, labels, act_lens, label_lens, lo, hi, lam=0.0, blank=0):
    """costs [B], gradient [B, T, U1, V] (zeros outside the boxes and on dead cells), live [B, T, U1] bool."""
    acts = np.asarray(acts, dtype=np.float64)
    B = acts.shape[0]
    costs = np.zeros(B)
    grads = np.zeros_like(acts)
    live = np.zeros(acts.shape[:3], dtype=bool)
    for b in range(B):
        T, U = int(act_lens[b]), int(label_lens[b])
        costs[b], grads[b, :T, :U + 1], live[b, :T, :U + 1] = ar_grad_one(
            acts[b], np.asarray(labels[b]), T, U, np.asarray(lo[b]), np.asarray(hi[b]), lam, blank)
    return costs, grads, live


def ar_autograd_one(z, labels, T, U, lo, hi, lam=0.0, blank=0):
    """The same cost and gradient by autograd through a float64 alpha recursion that leaves the masked label steps out
    (and scales the gradient of the label log-probabilities by 1 + lambda: FastEmit's definition).  None where no
    alignment exists."""
    zt = torch.tensor(np.asarray(z, dtype=np.float64)[:T, :U + 1], requires_grad=True)
    lp = torch.log_softmax(zt, dim=-1)
    alpha = [[None] * (U + 1) for _ in range(T)]
    for t in range(T):
        for u in range(U + 1):
            if t == 0 and u == 0:
                alpha[t][u] = torch.zeros((), dtype=torch.float64)
                continue
            terms = []
            if t > 0 and alpha[t - 1][u] is not None:
                terms.append(alpha[t - 1][u] + lp[t - 1, u, blank])
            if u > 0 and alpha[t][u - 1] is not None and int(lo[u - 1]) <= t <= int(hi[u - 1]):
                terms.append(alpha[t][u - 1] + FR._ScaleGrad.apply(lp[t, u - 1, int(labels[u - 1])], 1.0 + lam))
            alpha[t][u] = torch.logsumexp(torch.stack(terms), 0) if terms else None
    if alpha[T - 1][U] is None:
        return None
    cost = -(alpha[T - 1][U] + lp[T - 1, U, blank])
    cost.backward()
    return cost.item(), zt.grad.numpy()


def respects(frames, lo, hi):
    return all(int(lo[u]) <= int(f) <= int(hi[u]) for u, f in enumerate(frames))


def ar_enumerate(lpb, lpl, lo, hi):
    """Every window-respecting alignment enumerated: (log of the summed probability, best score, the frames tuples that
    reach it, number of alignments).  lpb [T, U+1], lpl [T, U] UNMASKED (fastemit_ref.cell_logprobs)."""
    T, U1 = lpb.shape
    total, best, arg, n = -np.inf, -np.inf, [], 0
    for frames in itertools.combinations_with_replacement(range(T), U1 - 1):
        if not respects(frames, lo, hi):
            continue
        s = FR.path_score(lpb, lpl, frames)
        total = np.logaddexp(total, s)
        n += 1
        if s > best:
            best, arg = s, [frames]
        elif s == best:
            arg.append(frames)
    return total, best, arg, n


def band_one(T, U, lo, hi):
    """(live [T, U+1] bool, feasible, band [T, 2]) from the windows alone; band[t] = (first, last) live column of frame
    t, (0, -1) where it has none."""
    elo, ehi = [0] * U, [0] * U
    m = 0
    for u in range(U):
        m = max(m, int(lo[u]))
        elo[u] = m
    m = T - 1
    for u in range(U - 1, -1, -1):
        m = min(m, int(hi[u]))
        ehi[u] = m
    feasible = all(elo[u] <= ehi[u] for u in range(U))
    live = np.zeros((T, U + 1), dtype=bool)
    if feasible:
        for u in range(U + 1):
            first = elo[u - 1] if u > 0 else 0
            last = ehi[u] if u < U else T - 1
            live[first:last + 1, u] = True
    band = np.zeros((T, 2), dtype=np.int64)
    band[:, 1] = -1
    for t in range(T):
        cols = np.nonzero(live[t])[0]
        if len(cols):
            assert (np.diff(cols) == 1).all()               # one interval per frame
            band[t] = (cols[0], cols[-1])
    return live, feasible, band


def band_table(lo, hi, act_lens, label_lens, Tm):
    """band [B, Tm, 2] and cells [B] for a batch (frames behind T_b: (0, -1))."""
    B = len(act_lens)
    band = np.zeros((B, Tm, 2), dtype=np.int64)
    band[:, :, 1] = -1
    cells = np.zeros(B, dtype=np.int64)
    for b in range(B):
        T, U = int(act_lens[b]), int(label_lens[b])
        live, _, band[b, :T] = band_one(T, U, lo[b], hi[b])
        cells[b] = live.sum()
    return band, cells


def live_from_band(band, U1):
    """[B, T, U1] bool from a band table."""
    band = np.asarray(band)
    u = np.arange(U1)[None, None, :]
    return (u >= band[:, :, :1]) & (u <= band[:, :, 1:])


def ar_viterbi_one(lpb, lpl, lo, hi):
    """(score, frames [U]) of the best window-respecting alignment (ties come from the blank predecessor);
    (-inf, all -1) where there is none."""
    T, U1 = lpb.shape
    U = U1 - 1
    lplm = np.array(lpl, dtype=np.float64, copy=True)
    for u in range(U):
        for t in range(T):
            if not (int(lo[u]) <= t <= int(hi[u])):
                lplm[t, u] = -np.inf
    if not band_one(T, U, lo, hi)[1]:
        return -np.inf, np.full(U, -1, dtype=np.int64)
    return FR.viterbi_one(lpb, lplm)


def windows_from_frames(frames, act_lens, label_lens, left, right, Tm):
    """alignment_windows' definition: lo = max(0, f - left), hi = min(T_b - 1, f + right); behind the labels 0, Tm - 1."""
    frames = np.asarray(frames)
    lo = np.zeros_like(frames)
    hi = np.full_like(frames, Tm - 1)
    for b in range(frames.shape[0]):
        U = int(label_lens[b])
        lo[b, :U] = np.maximum(0, frames[b, :U] - left)
        hi[b, :U] = np.minimum(int(act_lens[b]) - 1, frames[b, :U] + right)
    return lo, hi


def random_alignment(rng, act_lens, label_lens, U):
    """frames [B, U] int32: sorted random frames < T_b for the labels of each utterance, -1 behind them."""
    B = len(act_lens)
    frames = np.full((B, U), -1, dtype=np.int32)
    for b in range(B):
        n = int(label_lens[b])
        frames[b, :n] = np.sort(rng.integers(0, int(act_lens[b]), size=n))
    return frames
