"""Float64 numpy restatement of the CTC alpha / beta recursion (Graves et al. 2006): the oracle of the CTC tests.

``beta(t, s)`` does NOT contain frame t's own log-probability (the convention of csrc/ctc_loss.hip), so the occupancy
of a state is ``exp(alpha + beta - ll)``.  Written from the definition; test_ctc_host.py checks it against a brute-force
enumeration of all paths and against ``torch.nn.functional.ctc_loss`` in float64.
"""
import numpy as np

NEG = -np.inf


def _lse(*xs):
    m = max(xs)
    if m == NEG:
        return NEG
    return m + np.log(sum(np.exp(x - m) for x in xs))


def log_softmax(z):
    z = np.asarray(z, dtype=np.float64)
    m = z.max(axis=-1, keepdims=True)
    return z - m - np.log(np.exp(z - m).sum(axis=-1, keepdims=True))


def extended(y, blank):
    ext = [blank]
    for v in y:
        ext += [int(v), blank]
    return ext


def ctc_one(logits, y, blank=0):
    """One utterance: ``logits`` [T, V] (T >= 1), ``y`` a sequence of labels.  Returns ``(cost, grad [T, V],
    occupancy [T, S], alpha [T, S], beta [T, S])``; no path: cost +inf, zero gradient and occupancy."""
    lp = log_softmax(logits)
    T, V = lp.shape
    ext = extended(y, blank)
    S = len(ext)
    skip = [s >= 3 and s % 2 == 1 and ext[s] != ext[s - 2] for s in range(S)]
    idx = np.array(ext)
    skip = np.array(skip, dtype=bool)
    pad1, pad2 = np.full(1, NEG), np.full(2, NEG)
    alpha = np.full((T, S), NEG)
    beta = np.full((T, S), NEG)
    alpha[0, :2] = lp[0, idx[:2]]
    for t in range(1, T):                            # (np.logaddexp(-inf, -inf) = -inf)
        prev = alpha[t - 1]
        a1 = np.concatenate([pad1, prev[:-1]])
        a2 = np.where(skip, np.concatenate([pad2, prev[:-2]])[:S], NEG)
        alpha[t] = np.logaddexp(np.logaddexp(prev, a1), a2) + lp[t, idx]
    beta[T - 1, max(0, S - 2):] = 0.0
    skip_from = np.concatenate([skip[2:], np.zeros(2, dtype=bool)])[:S]      # state s + 2 may be entered from s
    for t in range(T - 2, -1, -1):
        e = beta[t + 1] + lp[t + 1, idx]
        b1 = np.concatenate([e[1:], pad1])
        b2 = np.where(skip_from, np.concatenate([e[2:], pad2])[:S], NEG)
        beta[t] = np.logaddexp(np.logaddexp(e, b1), b2)
    ll = _lse(alpha[T - 1, S - 1], alpha[T - 1, S - 2]) if S > 1 else alpha[T - 1, 0]
    grad = np.zeros((T, V))
    occ = np.zeros((T, S))
    if ll == NEG:
        return np.inf, grad, occ, alpha, beta
    with np.errstate(invalid="ignore"):
        occ = np.exp(alpha + beta - ll)          # (-inf + -inf = -inf: no +inf operand)
    occ[~np.isfinite(alpha + beta)] = 0.0
    grad = np.exp(lp)
    for s in range(S):
        grad[:, ext[s]] -= occ[:, s]
    return -ll, grad, occ, alpha, beta


def ctc_batch(logits, labels, act_lens, label_lens, blank=0):
    """Batch: ``logits`` [B, T, V], ``labels`` [B, U].  Returns ``(costs [B], grads [B, T, V], occ: list of [T_b, S_b],
    live: list of bool [T_b, S_b] - the states with finite alpha and finite beta)``.  Rows t >= T_b have zero gradient;
    T_b <= 0 costs +inf."""
    logits = np.asarray(logits, dtype=np.float64)
    B, T, V = logits.shape
    costs = np.zeros(B)
    grads = np.zeros((B, T, V))
    occs, lives = [], []
    for b in range(B):
        Tb, Ub = int(act_lens[b]), int(label_lens[b])
        if Tb <= 0:
            costs[b] = np.inf
            occs.append(np.zeros((0, 2 * Ub + 1)))
            lives.append(np.zeros((0, 2 * Ub + 1), dtype=bool))
            continue
        c, g, o, a, bt = ctc_one(logits[b, :Tb], [int(v) for v in labels[b][:Ub]], blank)
        costs[b] = c
        grads[b, :Tb] = g
        occs.append(o)
        lives.append(np.isfinite(a) & np.isfinite(bt))
    return costs, grads, occs, lives


def repeats(y):
    return sum(1 for i in range(1, len(y)) if y[i] == y[i - 1])


def greedy(logits, act_lens, blank=0):
    """CTC greedy decode of [B, T, V] logits in float64: arg max per frame (lowest index on ties), keep a frame iff its
    symbol is not blank and differs from the frame before.  Returns per utterance (tokens, frames, neglogp)."""
    logits = np.asarray(logits, dtype=np.float64)
    out = []
    for b in range(logits.shape[0]):
        Tb = int(act_lens[b])
        z = logits[b, :Tb]
        k = z.argmax(axis=-1) if Tb else np.zeros(0, dtype=np.int64)
        lp = log_softmax(z) if Tb else np.zeros((0, logits.shape[2]))
        toks, frs, nl = [], [], 0.0
        for t in range(Tb):
            if k[t] != blank and (t == 0 or k[t] != k[t - 1]):
                toks.append(int(k[t]))
                frs.append(t)
                nl -= lp[t, k[t]]
        out.append((np.array(toks, dtype=np.int64), np.array(frs, dtype=np.int64), nl))
    return out
