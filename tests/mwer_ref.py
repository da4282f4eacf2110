"""Float64 oracle of the MWER risk layer (csrc/mwer.hip), written plainly: per utterance the softmax of the negated costs
over the live slots, the expected number of errors under it, and its derivative with respect to every cost.  No shift by
the smallest error count (the kernel's device for exact zeros): the errors enter as they are.  Slots behind ``n_hyp``
and slots whose cost is +inf are excluded explicitly; they get posterior 0 and coefficient 0, and an utterance without a
live slot has risk 0.  Pinned by tests/test_mwer_host.py against torch autograd and central differences."""
import numpy as np


def live_mask(costs, n_hyp=None):
    costs = np.asarray(costs, dtype=np.float64)
    B, N = costs.shape
    live = ~np.isposinf(costs)
    if n_hyp is not None:
        live &= np.arange(N)[None, :] < np.asarray(n_hyp).reshape(B, 1)
    return live


def risk(costs, errs, n_hyp=None, scale=1.0):
    """costs [B, N] (finite or +inf), errs [B, N] integers -> (risk [B], post [B, N], coef [B, N]) in float64, with
    ``coef[b, n] = d(scale * risk[b]) / d costs[b, n] = -scale * post[b, n] * (errs[b, n] - risk[b])``."""
    costs = np.asarray(costs, dtype=np.float64)
    errs = np.asarray(errs)
    B, N = costs.shape
    live = live_mask(costs, n_hyp)
    out_risk = np.zeros(B)
    post = np.zeros((B, N))
    coef = np.zeros((B, N))
    for b in range(B):
        idx = np.nonzero(live[b])[0]
        if idx.size == 0:
            continue
        c = costs[b, idx]
        e = errs[b, idx].astype(np.float64)
        w = np.exp(-(c - c.min()))
        p = w / w.sum()
        r = float((p * e).sum())
        out_risk[b] = r
        post[b, idx] = p
        coef[b, idx] = -scale * p * (e - r)
    return out_risk, post, coef


def reduced(risks, scale=1.0, nll_weight=0.0, ref_costs=None):
    """scale * sum_b (risk_b + nll_weight * ref_costs[b]); without ref_costs the second term is absent."""
    total = np.asarray(risks, dtype=np.float64).copy()
    if ref_costs is not None:
        total = total + nll_weight * np.asarray(ref_costs, dtype=np.float64)
    return scale * float(total.sum())
