"""Float64 numpy oracle of the N-best CTC scorer (csrc/ctc_score.hip, ``loss.ctc_score_nbest``) and a restatement of the
combine-and-sort rule of ``decode.ctc_rescore``.

The score of a hypothesis is minus ``ctc_ref.ctc_one``'s cost on the utterance's first ``T_b`` rows: ``-inf`` where the
cost is ``+inf``, where ``T_b = 0``, where a token lies outside ``[0, V)`` and for a slot beyond ``n_hyp``.
test_ctc_score_host.py pins it on the enumeration of all frame labellings.
"""
import numpy as np

import ctc_ref as CR

NEG = -np.inf


def score_one(logits, y, blank=0):
    """``logits`` [T, V] (T >= 0), ``y`` a token sequence without blanks: log of the summed probability of all CTC
    paths of ``y``."""
    logits = np.asarray(logits, dtype=np.float64)
    T, V = logits.shape
    y = [int(v) for v in y]
    if T == 0 or any(v < 0 or v >= V for v in y):
        return NEG
    cost = CR.ctc_one(logits, y, blank)[0]
    return NEG if cost == np.inf else -cost


def score_nbest(logits, act_lens, hyps, hyp_lens, n_hyp=None, blank=0):
    """``logits`` [B, T, V], ``hyps`` [B, N, U], ``hyp_lens`` [B, N], ``n_hyp`` [B] or None (all N): float64 [B, N]."""
    logits = np.asarray(logits, dtype=np.float64)
    hyps, hyp_lens = np.asarray(hyps), np.asarray(hyp_lens)
    B, N = hyps.shape[:2]
    out = np.full((B, N), NEG)
    for b in range(B):
        live = N if n_hyp is None else int(n_hyp[b])
        for n in range(live):
            out[b, n] = score_one(logits[b, :int(act_lens[b])], hyps[b, n, :int(hyp_lens[b, n])], blank)
    return out


def has_path(y, Tb):
    """A hypothesis has a CTC path over ``Tb`` frames iff ``Tb >= max(1, len(y) + repeats(y))``."""
    return Tb >= max(1, len(y) + CR.repeats(list(y)))


def combine(logp, ctc_logp, weight):
    """The rule of ``decode.ctc_rescore`` on one list: ``(combined, order)``.  ``combined[i] = logp[i] + weight *
    ctc_logp[i]`` in float64, for ``weight == 0`` ``logp[i]`` itself; ``order``: indices by ``combined`` descending,
    ties in their original order (Python's ``sorted`` is stable)."""
    logp = [float(v) for v in logp]
    ctc_logp = [float(v) for v in ctc_logp]
    if weight == 0:
        combined = list(logp)
    else:
        combined = [np.float64(a) + np.float64(weight) * np.float64(c) for a, c in zip(logp, ctc_logp)]
    order = sorted(range(len(combined)), key=lambda i: -combined[i])
    return np.array(combined, dtype=np.float64), np.array(order, dtype=np.int64)
