"""Float64 numpy restatement of the CTC forced aligner (csrc/ctc_loss.hip, ``ctc_alpha_beta<C, true>`` and
``ctc_viterbi_backtrace``): the oracle of the CTC aligner's tests.

Viterbi over the loss's lattice of ``S = 2 U + 1`` states (blank, y_0, blank, ..., blank):
    v(0,0) = 0.0 + lp(0,0),  v(0,1) = 0.0 + lp(0,1),  v(0,s>1) = -inf
    v(t,s) = max(v(t-1,s), v(t-1,s-1), [skip(s)] v(t-1,s-2)) + lp(t,s)          (one max, then one add)
    score  = max(v(T-1,S-1), v(T-1,S-2))                                          (U = 0: v(T-1,0))
Tie rule - the later emission wins: the path ends in state S - 2 when v(T-1,S-2) >= v(T-1,S-1); walking back from
(t,s), among the predecessors whose v(t-1,.) equals the maximum, s - 2 (where the skip is allowed), else s - 1, else s.

Two forms: ``replay`` on given log-probability planes (fed the kernel's own float32 planes it reproduces the kernel's
float64 ``v`` bit for bit: the same operations in the same order), ``align_one`` / ``align_batch`` from logits through
``ctc_ref.log_softmax``.  test_ctc_align_host.py pins both on the enumeration of all paths.
"""
import numpy as np

import ctc_ref as CR

NEG = -np.inf


def replay(lpb, lpl, y):
    """One utterance: ``lpb`` [T] the blank's and ``lpl`` [T, >= U] the labels' log-probabilities (any float dtype,
    widened to float64 as the kernel widens them), ``y`` the U labels.  Returns ``(frames [U], ends [U], score,
    v [T, S], states [T])``: int64 first / last frame per label, the float64 score, the lattice and the state the
    best path is in on every frame.  No path (T = 0 included): frames and ends of -1, score -inf, states of -1."""
    y = [int(k) for k in y]
    U = len(y)
    S = 2 * U + 1
    lpb = np.asarray(lpb, dtype=np.float64).reshape(-1)
    T = lpb.shape[0]
    lp = np.empty((T, S))
    lp[:, 0::2] = lpb[:, None]
    if U and T:
        lp[:, 1::2] = np.asarray(lpl, dtype=np.float64).reshape(T, -1)[:, :U]
    skip = np.zeros(S, dtype=bool)
    for s in range(3, S, 2):
        skip[s] = y[s // 2] != y[s // 2 - 1]
    v = np.full((T, S), NEG)
    none = (np.full(U, -1, dtype=np.int64), np.full(U, -1, dtype=np.int64), NEG, v, np.full(T, -1, dtype=np.int64))
    if T == 0:
        return none
    v[0, :2] = 0.0 + lp[0, :2]
    for t in range(1, T):
        prev = v[t - 1]
        a1 = np.concatenate([[NEG], prev[:-1]])
        a2 = np.where(skip, np.concatenate([[NEG, NEG], prev[:-2]])[:S], NEG)
        v[t] = np.maximum(np.maximum(prev, a1), a2) + lp[t]
    score = max(v[T - 1, S - 1], v[T - 1, S - 2]) if S >= 2 else v[T - 1, 0]
    if score == NEG:
        return none
    s = S - 1
    if S >= 2 and v[T - 1, S - 2] >= v[T - 1, S - 1]:
        s = S - 2
    states = np.empty(T, dtype=np.int64)
    states[T - 1] = s
    for t in range(T - 1, 0, -1):
        prev = v[t - 1]
        a0 = prev[s]
        a1 = prev[s - 1] if s >= 1 else NEG
        a2 = prev[s - 2] if skip[s] else NEG
        m = max(a0, a1, a2)
        if skip[s] and a2 == m:
            s -= 2
        elif s >= 1 and a1 == m:
            s -= 1
        states[t - 1] = s
    frames = np.full(U, -1, dtype=np.int64)
    ends = np.full(U, -1, dtype=np.int64)
    for t in range(T):
        if states[t] & 1:
            u = states[t] >> 1
            if frames[u] < 0:
                frames[u] = t
            ends[u] = t
    return frames, ends, float(score), v, states


def align_one(logits, y, blank=0):
    """One utterance from ``logits`` [T, V] in float64: ``replay`` on ``ctc_ref.log_softmax``."""
    logits = np.asarray(logits, dtype=np.float64)
    if logits.shape[0] == 0:
        return replay(np.zeros(0), np.zeros((0, len(y))), y)
    lp = CR.log_softmax(logits)
    idx = np.asarray([int(k) for k in y], dtype=np.int64)
    return replay(lp[:, blank], lp[:, idx], y)


def align_batch(logits, labels, act_lens, label_lens, blank=0):
    """Batch: ``logits`` [B, T, V], ``labels`` [B, U].  Returns ``(frames [B, U], ends [B, U], scores [B], states: list
    of [T_b])`` with -1 behind ``label_lens[b]``."""
    logits = np.asarray(logits, dtype=np.float64)
    B, U = logits.shape[0], np.asarray(labels).shape[1]
    frames = np.full((B, U), -1, dtype=np.int64)
    ends = np.full((B, U), -1, dtype=np.int64)
    scores = np.full(B, NEG)
    states = []
    for b in range(B):
        Tb, Ub = max(0, int(act_lens[b])), int(label_lens[b])
        f, e, sc, _, st = align_one(logits[b, :Tb], labels[b][:Ub], blank)
        frames[b, :Ub], ends[b, :Ub], scores[b] = f, e, sc
        states.append(st)
    return frames, ends, scores, states


def path_symbols(states, y, blank=0):
    """The frame-by-frame symbols of a state sequence."""
    return [blank if s % 2 == 0 else int(y[s // 2]) for s in states]


def rescore(logits, states, y, blank=0):
    """The float64 log-probability of a state sequence under ``logits`` [T, V]."""
    lp = CR.log_softmax(logits)
    return float(sum(lp[t, k] for t, k in enumerate(path_symbols(states, y, blank))))


def states_from_spans(frames, ends, T):
    """The state sequence [T] of a path given every label's first and last frame (blank states in between)."""
    states = np.empty(T, dtype=np.int64)
    u, U = 0, len(frames)
    for t in range(T):
        while u < U and t > ends[u]:
            u += 1
        states[t] = 2 * u + 1 if u < U and frames[u] <= t else 2 * u
    return states
