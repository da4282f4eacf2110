"""CPU restatement of the beam search WITH per-token detail, shared by test_nbest_host.py and test_nbest_gpu.py
(test-local code; the model arithmetic is oracle/models_ref.py's, unmodified).

``nbest_one`` is oracle/beam_ref.beam_search_one (prefix=False) with one difference: every hypothesis carries, per
token, the encoder frame on which the expansion that produced it ran and the increment the token added to the score
(child score - score of the popped parent, a Python-float difference), and the WHOLE final list B is returned, in
B's order (insertion order).  With ``lm`` (an object with ``zero()`` / ``forward(tokens, hidden)``, the RefLM of
tests/test_lm_fusion_gpu.py) a non-blank child scores ``logp(y*) + lp_rnnt[k] + (lm_weight * lp_lm[k] + length_bonus)``
as the fused search states it there.

It also reports the smallest gap between the best and the second-best candidate of A over all pops: a search in fp32
arithmetic can only be expected to take the same pops where that gap is well above its score error.

``path_logp`` re-scores a hypothesis from a dense log-softmax lattice, independently of any search:
the path that emits token u on frames[u] and a blank on every frame has
    log p = sum_u lp[frames[u], u, y_u] + sum_t lp[t, #{u: frames[u] <= t}, blank]."""
import numpy as np
import torch

from oracle import models_ref as M


class _Hyp:
    __slots__ = ("k", "tok", "h", "logp", "frames", "incs", "lm_tok", "lm_h")

    def __init__(self, k, tok, h, logp, frames, incs, lm_tok=None, lm_h=None):
        self.k, self.tok, self.h, self.logp, self.frames, self.incs = k, tok, h, logp, frames, incs
        self.lm_tok, self.lm_h = lm_tok, lm_h


def _pop_gap(A):
    if len(A) < 2:
        return float("inf")
    v = np.array([a.logp for a in A])
    i = int(v.argmax())
    best = v[i]
    v[i] = -np.inf
    return float(best - v.max())


def nbest_one(sd, h_enc, W=10, blank=M.NUL, lm=None, lm_weight=0.0, length_bonus=0.0, lm_bos=1):
    """h_enc [T, P_enc] fp32 of ONE utterance -> (B, expansions, min_gap); B a list of dicts with ``tokens`` (list),
    ``frames`` (list), ``token_logp`` (list of floats), ``logp`` (float, log p - fused with an LM)."""
    L = M.n_dec_layers(sd)
    H = sd["decoder.lstm.weight_hh_l0"].shape[1]
    zero = (torch.zeros(L, 1, H), torch.zeros(L, 1, H))
    V = sd["joint.joint.2.weight"].shape[0]
    B = [_Hyp([], M.BOS, zero, 0.0, [], [], lm_bos, lm.zero() if lm is not None else None)]
    n_expansions = 0
    min_gap = float("inf")
    for t, x in enumerate(h_enc):
        A = B
        B = []
        while True:
            min_gap = min(min_gap, _pop_gap(A))
            y_hat = max(A, key=lambda a: a.logp)
            A.remove(y_hat)
            pred, hidden = M.decoder_forward(sd, torch.tensor([[y_hat.tok]]), y_hat.h)
            logits = M.joint_forward(sd, x[None, :], pred[:, 0])[0]
            logp = torch.log_softmax(logits, dim=0)
            if lm is not None:
                lp_lm, lm_hidden = lm.forward(torch.tensor([[y_hat.lm_tok]]), y_hat.lm_h)
                lp_lm = lp_lm[0]
            n_expansions += 1
            for k in range(V):
                if k == blank:
                    B.append(_Hyp(y_hat.k, y_hat.tok, y_hat.h, y_hat.logp + float(logp[k]), y_hat.frames, y_hat.incs,
                                  y_hat.lm_tok, y_hat.lm_h))
                    continue
                if lm is not None:
                    lp = y_hat.logp + float(logp[k]) + (lm_weight * float(lp_lm[k]) + length_bonus)
                    A.append(_Hyp(y_hat.k + [k], k, hidden, lp, y_hat.frames + [t], y_hat.incs + [lp - y_hat.logp], k,
                                  lm_hidden))
                else:
                    lp = y_hat.logp + float(logp[k])
                    A.append(_Hyp(y_hat.k + [k], k, hidden, lp, y_hat.frames + [t], y_hat.incs + [lp - y_hat.logp]))
            y_a = max(A, key=lambda a: a.logp)
            y_b = max(B, key=lambda a: a.logp)
            if len(B) >= W and y_b.logp >= y_a.logp:
                break
        B = B[:W]
    out = [dict(tokens=list(h.k), frames=list(h.frames), token_logp=list(h.incs), logp=h.logp) for h in B]
    return out, n_expansions, min_gap


def encode(sd, xs, xlen=None, time_reductions=(1,)):
    """(h_enc [B, T, P], lens) as oracle/beam_ref.beam_search takes them."""
    h_enc, _ = M.encoder_forward(sd, xs, None, time_reductions)
    Bn, T = h_enc.shape[0], h_enc.shape[1]
    lens = [T] * Bn if xlen is None else [int(v) for v in M.scale_length(T, xlen)]
    return h_enc, lens


def nbest(sd, xs, xlen=None, W=10, **kw):
    """xs [B, T0, I] -> (list of B lists, total expansions, smallest pop gap of the batch)."""
    h_enc, lens = encode(sd, xs, xlen)
    res, total, gap = [], 0, float("inf")
    for b in range(h_enc.shape[0]):
        r, n, g = nbest_one(sd, h_enc[b, :lens[b]], W, **kw)
        res.append(r)
        total += n
        gap = min(gap, g)
    return res, total, gap


def lattice_logp(sd, h_enc, tokens):
    """Dense log-softmax lattice lp [T, U + 1, V] (float64 of the fp32 model arithmetic) of one utterance for the label
    sequence ``tokens``: the prediction network reads BOS + tokens, the joint every (t, u) pair."""
    ys = torch.tensor([[M.BOS] + [int(k) for k in tokens]])
    L = M.n_dec_layers(sd)
    H = sd["decoder.lstm.weight_hh_l0"].shape[1]
    state = (torch.zeros(L, 1, H), torch.zeros(L, 1, H))
    preds = []
    for u in range(ys.shape[1]):
        pred, state = M.decoder_forward(sd, ys[:, u:u + 1], state)
        preds.append(pred[0, 0])
    rows = []
    for x in h_enc:
        rows.append(torch.stack([torch.log_softmax(M.joint_forward(sd, x[None, :], p[None, :])[0], dim=0)
                                 for p in preds]))
    if not rows:
        return np.zeros((0, len(preds), sd["joint.joint.2.weight"].shape[0]))
    return torch.stack(rows).double().numpy()


def path_logp(lp, tokens, frames, blank=M.NUL):
    """(log p of the path, the per-token terms lp[frames[u], u, y_u]) - see the module docstring."""
    T = lp.shape[0]
    frames = np.asarray(frames, dtype=np.int64)
    terms = np.array([lp[frames[u], u, int(tokens[u])] for u in range(len(tokens))], dtype=np.float64)
    total = float(terms.sum())
    for t in range(T):
        total += float(lp[t, int((frames <= t).sum()), blank])
    return total, terms
