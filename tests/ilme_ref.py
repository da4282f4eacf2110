"""ORACLE (test infrastructure only): internal-LM estimation (ILME) in the frame-synchronous beam search
(csrc/decode_sync.hip, sync_row_topw_ilm; decode.sync_beam_search*(ilm_weight=)) and the internal LM as a scorer
(csrc/ilm_score.hip; Transducer.ilm_logprobs) restated in Python floats on ``sync_fusion_ref``: its ``Fusion`` gains the
ILM term, and ``search_core`` / ``StreamSearch`` - which ask the fusion for a frame's candidates - run on it as they are.
The model arithmetic is oracle/models_ref.py's; none of it is restated here.

For hypothesis i whose last token is ``tok`` and whose prediction-network state from before it is ``state``:
  * pred = the prediction network's output after ``tok`` (``M.decoder_forward``);
  * z_ilm = ``M.joint_forward(sd, zeros, pred)``: the joint on an all-zero encoder row;
  * lp_ilm[k] = (z_ilm[k] - m) - log(sum_{v != blank} exp(z_ilm[v] - m)), m = max_{v != blank} z_ilm[v]; blank has none;
  * a non-blank k scores, Python floats in this order,
      c = logp_i + lp_i[k];  c = c + (lm_weight * lp_lm_i[k] + length_bonus);  c = c - ilm_weight * lp_ilm_i[k];
      c = c + D(i, k)
    where a term is absent when its feature is; blank scores ``logp_i + lp_i[blank]``; ``token_logp`` stays lp_i[k].
ILME carries no state of its own: selection, folding, ranking, the tree and the commit rule are ``sync_fusion_ref``'s."""
import math

import torch

import sync_fusion_ref as F
from oracle import models_ref as M


def ilm_log_softmax(z, blank=M.NUL):
    """The blank-excluded log-softmax of one row of logits (a list or 1-D tensor) as a list of Python floats; the blank's
    entry is None."""
    z = [float(v) for v in (z.tolist() if torch.is_tensor(z) else z)]
    rest = [v for k, v in enumerate(z) if k != blank]
    m = max(rest)
    logs = math.log(sum(math.exp(v - m) for v in rest))
    return [None if k == blank else (v - m) - logs for k, v in enumerate(z)]


def model_ilm(sd, blank=M.NUL):
    """``ilm(tok, state) -> lp_ilm`` (list, None at blank) of the transducer ``sd``: the row's internal-LM
    log-probabilities from its last token and the prediction-network state from before it."""
    P = sd["joint.joint.0.weight"].shape[1] - sd["decoder.proj.weight"].shape[0]

    def ilm(tok, state):
        pred, _ = M.decoder_forward(sd, torch.tensor([[tok]]), state)
        return ilm_log_softmax(M.joint_forward(sd, torch.zeros(1, P, dtype=pred.dtype), pred[:, 0])[0], blank)

    return ilm


class Fusion(F.Fusion):
    """``sync_fusion_ref.Fusion`` with ``ilm`` (``ilm(tok, state) -> lp_ilm``, see ``model_ilm``) and ``ilm_weight``
    (None: no ILME, the base class's candidates to the last bit)."""

    def __init__(self, ilm=None, ilm_weight=None, **kw):
        super().__init__(**kw)
        self.ilm, self.ilm_weight = ilm, ilm_weight

    def candidates(self, rows, t, expand, blank):
        if self.ilm_weight is None:
            return super().candidates(rows, t, expand, blank)
        cands, steps = [], []
        for i, h in enumerate(rows):
            lp, new_state = expand(t, h.tok, h.state)
            lp_lm, lm_new = self.lm_step(h.lm_tok, h.lm_state)
            lp_ilm = self.ilm(h.tok, h.state)
            steps.append((lp, new_state, lm_new))
            for k in range(len(lp)):
                score, d = h.logp + float(lp[k]), 0.0
                if k != blank:
                    if self.lm is not None:
                        score = score + (self.lm_weight * float(lp_lm[k]) + self.length_bonus)
                    score = score - self.ilm_weight * lp_ilm[k]
                    if self.bias is not None:
                        d = self.delta(h.seq, k)
                        score = score + d
                cands.append((score, i, k, d))
        cands.sort(key=lambda c: (-c[0], c[1], c[2]))
        return cands, steps


search_core = F.search_core         # (they ask ``fusion.candidates`` for the frame: the ILM term is in there)
search_one = F.search_one
search = F.search


def stream_search(sd, h_enc, W, fusion, blank=M.NUL):
    """The streaming form over ONE stream's encoder output ``h_enc`` [T, P]: a ``sync_fusion_ref.StreamSearch`` on the
    ILME fusion; ``advance(n)`` takes the next n frames, ``beam()`` is the offline oracle's list over the frames so far."""
    expand, zero = F.model_expand(sd, h_enc)
    return F.StreamSearch(W, expand, zero, M.BOS, fusion, blank)


def ilm_logprobs(sd, ys, ylen, blank=M.NUL):
    """Teacher-forced per-token internal-LM log-probabilities: nested lists [B][U], 0.0 behind ``ylen``.  The prediction
    network runs from BOS (``M.decoder_forward`` without a state); position u scores ys[b, u]."""
    ys = torch.as_tensor(ys)
    B, U = ys.shape
    P = sd["joint.joint.0.weight"].shape[1] - sd["decoder.proj.weight"].shape[0]
    h_dec, _ = M.decoder_forward(sd, ys, None)              # [B, U + 1, P2]
    out = []
    for b in range(B):
        row = []
        for u in range(U):
            if u >= int(ylen[b]):
                row.append(0.0)
                continue
            z = M.joint_forward(sd, torch.zeros(1, P, dtype=h_dec.dtype), h_dec[b, u][None])[0]
            row.append(ilm_log_softmax(z, blank)[int(ys[b, u])])
        out.append(row)
    return out
