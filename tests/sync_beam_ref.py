"""ORACLE (test infrastructure only): the frame-synchronous beam search of csrc/decode_sync.hip restated in Python
floats over oracle.models_ref (fp64 sums of the fp32 model's log-probs), one utterance at a time.

Per utterance, blank = 0, beam width W:
  1. the beam starts as the empty sequence with logp 0, a zero prediction-network state and last token BOS;
  2. on frame t hypothesis i (in beam order) gives lp_i = log_softmax(joint(enc_t, pred_i)); candidate (i, k) scores
     logp_i + lp_i[k];
  3. the W best candidates are kept, ordered by score descending, then i, then k;
  4. (i, blank) keeps i's sequence, state and per-token detail; (i, k) appends k, recording frame t and lp_i[k];
  5. kept candidates with the same token sequence (identity by tuple) are folded: logp = max + log1p(exp(min - max)),
     at the place of the better ranked one, with the detail and state of the one that did not append on this frame;
  6. after the last frame the beam is sorted by logp descending, ties keeping beam order.
A hypothesis carries the state from BEFORE its last token, as the engine's rows do: expanding it runs the prediction
network on that token.

``search_one`` also returns what the GPU tests need to know that fp32 rounding cannot flip a choice: the smallest
selection margin (kept W-th candidate minus the first dropped one, over all frames), the smallest gap between adjacent
final ranks, and the number of merges."""
import math

import numpy as np
import torch

from oracle import models_ref as M


class _Hyp:
    __slots__ = ("seq", "logp", "tok", "state", "frames", "tlp")

    def __init__(self, seq, logp, tok, state, frames, tlp):
        self.seq, self.logp, self.tok, self.state, self.frames, self.tlp = seq, logp, tok, state, frames, tlp


def search_core(T, W, expand, root_state, root_tok, blank=M.NUL):
    """Steps 1-6 over any model: ``expand(t, tok, state) -> (lp: sequence of V floats, state after tok)``.
    Returns ``(beam, info)``: the ranked list of dicts ``tokens`` / ``frames`` / ``token_logp`` / ``logp`` and
    ``info = dict(margin, rank_gap, merges)``."""
    beam = [_Hyp((), 0.0, root_tok, root_state, (), ())]
    margin, merges = float("inf"), 0
    for t in range(T):
        cands, steps = [], []
        for i, h in enumerate(beam):
            lp, new_state = expand(t, h.tok, h.state)
            steps.append((lp, new_state))
            cands.extend((h.logp + float(lp[k]), i, k) for k in range(len(lp)))
        cands.sort(key=lambda c: (-c[0], c[1], c[2]))
        if len(cands) > W:
            margin = min(margin, cands[W - 1][0] - cands[W][0])
        new, place = [], {}
        for score, i, k in cands[:W]:
            h = beam[i]
            if k == blank:
                child = _Hyp(h.seq, score, h.tok, h.state, h.frames, h.tlp)
            else:
                child = _Hyp(h.seq + (k,), score, k, steps[i][1], h.frames + (t,), h.tlp + (float(steps[i][0][k]),))
            j = place.get(child.seq)
            if j is None:
                place[child.seq] = len(new)
                new.append(child)
                continue
            merges += 1
            old = new[j]
            mx, mn = max(old.logp, child.logp), min(old.logp, child.logp)
            keep = child if k == blank else old      # the one that did not append on this frame: the older node
            new[j] = _Hyp(keep.seq, mx + math.log1p(math.exp(mn - mx)), keep.tok, keep.state, keep.frames, keep.tlp)
        beam = new
    order = sorted(range(len(beam)), key=lambda j: -beam[j].logp)      # stable: ties keep beam order
    ranked = [beam[j] for j in order]
    gaps = [a.logp - b.logp for a, b in zip(ranked, ranked[1:])]
    out = [dict(tokens=list(h.seq), frames=list(h.frames), token_logp=list(h.tlp), logp=h.logp) for h in ranked]
    return out, dict(margin=margin, rank_gap=min(gaps) if gaps else float("inf"), merges=merges)


def search_one(sd, h_enc, W=10, blank=M.NUL):
    """h_enc [T, P_enc] fp32 of ONE utterance -> ``search_core``'s result on the model of the state dict ``sd``."""
    L = M.n_dec_layers(sd)
    H = sd["decoder.lstm.weight_hh_l0"].shape[1]
    zero = (torch.zeros(L, 1, H), torch.zeros(L, 1, H))

    def expand(t, tok, state):
        pred, new_state = M.decoder_forward(sd, torch.tensor([[tok]]), state)
        lp = torch.log_softmax(M.joint_forward(sd, h_enc[t][None, :], pred[:, 0])[0], dim=0)
        return lp.tolist(), new_state

    return search_core(h_enc.shape[0], W, expand, zero, M.BOS, blank)


def encode(sd, xs, xlen=None, time_reductions=(1,)):
    """(h_enc [B, T, P], lens): the encoder and ``scale_length`` as the engine's searches apply them."""
    h_enc, _ = M.encoder_forward(sd, xs, None, time_reductions)
    Bn, T = h_enc.shape[0], h_enc.shape[1]
    lens = [T] * Bn if xlen is None else [int(v) for v in M.scale_length(T, xlen)]
    return h_enc, lens


def search(sd, xs, xlen=None, W=10):
    """xs [B, T0, I] -> (list of B ranked lists, list of B info dicts)."""
    h_enc, lens = encode(sd, xs, xlen)
    res, infos = [], []
    for b in range(h_enc.shape[0]):
        r, info = search_one(sd, h_enc[b, :lens[b]], W)
        res.append(r)
        infos.append(info)
    return res, infos


def sharpened(sd, scale=6.0, blank_bias=3.0):
    """A copy of ``sd`` whose output layer is scaled and whose blank is raised: peaked distributions with a likely blank,
    so that margins are wide and both blank and token children survive."""
    sd = {k: v.clone() for k, v in sd.items()}
    sd["joint.joint.2.weight"] *= scale
    sd["joint.joint.2.bias"] *= scale
    sd["joint.joint.2.bias"][M.NUL] += blank_bias
    return sd
