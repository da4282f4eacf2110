"""CPU oracle of the beam search with contextual biasing, shared by test_bias_host.py and test_bias_gpu.py (test-local
code; the model arithmetic is oracle/models_ref.py's, unmodified).

``bias_beam_one`` is the fused fp64 beam loop of tests/test_lm_fusion_gpu.py (``fused_beam_one``, itself a copy of
oracle/beam_ref.beam_search_one with ``prefix=False``) with a bias state per hypothesis and, as tests/nbest_ref.py
keeps them, the frame and the score increment of every token; it returns the WHOLE final list B.

The automaton is written independently of ``edgedict_amd.bias.ContextGraph``, by brute force (``BruteBias``):
  * the state after a token sequence y is the longest suffix of y that is a prefix of some phrase (a trie path), found
    by trying every suffix length from the longest phrase down;
  * ``held`` / ``pend`` of a path are computed by walking it from the root: ``held = pend(parent) + beta(edge)`` with
    ``beta(edge)`` the largest boost of the phrases that share the edge, ``pend = 0`` where a phrase ends (its bonus is
    banked) and ``held`` elsewhere;
  * consuming k after y adds ``D = held(state(y + [k])) - pend(state(y))``.
A non-blank child k of the popped hypothesis y* scores ``(logp(y*) + lp_rnnt[k]) + D``, with an LM
``((logp(y*) + lp_rnnt[k]) + (lm_weight * lp_lm[k] + length_bonus)) + D`` (Python floats, in this order); the blank
child keeps ``logp(y*) + lp_rnnt[blank]``."""
import numpy as np
import torch

from oracle import models_ref as M


class BruteBias:
    def __init__(self, phrases, boost, phrase_boosts=None):
        self.phrases = [tuple(int(k) for k in p) for p in phrases]
        if phrase_boosts is None:
            self.boosts = [float(boost)] * len(self.phrases)
        else:
            self.boosts = [float(boost) if x is None else float(x) for x in phrase_boosts]
        self.ends = set(self.phrases)
        self.paths = {()}
        for p in self.phrases:
            for i in range(1, len(p) + 1):
                self.paths.add(p[:i])
        self.maxlen = max([len(p) for p in self.phrases], default=0)

    def state(self, tokens):
        """The longest suffix of ``tokens`` that is a trie path, as a tuple."""
        tokens = tuple(int(k) for k in tokens)
        for n in range(min(self.maxlen, len(tokens)), 0, -1):
            if tokens[len(tokens) - n:] in self.paths:
                return tokens[len(tokens) - n:]
        return ()

    def beta(self, path):
        return max(b for p, b in zip(self.phrases, self.boosts) if p[:len(path)] == path)

    def held_pend(self, path):
        held = pend = 0.0
        for i in range(1, len(path) + 1):
            held = pend + self.beta(path[:i])
            pend = 0.0 if path[:i] in self.ends else held
        return held, pend

    def delta(self, tokens, k):
        """The increment of token k after the sequence ``tokens``."""
        s = self.state(tokens)
        n = self.state(tuple(tokens) + (int(k),))
        return self.held_pend(n)[0] - self.held_pend(s)[1]

    def score(self, tokens):
        total = 0.0
        for i, k in enumerate(tokens):
            total += self.delta(tokens[:i], k)
        return total


class _Hyp:
    __slots__ = ("k", "tok", "h", "logp", "frames", "incs", "lm_tok", "lm_h")

    def __init__(self, k, tok, h, logp, frames, incs, lm_tok=None, lm_h=None):
        self.k, self.tok, self.h, self.logp, self.frames, self.incs = k, tok, h, logp, frames, incs
        self.lm_tok, self.lm_h = lm_tok, lm_h


def bias_beam_one(sd, h_enc, W, bias=None, lm=None, lm_weight=0.0, length_bonus=0.0, lm_bos=1, blank=M.NUL,
                  max_expansions=400):
    """h_enc [T, P_enc] fp32 of ONE utterance -> dict:
    ``B``            the final list B in its own order: dicts with tokens / frames / token_logp (lists) and logp
    ``expansions``   pops
    ``retractions``  popped hypotheses whose last token gave a pending bonus back (D < 0)
    ``trace``        {(frame, iteration in the frame): automaton state of the popped hypothesis, a tuple}
    More than ``max_expansions`` pops in one frame raise (a boost that pays for a token outright never stops)."""
    L = M.n_dec_layers(sd)
    H = sd["decoder.lstm.weight_hh_l0"].shape[1]
    zero = (torch.zeros(L, 1, H), torch.zeros(L, 1, H))
    V = sd["joint.joint.2.weight"].shape[0]
    B = [_Hyp([], M.BOS, zero, 0.0, [], [], lm_bos, lm.zero() if lm is not None else None)]
    n_expansions = retractions = 0
    trace = {}
    for t, x in enumerate(h_enc):
        A = B
        B = []
        it = 0
        while True:
            y_hat = max(A, key=lambda a: a.logp)
            A.remove(y_hat)
            pred, hidden = M.decoder_forward(sd, torch.tensor([[y_hat.tok]]), y_hat.h)
            logp = torch.log_softmax(M.joint_forward(sd, x[None, :], pred[:, 0])[0], dim=0)
            lm_hidden = None
            if lm is not None:
                lp_lm, lm_hidden = lm.forward(torch.tensor([[y_hat.lm_tok]]), y_hat.lm_h)
                lp_lm = lp_lm[0]
            n_expansions += 1
            if bias is not None:
                s = bias.state(y_hat.k)
                pend_s = bias.held_pend(s)[1]
                trace[(t, it)] = s
                if y_hat.k and bias.delta(y_hat.k[:-1], y_hat.k[-1]) < 0:
                    retractions += 1
            it += 1
            if it > max_expansions:
                raise RuntimeError("bias_beam_one: more than %d expansions in frame %d" % (max_expansions, t))
            for k in range(V):
                if k == blank:
                    B.append(_Hyp(y_hat.k, y_hat.tok, y_hat.h, y_hat.logp + float(logp[k]), y_hat.frames, y_hat.incs,
                                  y_hat.lm_tok, y_hat.lm_h))
                    continue
                lp = y_hat.logp + float(logp[k])
                if lm is not None:
                    lp = lp + (lm_weight * float(lp_lm[k]) + length_bonus)
                if bias is not None:
                    lp = lp + (bias.held_pend(bias.state(y_hat.k + [k]))[0] - pend_s)
                A.append(_Hyp(y_hat.k + [k], k, hidden, lp, y_hat.frames + [t], y_hat.incs + [lp - y_hat.logp], k,
                              lm_hidden))
            y_a = max(A, key=lambda a: a.logp)
            y_b = max(B, key=lambda a: a.logp)
            if len(B) >= W and y_b.logp >= y_a.logp:
                break
        B = B[:W]
    out = [dict(tokens=list(h.k), frames=list(h.frames), token_logp=list(h.incs), logp=h.logp) for h in B]
    return dict(B=out, expansions=n_expansions, retractions=retractions, trace=trace)


def bias_beam(sd, xs, xlen, W, bias=None, **kw):
    """xs [B, T0, I] -> (one ``bias_beam_one`` dict per utterance, total expansions)."""
    h_enc, _ = M.encoder_forward(sd, xs, None)
    Bn, T = h_enc.shape[0], h_enc.shape[1]
    lens = [T] * Bn if xlen is None else [int(v) for v in M.scale_length(T, xlen)]
    res = [bias_beam_one(sd, h_enc[b, :lens[b]], W, bias, **kw) for b in range(Bn)]
    return res, sum(r["expansions"] for r in res)


def best(res):
    """(tokens as int64 arrays, scores = -logp) of entry 0 per utterance, as ``beam_search_batch`` returns them."""
    return ([np.array(r["B"][0]["tokens"], dtype=np.int64) for r in res],
            np.array([-r["B"][0]["logp"] for r in res], dtype=np.float64))
