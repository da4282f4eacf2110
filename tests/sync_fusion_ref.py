"""ORACLE (test infrastructure only): the frame-synchronous beam search with LM shallow fusion and contextual biasing
(csrc/decode_sync.hip, the *_fused kernels; decode.sync_beam_search*(lm=, bias=)) restated in Python floats:
``sync_beam_ref.search_core`` generalised by a per-hypothesis LM and a brute-force phrase automaton, and the streaming
form on ``sync_stream_ref.StreamSearch``'s tree and commit rule.  The model arithmetic is oracle/models_ref.py's, the
LM's is ``test_lm_fusion_gpu.RefLM``'s and the automaton's is ``bias_ref.BruteBias``'s; none of it is restated here.

Per utterance, on frame t, hypothesis i in beam order has score logp_i, sequence y_i, an LM state and the automaton
state after y_i:
  * the LM state is carried as the prediction network's: the state from BEFORE the hypothesis' last token.  Every frame
    every hypothesis steps the LM on its last token - the empty sequence on ``lm_bos`` from a zero state - which gives
    lp_lm (fp32 log-softmax);
  * D(i, k) = held(state(y_i + [k])) - pend(state(y_i))     (``BruteBias.delta``);
  * blank scores ``logp_i + lp_i[blank]``; a non-blank k scores
    ``((logp_i + lp_i[k]) + (lm_weight * lp_lm_i[k] + length_bonus)) + D(i, k)``, Python floats in this order; a term
    is absent when its feature is;
  * selection (score descending, then i, then k), folding and the final ranking are ``search_core``'s; a token child
    takes the LM state after i's last token, a blank child keeps its parent's, and the two partners of a fold hold the
    same sequence, so the same LM and automaton state;
  * ``token_logp`` stays lp_i[k] on the node's creation frame; nothing is settled at the end of an utterance.
``info`` is ``search_core``'s (margin, rank_gap, merges) plus ``retractions``: kept token children with D < 0, a
partial match that broke and gave its pending bonus back."""
import math

import torch

import sync_beam_ref as S
import sync_stream_ref as SS
from oracle import models_ref as M


class Fusion:
    """What the fused score adds: ``lm`` (``zero()`` / ``forward(tokens, hidden) -> (log-probs [1, V], hidden)``, or
    None) with its weight, bonus and root token, and ``bias`` (a ``BruteBias`` or None)."""

    def __init__(self, lm=None, lm_weight=0.0, length_bonus=0.0, lm_bos=1, bias=None):
        self.lm, self.lm_weight, self.length_bonus, self.lm_bos, self.bias = lm, lm_weight, length_bonus, lm_bos, bias
        self._delta = {}
        self.visited = set()        # (automaton state as a trie path, k) of every candidate scored with a list

    def root(self):
        """(LM token, LM state) of the empty sequence."""
        return self.lm_bos, (self.lm.zero() if self.lm is not None else None)

    def lm_step(self, tok, state):
        if self.lm is None:
            return None, None
        lp, new = self.lm.forward(torch.tensor([[tok]]), state)
        return lp[0].tolist(), new

    def delta(self, seq, k):
        """``BruteBias.delta(seq, k)``.  The increment depends on ``seq`` through its automaton state alone (the longest
        suffix that is a trie path), so it is computed once per (state, k) - from the state's own path, whose state it
        is."""
        s = self.bias.state(seq)
        d = self._delta.get((s, k))
        if d is None:
            d = self._delta[(s, k)] = self.bias.delta(s, k)
        self.visited.add((s, k))
        return d

    def candidates(self, rows, t, expand, blank):
        """Every candidate of the frame as (score, i, k, D), and per row (lp, state after, LM state after)."""
        cands, steps = [], []
        for i, h in enumerate(rows):
            lp, new_state = expand(t, h.tok, h.state)
            lp_lm, lm_new = self.lm_step(h.lm_tok, h.lm_state)
            steps.append((lp, new_state, lm_new))
            for k in range(len(lp)):
                score, d = h.logp + float(lp[k]), 0.0
                if k != blank:
                    if self.lm is not None:
                        score = score + (self.lm_weight * float(lp_lm[k]) + self.length_bonus)
                    if self.bias is not None:
                        d = self.delta(h.seq, k)
                        score = score + d
                cands.append((score, i, k, d))
        cands.sort(key=lambda c: (-c[0], c[1], c[2]))
        return cands, steps


class _Hyp:
    __slots__ = ("seq", "logp", "tok", "state", "frames", "tlp", "lm_tok", "lm_state")

    def __init__(self, seq, logp, tok, state, frames, tlp, lm_tok, lm_state):
        self.seq, self.logp, self.tok, self.state, self.frames, self.tlp = seq, logp, tok, state, frames, tlp
        self.lm_tok, self.lm_state = lm_tok, lm_state


def search_core(T, W, expand, root_state, root_tok, fusion, blank=M.NUL):
    """``sync_beam_ref.search_core`` on the fused score.  Returns ``(beam, info)``, info with ``retractions`` added."""
    beam = [_Hyp((), 0.0, root_tok, root_state, (), (), *fusion.root())]
    margin, merges, retractions = float("inf"), 0, 0
    for t in range(T):
        cands, steps = fusion.candidates(beam, t, expand, blank)
        if len(cands) > W:
            margin = min(margin, cands[W - 1][0] - cands[W][0])
        new, place = [], {}
        for score, i, k, d in cands[:W]:
            h = beam[i]
            if k == blank:
                child = _Hyp(h.seq, score, h.tok, h.state, h.frames, h.tlp, h.lm_tok, h.lm_state)
            else:
                retractions += d < 0
                child = _Hyp(h.seq + (k,), score, k, steps[i][1], h.frames + (t,), h.tlp + (float(steps[i][0][k]),), k,
                             steps[i][2])
            j = place.get(child.seq)
            if j is None:
                place[child.seq] = len(new)
                new.append(child)
                continue
            merges += 1
            old = new[j]
            mx, mn = max(old.logp, child.logp), min(old.logp, child.logp)
            keep = child if k == blank else old      # the one that did not append on this frame: the older node
            new[j] = _Hyp(keep.seq, mx + math.log1p(math.exp(mn - mx)), keep.tok, keep.state, keep.frames, keep.tlp,
                          keep.lm_tok, keep.lm_state)
        beam = new
    order = sorted(range(len(beam)), key=lambda j: -beam[j].logp)      # stable: ties keep beam order
    ranked = [beam[j] for j in order]
    gaps = [a.logp - b.logp for a, b in zip(ranked, ranked[1:])]
    out = [dict(tokens=list(h.seq), frames=list(h.frames), token_logp=list(h.tlp), logp=h.logp) for h in ranked]
    return out, dict(margin=margin, rank_gap=min(gaps) if gaps else float("inf"), merges=merges,
                     retractions=int(retractions))


def model_expand(sd, h_enc):
    """(expand, zero state) of the transducer ``sd`` over ONE utterance's encoder output, as ``sync_beam_ref.search_one``
    builds them."""
    L = M.n_dec_layers(sd)
    H = sd["decoder.lstm.weight_hh_l0"].shape[1]
    zero = (torch.zeros(L, 1, H), torch.zeros(L, 1, H))

    def expand(t, tok, state):
        pred, new_state = M.decoder_forward(sd, torch.tensor([[tok]]), state)
        lp = torch.log_softmax(M.joint_forward(sd, h_enc[t][None, :], pred[:, 0])[0], dim=0)
        return lp.tolist(), new_state

    return expand, zero


def search_one(sd, h_enc, W, fusion, blank=M.NUL):
    expand, zero = model_expand(sd, h_enc)
    return search_core(h_enc.shape[0], W, expand, zero, M.BOS, fusion, blank)


def search(sd, xs, xlen, W, fusion):
    """xs [B, T0, I] -> (list of B ranked lists, list of B info dicts); ``fusion`` is shared (its LM and list are
    read-only, ``visited`` accumulates)."""
    h_enc, lens = S.encode(sd, xs, xlen)
    res, infos = [], []
    for b in range(h_enc.shape[0]):
        r, info = search_one(sd, h_enc[b, :lens[b]], W, fusion)
        res.append(r)
        infos.append(info)
    return res, infos


class _Row(SS._Row):
    __slots__ = ("lm_tok", "lm_state")

    def __init__(self, seq, logp, tok, state, node, lm_tok, lm_state):
        super().__init__(seq, logp, tok, state, node)
        self.lm_tok, self.lm_state = lm_tok, lm_state


class StreamSearch(SS.StreamSearch):
    """``sync_stream_ref.StreamSearch`` on the fused score: its tree, its commit rule and its read-out, with the frame
    restated for rows that carry an LM token and state.  The automaton state is the sequence's, committed tokens
    included, and the LM's root token is ``lm_bos`` for the empty sequence only."""

    def __init__(self, W, expand, root_state, root_tok, fusion, blank=0):
        super().__init__(W, expand, root_state, root_tok, blank)
        self.fusion = fusion
        self.rows = [_Row((), 0.0, root_tok, root_state, -1, *fusion.root())]
        self.retractions = 0

    def _frame(self, t):
        W, blank = self.W, self.blank
        cands, steps = self.fusion.candidates(self.rows, t, self.expand, blank)
        if len(cands) > W:
            self.margin = min(self.margin, cands[W - 1][0] - cands[W][0])
        new, place = [], {}
        for score, i, k, d in cands[:W]:
            h = self.rows[i]
            if k == blank:
                child = _Row(h.seq, score, h.tok, h.state, h.node, h.lm_tok, h.lm_state)
            else:
                self.retractions += d < 0
                child = _Row(h.seq + (k,), score, k, steps[i][1], ("new", h.node, k, float(steps[i][0][k])), k,
                             steps[i][2])
            j = place.get(child.seq)
            if j is None:
                place[child.seq] = len(new)
                new.append(child)
                continue
            self.merges += 1
            old = new[j]
            mx, mn = max(old.logp, child.logp), min(old.logp, child.logp)
            keep = child if k == blank else old
            new[j] = _Row(keep.seq, mx + math.log1p(math.exp(mn - mx)), keep.tok, keep.state, keep.node, keep.lm_tok,
                          keep.lm_state)
        for h in new:               # the surviving token children get their nodes, in beam order
            if isinstance(h.node, tuple):
                _, parent, k, lp = h.node
                self.tree[self.next_id] = (parent, k, t, lp)
                h.node = self.next_id
                self.next_id += 1
        self.rows = new
