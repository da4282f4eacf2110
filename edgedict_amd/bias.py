"""Contextual biasing (phrase boosting) for the beam searches: a list of phrases, given at run time, that the search
should prefer - names, product words, commands - with no retraining.

``ContextGraph`` turns the list into a phrase automaton on the host (plain Python / numpy) and uploads it once per
device as a few small tables; the searches (``decode.beam_search_batch(..., bias=graph)`` and every other beam search,
offline, N-best and streaming) carry one automaton state per hypothesis beside the prediction network's ``(h, c)`` and
add one fp64 term per non-blank child inside the native search loop (csrc/decode.hip ``beam_pop_bias`` /
``beam_expand_bias`` and their detail / LM forms).

Semantics
---------
A phrase is a non-empty sequence of token ids in ``[0, V)`` without ``blank`` and ``BOS``, with a per-token boost
``beta >= 0`` (``boost`` for the whole list, ``phrase_boosts[i]`` for phrase i; a trie edge shared by several phrases
takes the largest).  The automaton is the phrases' trie (root 0) with Aho-Corasick failure links: the state after a
token sequence y is the longest suffix of y that is a path from the root, ``goto(s, k)`` the fully resolved transition.
For a node n entered over edge e from its parent p::

    held[n] = pend[p] + beta(e)
    pend[n] = 0 if a phrase ends at n (its bonus is banked and never taken back) else held[n]
    held[0] = pend[0] = 0

Consuming token k in state s moves to ``n = goto(s, k)`` and adds ``D(s, k) = held[n] - pend[s]`` (one fp64
subtraction of two table values): a partial match that breaks gives its bonus back, a completed phrase keeps it.

In the search a hypothesis carries the state BEFORE its last token (as it carries the prediction network's and the
LM's); popping y* with last token ``tok`` from carried state ``s0`` gives ``s = goto(s0, tok)`` (the root's token is BOS
or the stream's root token; BOS is in no phrase).  The blank child keeps ``base + lp_rnnt[blank]``; a non-blank child k
scores ``(base + lp_rnnt[k]) + D(s, k)``, with an LM ``((base + lp_rnnt[k]) + F) + D(s, k)`` with the fused term
``F = lm_weight * lp_lm[k] + length_bonus`` (fp64, in this order).  ``NBestResult.token_logp`` and ``logp`` include the
bias increments (the detail is the difference of pool scores, so nothing else changes).

The CTC prefix beam search (``decode.ctc_beam_search`` / ``loss.ctc_prefix_beam``, csrc/ctc_decode.hip) reads the same
tables: a prefix carries the state AFTER its last token and the total ``score(tokens)``, which enters its ranking and
its reported ``logp``; a frame's candidate list is cut before the bias is seen.

Not in scope
------------
* No output links: a phrase that occurs only INSIDE a longer partial match that then breaks is not credited.
* No end-of-utterance retraction: a bonus still pending when the audio ends stays in the score.
* The greedy search is not biased.
* ``prefix=True`` (the prefix-sum merge) with a bias list raises ``ValueError``, as it does with an LM.
* The kernels read only the tables below: the host-side automaton can be refined without touching them.

Device tables
-------------
A dense ``[S][V]`` transition table would be 128 MB at 4 k states x 4 k tokens.  Stored instead:
``root_next[V]`` int32 (``goto(0, k)``), ``held[S]`` / ``pend[S]`` fp64, and per state a CSR row (``row_ptr[S + 1]``)
of ``(exc_tok, exc_next)`` pairs sorted by token: the EXCEPTIONS, the tokens where ``goto(s, k) != goto(0, k)`` - at
most the children along s's failure chain.
"""
import ctypes

import numpy as np

from .tokenizer import BOS, NUL


class BeamBias(ctypes.Structure):
    """ctypes mirror of ``edgedict_beam_bias_t`` (include/edgedict_hip.h)."""
    _fields_ = [("S", ctypes.c_int), ("V", ctypes.c_int), ("n_exc", ctypes.c_int),
                ("root_next", ctypes.c_void_p), ("held", ctypes.c_void_p), ("pend", ctypes.c_void_p),
                ("row_ptr", ctypes.c_void_p), ("exc_tok", ctypes.c_void_p), ("exc_next", ctypes.c_void_p)]


class ContextGraph:
    """The phrase automaton of a bias list (module docstring).

    ``phrases``        sequence of token-id sequences; an empty LIST is allowed and means "no bias"
    ``boost``          per-token boost beta >= 0 of every phrase without one of its own
    ``vocab_size``     V of the transducer the graph is for
    ``phrase_boosts``  optional, one beta >= 0 (or None: ``boost``) per phrase
    """

    def __init__(self, phrases, boost, vocab_size, *, blank=NUL, bos=BOS, phrase_boosts=None):
        V = int(vocab_size)
        if V < 1:
            raise ValueError("ContextGraph: vocab_size must be >= 1")
        boost = float(boost)
        if not boost >= 0.0 or not np.isfinite(boost):
            raise ValueError("ContextGraph: boost must be a finite number >= 0 (got %r)" % boost)
        phrases = [[int(k) for k in p] for p in phrases]
        if phrase_boosts is None:
            betas = [boost] * len(phrases)
        else:
            if len(phrase_boosts) != len(phrases):
                raise ValueError("ContextGraph: %d phrase_boosts for %d phrases" % (len(phrase_boosts), len(phrases)))
            betas = [boost if x is None else float(x) for x in phrase_boosts]
        for i, (p, beta) in enumerate(zip(phrases, betas)):
            if not p:
                raise ValueError("ContextGraph: phrase %d is empty" % i)
            if not beta >= 0.0 or not np.isfinite(beta):
                raise ValueError("ContextGraph: phrase %d has boost %r (must be finite and >= 0)" % (i, beta))
            for k in p:
                if not 0 <= k < V:
                    raise ValueError("ContextGraph: phrase %d has token %d outside [0, %d)" % (i, k, V))
                if k == blank or k == bos:
                    raise ValueError("ContextGraph: phrase %d contains the %s token %d"
                                     % (i, "blank" if k == blank else "BOS", k))
        self.V, self.blank, self.bos = V, int(blank), int(bos)
        self.phrases, self.boosts = phrases, betas

        # the trie; nodes are numbered in creation order, so a parent precedes its children
        children, parent, edge_beta, ends = [{}], [-1], [0.0], [False]
        for p, beta in zip(phrases, betas):
            s = 0
            for k in p:
                n = children[s].get(k)
                if n is None:
                    n = len(children)
                    children[s][k] = n
                    children.append({})
                    parent.append(s)
                    edge_beta.append(beta)
                    ends.append(False)
                elif beta > edge_beta[n]:
                    edge_beta[n] = beta
                s = n
            ends[s] = True
        S = len(children)
        held, pend = [0.0] * S, [0.0] * S
        for n in range(1, S):
            held[n] = pend[parent[n]] + edge_beta[n]
            pend[n] = 0.0 if ends[n] else held[n]

        # failure links breadth first; the exceptions of s are those of fail(s) overridden by s's own children
        root_next = np.zeros(V, dtype=np.int32)
        for k, n in children[0].items():
            root_next[k] = n
        fail = [0] * S
        rows = [None] * S
        rows[0] = {}
        queue = list(children[0].values())
        for n in queue:
            rows[n] = dict(children[n])
        head = 0
        while head < len(queue):
            s = queue[head]
            head += 1
            for k, n in children[s].items():
                f = fail[s]
                # goto(fail(s), k): fail(s) is shallower than s, its row is final
                fail[n] = rows[f].get(k, int(root_next[k])) if s != 0 else 0
                row = dict(rows[fail[n]])
                row.update(children[n])
                rows[n] = row
                queue.append(n)
        row_ptr = np.zeros(S + 1, dtype=np.int32)
        toks, nexts = [], []
        for s in range(S):
            for k in sorted(rows[s]):
                if rows[s][k] != root_next[k]:
                    toks.append(k)
                    nexts.append(rows[s][k])
            row_ptr[s + 1] = len(toks)
        self.n_states = S
        self.held = np.asarray(held, dtype=np.float64)
        self.pend = np.asarray(pend, dtype=np.float64)
        self.root_next = root_next
        self.row_ptr = row_ptr
        self.exc_tok = np.asarray(toks, dtype=np.int32)
        self.exc_next = np.asarray(nexts, dtype=np.int32)
        self._device = {}

    @classmethod
    def from_text(cls, texts, tokenizer, boost, vocab_size=None, **kw):
        """Phrases given as text, encoded with the project's tokenizer object (``stream.StreamDecoder``'s: anything
        with ``encode(text)`` returning ids or an object with ``.ids``, possibly wrapped as ``.tokenizer``; its
        ``vocab_size`` is the default V)."""
        inner = getattr(tokenizer, "tokenizer", tokenizer)
        if vocab_size is None:
            vocab_size = getattr(tokenizer, "vocab_size", None)
            if vocab_size is None:
                raise ValueError("ContextGraph.from_text: the tokenizer has no vocab_size, pass one")
        phrases = []
        for text in texts:
            enc = inner.encode(text)
            phrases.append([int(k) for k in getattr(enc, "ids", enc)])
        return cls(phrases, boost, vocab_size, **kw)

    def __len__(self):
        return len(self.phrases)

    @property
    def empty(self):
        """No phrase: the searches run their plain path."""
        return not self.phrases

    # ---- the automaton, as the kernels read it (root_next plus the exceptions)
    def goto(self, s, k):
        s, k = int(s), int(k)
        if not 0 <= s < self.n_states or not 0 <= k < self.V:
            raise ValueError("ContextGraph.goto: state %d / token %d out of range" % (s, k))
        lo, hi = int(self.row_ptr[s]), int(self.row_ptr[s + 1])
        i = lo + int(np.searchsorted(self.exc_tok[lo:hi], k))
        if i < hi and self.exc_tok[i] == k:
            return int(self.exc_next[i])
        return int(self.root_next[k])

    def delta(self, s, k):
        """D(s, k) = held[goto(s, k)] - pend[s]"""
        return float(self.held[self.goto(s, k)]) - float(self.pend[int(s)])

    def score(self, tokens):
        """The total bias of a token sequence read from the root: the sum of its increments, in order."""
        s, total = 0, 0.0
        for k in tokens:
            total += self.delta(s, k)
            s = self.goto(s, k)
        return total

    # ---- device side
    def tables(self, device):
        """The device tables (uploaded once per device): dict of tensors and the ``BeamBias`` struct."""
        import torch
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        hit = self._device.get(device)
        if hit is not None:
            return hit
        one = lambda a: torch.from_numpy(a if a.size else np.zeros(1, dtype=a.dtype)).to(device)
        t = dict(root_next=one(self.root_next), held=one(self.held), pend=one(self.pend), row_ptr=one(self.row_ptr),
                 exc_tok=one(self.exc_tok), exc_next=one(self.exc_next))
        s = BeamBias()
        s.S, s.V, s.n_exc = self.n_states, self.V, int(self.exc_tok.size)
        for name, ten in t.items():
            setattr(s, name, ten.data_ptr())
        t["struct"] = s
        self._device[device] = t
        return t

    def ref(self, device):
        """``const edgedict_beam_bias_t*`` for a native call on ``device``."""
        return ctypes.byref(self.tables(device)["struct"])


def check_bias_args(bias, V=None, prefix=False):
    """The argument rules of every beam search that takes a bias list (raised before anything is launched)."""
    if bias is None:
        return
    if not isinstance(bias, ContextGraph):
        raise ValueError("bias must be an edgedict_amd.bias.ContextGraph (got %s)" % type(bias).__name__)
    if bias.empty:
        return
    if prefix:
        raise ValueError("prefix=True (the prefix-sum merge) is not supported with a bias list")
    if V is not None and bias.V != V:
        raise ValueError("the bias list's vocabulary (vocab_size = %d) differs from the transducer's (V = %d)"
                         % (bias.V, V))


def active(bias):
    """``bias`` if the searches have to carry it, None for no list or an empty one (the plain path)."""
    return None if bias is None or bias.empty else bias
