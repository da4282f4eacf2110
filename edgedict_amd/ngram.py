"""Back-off n-gram language model over the transducer's token ids: the engine's second kind of LM (the first is the
LSTM ``lm.LMModel``), held in a few device tables and cheap enough to be read inside a search kernel.

``NGramLM`` builds the model on the host (plain Python / numpy) from an ARPA file (``from_arpa``) or from token lists
(``train``) and uploads it once per device, as ``bias.ContextGraph`` does its automaton.  The CTC prefix beam search
reads it (``loss.ctc_prefix_beam(..., lm=, lm_weight=, length_bonus=)``, csrc/ctc_decode.hip), and so does the
frame-synchronous RNN-T search (``decode.sync_beam_search*(lm=)`` and its streaming forms, csrc/decode_sync.hip: a
row's image of ``step(s, .)`` / ``next(s, .)`` in LDS, vocabularies up to ``SYNC_NGRAM_MAX_V``); csrc/ngram.hip scores
sentences (``score_nbest`` / ``score_lists``, ``decode.lm_rescore``) and writes dense per-state rows (``logprobs``).

Symbols and states
------------------
The symbols are the ids ``0 .. V-1`` plus ``eos = V``, which exists in the tables only.  ``<s>`` is the ``BOS`` id and
occurs only inside contexts.  ``blank`` is no symbol: its unigram entry is 0.0 and is never read.  A STATE is a context
of ``0 .. order-1`` tokens; state 0 is the empty context, the set of states is closed under dropping the oldest token,
and ``start`` is the state of the context ``(BOS,)`` (0 if the model has none).

Tables (natural-log float64)
----------------------------
``uni_lp[V+1]`` / ``uni_next[V+1]``: the unigrams and the state after them; ``row_ptr[S+1]``: per state a row of
``(arc_tok, arc_lp, arc_next)`` sorted by token (state 0: empty, its row is ``uni_*``); ``fail[S]``: the state of the
context without its oldest token; ``backoff[S]``.  ``arc_next`` / ``uni_next`` name the longest suffix of
context + token that is a state.

The score, in exactly this order of float64 additions::

    step(s, k):  acc = 0.0
                 repeat:  if s == 0:       return acc + uni_lp[k], uni_next[k]
                          if k in row(s):  return acc + arc_lp, arc_next
                          acc = acc + backoff[s];  s = fail[s]

The kernels add in the same order, so a sentence's score on the device is the host's bit for bit.

ARPA values are kept as the file's log10 numbers and multiplied by ``ln 10`` once, in float64: reading what ``to_arpa``
wrote gives identical tables.
"""
import ctypes
import math
import os

import numpy as np

from .tokenizer import BOS, NUL

LN10 = math.log(10.0)
MAX_ORDER = 6
# the largest vocabulary the frame-synchronous search takes an n-gram for: a row's image (12 bytes a symbol) has to fit
# the 64 KiB of LDS a launch gets (SB_NGRAM_MAX_V of csrc/decode_sync.hip)
SYNC_NGRAM_MAX_V = 5376


class NGramStruct(ctypes.Structure):
    """ctypes mirror of ``edgedict_ngram_lm_t`` (include/edgedict_hip.h)."""
    _fields_ = [("V", ctypes.c_int), ("order", ctypes.c_int), ("S", ctypes.c_int), ("n_arcs", ctypes.c_int),
                ("start", ctypes.c_int), ("blank", ctypes.c_int),
                ("uni_lp", ctypes.c_void_p), ("uni_next", ctypes.c_void_p), ("row_ptr", ctypes.c_void_p),
                ("fail", ctypes.c_void_p), ("backoff", ctypes.c_void_p), ("arc_tok", ctypes.c_void_p),
                ("arc_lp", ctypes.c_void_p), ("arc_next", ctypes.c_void_p),
                ("weight", ctypes.c_double), ("length_bonus", ctypes.c_double)]


class CtcBeamOpts(ctypes.Structure):
    """ctypes mirror of ``edgedict_ctc_beam_opts_t``."""
    _fields_ = [("bias", ctypes.c_void_p), ("ngram", ctypes.c_void_p)]


_TABLES = ("uni_lp", "uni_next", "row_ptr", "fail", "backoff", "arc_tok", "arc_lp", "arc_next")


class NGramLM:
    """A back-off n-gram (module docstring).  Build one with ``from_arpa`` or ``train``."""

    def __init__(self, vocab_size, order, uni10, arcs10, backoff10, *, blank=NUL, bos=BOS, words=None, unk10=None,
                 explicit=None):
        """``uni10`` [V + 1] log10 unigrams (blank: 0), ``arcs10`` {context tuple: {token: log10 p}} for contexts of
        1 .. order - 1 tokens, ``backoff10`` {context tuple: log10 back-off weight}.  Not meant to be called directly."""
        V, order = int(vocab_size), int(order)
        if V < 2:
            raise ValueError("NGramLM: vocab_size must be >= 2")
        if not 1 <= order <= MAX_ORDER:
            raise ValueError("NGramLM: order %d outside [1, %d]" % (order, MAX_ORDER))
        self.V, self.order, self.blank, self.bos, self.eos = V, order, int(blank), int(bos), V
        self.words = dict(words) if words is not None else {k: str(k) for k in range(V)}
        self.unk10 = unk10
        self.explicit = set(range(V + 1)) - {self.blank} if explicit is None else set(explicit)
        uni10 = np.array(uni10, dtype=np.float64)
        uni10[self.blank] = 0.0
        if not np.isfinite(uni10).all():
            raise ValueError("NGramLM: every unigram must be finite")
        arcs10 = {tuple(h): dict(row) for h, row in arcs10.items() if row and 1 <= len(h) < order}
        backoff10 = {tuple(h): float(v) for h, v in backoff10.items() if 1 <= len(h) < order}
        # the states: the contexts with arcs or with a back-off weight that matters, closed under dropping the oldest
        ctxs = set(arcs10) | {h for h, v in backoff10.items() if v != 0.0}
        for h in list(ctxs):
            while len(h) > 1:
                h = h[1:]
                ctxs.add(h)
        ctxs = [()] + sorted(ctxs, key=lambda h: (len(h), h))
        self.contexts = ctxs
        index = {h: s for s, h in enumerate(ctxs)}
        self._index = index
        S = len(ctxs)

        def longest(h):
            h = tuple(h)[-(order - 1):] if order > 1 else ()
            while h not in index:
                h = h[1:]
            return index[h]

        self.uni10 = uni10
        self.uni_lp = uni10 * LN10
        self.uni_lp[self.blank] = 0.0
        self.uni_next = np.array([0 if k in (self.eos, self.blank) else longest((k,)) for k in range(V + 1)],
                                 dtype=np.int32)
        self.fail = np.array([0] + [index[h[1:]] for h in ctxs[1:]], dtype=np.int32)
        self.backoff10 = np.array([0.0] + [backoff10.get(h, 0.0) for h in ctxs[1:]], dtype=np.float64)
        self.backoff = self.backoff10 * LN10
        row_ptr = np.zeros(S + 1, dtype=np.int32)
        toks, lps, nexts = [], [], []
        for s, h in enumerate(ctxs):
            row = arcs10.get(h, {}) if s else {}
            for k in sorted(row):
                toks.append(k)
                lps.append(row[k])
                nexts.append(0 if k == self.eos else longest(h + (k,)))
            row_ptr[s + 1] = len(toks)
        self.row_ptr = row_ptr
        self.arc_tok = np.array(toks, dtype=np.int32)
        self.arc10 = np.array(lps, dtype=np.float64)
        self.arc_lp = self.arc10 * LN10
        self.arc_next = np.array(nexts, dtype=np.int32)
        if not (np.isfinite(self.arc_lp).all() and np.isfinite(self.backoff).all()):
            raise ValueError("NGramLM: every n-gram value and back-off weight must be finite")
        self.n_states, self.n_arcs = S, int(self.arc_tok.size)
        self.start = index.get((self.bos,), 0)
        self._device = {}
        self._rows = None

    # ------------------------------------------------------------------------------------------------ construction
    @classmethod
    def from_arpa(cls, path_or_text, symbols=None, vocab_size=None, unk_logp=None, *, blank=NUL, bos=BOS):
        """Read an ARPA file (a path, or the text itself).  ``symbols`` maps the file's words to ids in ``[0, V)``
        (default: a word is its id in decimal); ``<s>`` is the BOS id inside contexts, ``</s>`` is ``eos``.  An id
        without a unigram takes the file's ``<unk>`` value, else ``unk_logp`` (natural log); with neither:
        ``ValueError``.  N-grams that predict ``<s>``, that have ``</s>`` in their context or that contain ``<unk>``
        are dropped."""
        if vocab_size is None:
            raise ValueError("NGramLM.from_arpa: vocab_size is required")
        V = int(vocab_size)
        text = path_or_text
        if not isinstance(text, str) or ("\n" not in text and "\\data\\" not in text):
            with open(os.fspath(path_or_text)) as f:
                text = f.read()
        if symbols is None:
            symbols = {str(k): k for k in range(V)}
        eos = V

        def ident(word, n):
            if word == "<s>":
                return bos
            if word == "</s>":
                return eos
            if word == "<unk>":
                return None
            if word not in symbols:
                raise ValueError("NGramLM.from_arpa: the word %r of a %d-gram is not in `symbols`" % (word, n))
            k = int(symbols[word])
            if not 0 <= k < V or k == blank or k == bos:
                raise ValueError("NGramLM.from_arpa: the word %r maps to %d (outside [0, %d), the blank or BOS)"
                                 % (word, k, V))
            return k

        section, order = 0, 0
        uni10 = {}
        unk10 = None
        arcs10, backoff10 = {}, {}
        for raw in text.splitlines():
            line = raw.strip()
            if not line or line == "\\data\\" or line.startswith("ngram "):
                continue
            if line == "\\end\\":
                break
            if line.startswith("\\") and line.endswith("-grams:"):
                section = int(line[1:-len("-grams:")])
                order = max(order, section)
                continue
            if section == 0:
                continue
            f = line.split()
            if len(f) not in (section + 1, section + 2):
                raise ValueError("NGramLM.from_arpa: malformed %d-gram line %r" % (section, raw))
            lp = float(f[0])
            gram = [ident(w, section) for w in f[1:1 + section]]
            bo = float(f[1 + section]) if len(f) == section + 2 else 0.0
            if section == 1:
                if f[1] == "<unk>":
                    unk10 = lp
                elif f[1] == "<s>":
                    backoff10[(bos,)] = bo
                else:
                    uni10[gram[0]] = lp
                    if gram[0] != eos:
                        backoff10[(gram[0],)] = bo
                continue
            if None in gram or gram[-1] == bos or eos in gram[:-1] or bos in gram[1:]:
                continue
            h = tuple(gram[:-1])
            arcs10.setdefault(h, {})[gram[-1]] = lp
            if gram[-1] != eos:
                backoff10[tuple(gram)] = bo
        if order < 1:
            raise ValueError("NGramLM.from_arpa: no n-gram section found")
        if unk10 is None and unk_logp is not None:
            unk10 = float(unk_logp) / LN10
        full = np.zeros(V + 1, dtype=np.float64)
        for k in range(V + 1):
            if k == blank:
                continue
            if k in uni10:
                full[k] = uni10[k]
            elif unk10 is not None:
                full[k] = unk10
            else:
                raise ValueError("NGramLM.from_arpa: id %d has no unigram and there is neither <unk> nor unk_logp" % k)
        words = {int(k): w for w, k in symbols.items()}
        return cls(V, order, full, arcs10, backoff10, blank=blank, bos=bos, words=words, unk10=unk10,
                   explicit=set(uni10))

    @classmethod
    def train(cls, token_lists, order, vocab_size, discount=0.75, *, blank=NUL, bos=BOS):
        """Estimate a model from token-id lists: interpolated absolute discounting stored in back-off form.  With
        ``c`` the counts of a sentence read as ``BOS t_1 .. t_n eos``::

            p(w | h) = (c(h w) - D) / c(h) + bo(h) p(w | h')     for c(h w) > 0      (the explicit arcs)
            p(w | h) =                       bo(h) p(w | h')     otherwise
            bo(h) = D N1+(h .) / c(h),   h' = h without its oldest token
            p(w)  = (c(w) + 1) / (N + V)   over the V - 1 non-blank ids and eos (add-one)"""
        V, order, D = int(vocab_size), int(order), float(discount)
        if not 1 <= order <= MAX_ORDER:
            raise ValueError("NGramLM.train: order %d outside [1, %d]" % (order, MAX_ORDER))
        if not 0.0 < D < 1.0:
            raise ValueError("NGramLM.train: discount must lie in (0, 1)")
        eos = V
        counts = {}
        for sent in token_lists:
            sent = [int(k) for k in sent]
            for k in sent:
                if not 0 <= k < V or k == blank or k == bos:
                    raise ValueError("NGramLM.train: token %d outside [0, %d), the blank or BOS" % (k, V))
            seq = [bos] + sent + [eos]
            for i in range(1, len(seq)):
                for n in range(order):
                    if i - n < 0:
                        break
                    row = counts.setdefault(tuple(seq[i - n:i]), {})
                    row[seq[i]] = row.get(seq[i], 0) + 1
        uni_c = counts.get((), {})
        N = sum(uni_c.values())
        p_uni = np.zeros(V + 1, dtype=np.float64)
        for k in range(V + 1):
            if k != blank:
                p_uni[k] = (uni_c.get(k, 0) + 1.0) / (N + V)
        total = {h: sum(row.values()) for h, row in counts.items()}
        bo = {h: D * len(row) / total[h] for h, row in counts.items() if h}
        explicit = {}

        def prob(h, w):
            if not h:
                return p_uni[w]
            if h not in counts:
                return prob(h[1:], w)
            hit = explicit[h].get(w)
            return hit if hit is not None else bo[h] * prob(h[1:], w)

        for h in sorted((h for h in counts if h), key=len):
            explicit[h] = {w: (c - D) / total[h] + bo[h] * prob(h[1:], w) for w, c in counts[h].items()}
        with np.errstate(divide="ignore"):
            uni10 = np.log10(p_uni)
        arcs10 = {h: {w: math.log10(p) for w, p in row.items()} for h, row in explicit.items()}
        backoff10 = {h: math.log10(v) for h, v in bo.items()}
        return cls(V, order, uni10, arcs10, backoff10, blank=blank, bos=bos)

    def to_arpa(self):
        """The model as ARPA text (log10 values with 17 significant digits: ``from_arpa`` gives the same tables back)."""
        word = lambda k: "<s>" if k == self.bos else "</s>" if k == self.eos else self.words[k]
        num = lambda x: repr(float(x))
        sections = [[] for _ in range(self.order)]
        bo_start = self.backoff10[self._index[(self.bos,)]] if (self.bos,) in self._index else 0.0
        sections[0].append("-99\t<s>\t" + num(bo_start))
        # the BOS id as a PREDICTED symbol has no word of its own (<s> is the context): its unigram travels as <unk>
        unk10 = self.unk10 if self.unk10 is not None else (self.uni10[self.bos] if self.bos in self.explicit else None)
        if unk10 is not None:
            sections[0].append(num(unk10) + "\t<unk>")
        for k in sorted(self.explicit):
            if k == self.blank or k == self.bos:
                continue
            line = num(self.uni10[k]) + "\t" + word(k)
            s = self._index.get((k,))
            if s is not None and k != self.eos and self.backoff10[s] != 0.0:
                line += "\t" + num(self.backoff10[s])
            sections[0].append(line)
        for s, h in enumerate(self.contexts):
            for a in range(int(self.row_ptr[s]), int(self.row_ptr[s + 1])):
                k = int(self.arc_tok[a])
                line = num(self.arc10[a]) + "\t" + " ".join(word(t) for t in h + (k,))
                n = self._index.get(h + (k,))
                if n is not None and self.backoff10[n] != 0.0:
                    line += "\t" + num(self.backoff10[n])
                sections[len(h)].append(line)
        out = ["\\data\\"] + ["ngram %d=%d" % (n + 1, len(sec)) for n, sec in enumerate(sections)] + [""]
        for n, sec in enumerate(sections):
            out += ["\\%d-grams:" % (n + 1)] + sec + [""]
        return "\n".join(out + ["\\end\\", ""])

    # ------------------------------------------------------------------------------------------------ the host score
    def _plain(self):
        # Python lists and per-state dicts: the restatement is called millions of times by the test oracle
        if self._rows is None:
            rows = [{} for _ in range(self.n_states)]
            for s in range(self.n_states):
                for a in range(int(self.row_ptr[s]), int(self.row_ptr[s + 1])):
                    rows[s][int(self.arc_tok[a])] = (float(self.arc_lp[a]), int(self.arc_next[a]))
            self._rows = (rows, self.uni_lp.tolist(), self.uni_next.tolist(), self.backoff.tolist(), self.fail.tolist())
        return self._rows

    def step(self, s, k):
        """``(log p(k | state s), next state)``: the module docstring's loop.  ``k`` in ``[0, V]`` (``V`` is eos)."""
        s, k = int(s), int(k)
        if not 0 <= s < self.n_states or not 0 <= k <= self.V:
            raise ValueError("NGramLM.step: state %d / token %d out of range" % (s, k))
        rows, uni_lp, uni_next, backoff, fail = self._plain()
        acc = 0.0
        while True:
            if s == 0:
                return acc + uni_lp[k], uni_next[k]
            hit = rows[s].get(k)
            if hit is not None:
                return acc + hit[0], hit[1]
            acc = acc + backoff[s]
            s = fail[s]

    def score(self, tokens, bos=True, eos=False):
        """The log-probability of a token sequence: the float64 sum of its steps in order from ``start`` (state 0 with
        ``bos=False``), then the ``eos`` step if asked.  A token outside ``[0, V)`` or the blank gives ``-inf``."""
        s = self.start if bos else 0
        total = 0.0
        for k in tokens:
            k = int(k)
            if not 0 <= k < self.V or k == self.blank:
                return -np.inf
            l, s = self.step(s, k)
            total = total + l
        if eos:
            total = total + self.step(s, self.eos)[0]
        return total

    # ------------------------------------------------------------------------------------------------ device side
    def tables(self, device):
        """The device tables (uploaded once per device): dict of tensors and the ``NGramStruct`` with weight 0."""
        import torch
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        hit = self._device.get(device)
        if hit is not None:
            return hit
        one = lambda a: torch.from_numpy(a if a.size else np.zeros(1, dtype=a.dtype)).to(device)
        t = {name: one(getattr(self, name)) for name in _TABLES}
        s = NGramStruct()
        s.V, s.order, s.S, s.n_arcs, s.start, s.blank = self.V, self.order, self.n_states, self.n_arcs, self.start, self.blank
        for name in _TABLES:
            setattr(s, name, t[name].data_ptr())
        s.weight, s.length_bonus = 0.0, 0.0
        t["struct"] = s
        self._device[device] = t
        return t

    def struct(self, device, weight=0.0, length_bonus=0.0):
        """An ``NGramStruct`` over the cached tables with the given fusion weight and per-token bonus."""
        s = NGramStruct()
        ctypes.pointer(s)[0] = self.tables(device)["struct"]
        s.weight, s.length_bonus = float(weight), float(length_bonus)
        return s

    def ref(self, device, weight=0.0, length_bonus=0.0):
        """``const edgedict_ngram_lm_t*`` for a native call on ``device``."""
        return ctypes.byref(self.struct(device, weight, length_bonus))

    def logprobs(self, states, return_next=False):
        """Dense rows: ``states`` int32 ``[R]`` (device) -> float32 ``[R, V]`` with ``lp[r, k] = float32(step(states[r],
        k))`` and 0 in the blank column - the ``lp_lm`` row format of the RNN-T searches.  ``return_next=True`` adds the
        int32 ``[R, V]`` next states (the blank column: the state itself)."""
        import torch
        from . import _lib
        if states.dtype != torch.int32 or states.dim() != 1 or not states.is_contiguous():
            raise ValueError("NGramLM.logprobs: states must be a contiguous int32 [R] tensor")
        _lib.require_cuda(states)
        R = states.shape[0]
        lp = torch.empty(R, self.V, dtype=torch.float32, device=states.device)
        nxt = torch.empty(R, self.V, dtype=torch.int32, device=states.device) if return_next else None
        if R:
            _lib.call("ngram_logprobs", self.ref(states.device), states, R, lp, nxt)
        return (lp, nxt) if return_next else lp

    def score_nbest(self, hyps, hyp_lens, n_hyp=None, bos=True, eos=False, return_token_lp=False):
        """Sentence scores in the N-best layout of ``loss.ctc_score_nbest``: ``hyps`` int32 ``[B, N, U]``, ``hyp_lens``
        int32 ``[B, N]``, ``n_hyp`` int32 ``[B]`` or None (device tensors).  Returns float64 ``[B, N]``:
        ``score(hyps[b, n, :hyp_lens[b, n]], bos, eos)`` bit for bit, ``-inf`` for a bad token and for the slots behind
        ``n_hyp[b]``.  ``return_token_lp=True`` adds float32 ``[B, N, U]``, the value of every step (0 behind)."""
        import torch
        from . import _lib
        for name, t in (("hyps", hyps), ("hyp_lens", hyp_lens), ("n_hyp", n_hyp)):
            if t is not None and (t.dtype != torch.int32 or not t.is_contiguous()):
                raise ValueError("NGramLM.score_nbest: %s must be a contiguous int32 tensor" % name)
        if hyps.dim() != 3 or tuple(hyp_lens.shape) != tuple(hyps.shape[:2]):
            raise ValueError("NGramLM.score_nbest: hyps must be [B, N, U] and hyp_lens [B, N] (got %s, %s)"
                             % (tuple(hyps.shape), tuple(hyp_lens.shape)))
        if n_hyp is not None and tuple(n_hyp.shape) != (hyps.shape[0],):
            raise ValueError("NGramLM.score_nbest: n_hyp must be [B]")
        _lib.require_cuda(hyps, hyp_lens, n_hyp)
        B, N, U = hyps.shape
        total = torch.empty(B, N, dtype=torch.float64, device=hyps.device)
        tlp = torch.empty(B, N, U, dtype=torch.float32, device=hyps.device) if return_token_lp else None
        if B * N:
            _lib.call("ngram_score", self.ref(hyps.device), hyps if U else None, hyp_lens, n_hyp, B, N, U, bool(bos),
                      bool(eos), total, tlp if U else None)
        return (total, tlp) if return_token_lp else total

    def score_lists(self, lists, device="cuda", bos=True, eos=False):
        """Score ``lists[b]`` (token sequences) for every b: one upload, one ``score_nbest`` call, one read.  Returns a
        list of float64 arrays."""
        import torch
        lists = [[np.asarray(t, dtype=np.int64).reshape(-1) for t in seqs] for seqs in lists]
        B = len(lists)
        N = max([len(seqs) for seqs in lists], default=0)
        U = max([t.size for seqs in lists for t in seqs], default=0)
        if B == 0 or N == 0:
            return [np.zeros(0, dtype=np.float64) for _ in lists]
        nh, nl = B * N * U, B * N
        host = np.zeros(nh + nl + B, dtype=np.int32)
        hyps, hyp_lens = host[:nh].reshape(B, N, U), host[nh:nh + nl].reshape(B, N)
        for b, seqs in enumerate(lists):
            host[nh + nl + b] = len(seqs)
            for n, t in enumerate(seqs):
                hyps[b, n, :t.size] = np.clip(t, -1, self.V)
                hyp_lens[b, n] = t.size
        dev = torch.from_numpy(host).to(device)
        total = self.score_nbest(dev[:nh].view(B, N, U), dev[nh:nh + nl].view(B, N), dev[nh + nl:], bos, eos)
        total = total.cpu().numpy()
        return [total[b, :len(seqs)].copy() for b, seqs in enumerate(lists)]


def check_ngram_args(lm, lm_weight, length_bonus, V=None, blank=None, owner="the head's", max_V=None):
    """The argument rules of ``lm=`` on the CTC prefix search, and - with ``owner="the transducer's"`` and
    ``max_V=SYNC_NGRAM_MAX_V`` - of an ``NGramLM`` on the frame-synchronous search (raised before anything is
    launched)."""
    if lm is None:
        if lm_weight is not None:
            raise ValueError("lm_weight without lm")
        return
    if not isinstance(lm, NGramLM):
        raise TypeError("lm must be an edgedict_amd.ngram.NGramLM for the CTC prefix search (got %s)"
                        % type(lm).__name__)
    if lm_weight is None:
        raise ValueError("lm_weight is required with lm")
    w, lb = float(lm_weight), float(length_bonus)
    if not (np.isfinite(w) and w >= 0.0):
        raise ValueError("lm_weight must be a finite number >= 0 (got %r)" % lm_weight)
    if not np.isfinite(lb):
        raise ValueError("length_bonus must be finite (got %r)" % length_bonus)
    if V is not None and lm.V != V:
        raise ValueError("the n-gram's vocabulary (vocab_size = %d) differs from %s (V = %d)" % (lm.V, owner, V))
    if blank is not None and lm.blank != blank:
        raise ValueError("the n-gram's blank (%d) differs from the search's (%d)" % (lm.blank, blank))
    if max_V is not None and lm.V > max_V:
        raise ValueError("the n-gram's vocabulary (vocab_size = %d) exceeds %d: the search keeps a row's n-gram image "
                         "(12 bytes a symbol) in 64 KiB of LDS" % (lm.V, max_V))
