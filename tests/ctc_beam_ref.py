"""Float64 numpy restatement of the CTC prefix beam search (csrc/ctc_decode.hip states the same search): the oracle of
the CTC beam tests, and the cases they share.

Per utterance; scores are float64 log-probabilities, ``-inf`` is zero.  A hypothesis is a node of a token tree
``(parent, token, frame it was created on)``, node 0 the empty prefix; it carries ``pb`` / ``pnb`` (paths ending in
blank / in its last token), ``tot = logadd(pb, pnb)``.  The beam starts as ``[root: pb 0, pnb -inf]``.  For every frame,
with ``lp = log_softmax(z[t])``:

1. candidates: the ``min(cand, V - 1)`` non-blank tokens of largest ``lp``, in that order, ties to the lower id;
2. stay: entry i keeps its slot with ``pb' = tot_i + lp[blank]`` and, unless it is the root, ``pnb' = pnb_i + lp[e_i]``;
3. extend: entry i, candidate c: ``p = (pb_i if c == e_i else tot_i) + lp[c]``; if the prefix ``(n_i, c)`` is beam entry
   j then ``pnb'_j = logadd(pnb'_j, p)``, otherwise it is a new candidate ``pb = -inf, pnb = p`` (no resurrection term);
   a candidate with ``p = -inf`` is no candidate;
4. select: the W best by ``logadd(pb', pnb')`` plus the node's bias total; ties to the lower canonical index (the stays
   in beam order, then the new candidates in the order step 3 made them); the new beam is in ranked order.

With a ``ContextGraph`` a node carries ``s = goto(s(parent), token)`` and ``Bn = Bn(parent) + D(s(parent), token)``;
``Bn`` enters the ranking and the reported ``logp`` only.

The decision margin is the minimum over all frames of (a) ``lp`` of the last kept candidate minus the first dropped
one, (b) the score of the last selected entry minus the first rejected one, (c) every gap between adjacent selected
entries: a search on slightly different scores decides the same while its errors stay below half of it.

``margin_nz`` is the same minimum over the gaps that are not EXACTLY zero.  bfloat16 logits repeat inside a frame (at
V = 520 two of a frame's tokens around the candidate cut share a value on most frames), and two tokens with the same
logit have bit-equal ``lp`` and, extended from the same entry, bit-equal scores - here and in the kernel, which forms
both from the same fp32 values - so both sides decide such a pair by the tie rule (lower token id, lower canonical
index), whatever the arithmetic error is.  A zero gap between scores that merely coincide would need two different
float64 sums to agree in every bit.
"""
import functools

import numpy as np

NEG = -np.inf


def logadd(a, b):
    m = max(a, b)
    if m == NEG:
        return NEG
    return m + np.log1p(np.exp(min(a, b) - m))


def log_softmax(z):
    z = np.asarray(z, dtype=np.float64)
    m = z.max(axis=-1, keepdims=True)
    return z - m - np.log(np.exp(z - m).sum(axis=-1, keepdims=True))


class Hyp:
    def __init__(self, tokens, frames, token_lp, logp):
        self.tokens, self.frames, self.token_lp, self.logp = tokens, frames, token_lp, logp


def search_one(z, W, cand, blank=0, graph=None):
    """One utterance: ``z`` [T, V] raw logits (T may be 0).  Returns ``(hyps, (margin, margin_nz), n_nodes)``: the
    ranked list of ``Hyp`` (tokens, creation frames, lp of each token on its frame, logp including the bias total) and
    the decision margins (``inf`` where nothing was decided)."""
    z = np.asarray(z, dtype=np.float64)
    T, V = z.shape
    K = min(int(cand), V - 1)
    # nodes: parent, token, frame, lp on that frame, automaton state, bias total
    par, tok, frm, tlp, st, bn = [-1], [-1], [-1], [0.0], [0], [0.0]
    beam = [(0, 0.0, NEG)]                                    # (node, pb, pnb)
    gaps = []
    for t in range(T):
        lp = log_softmax(z[t])
        order = sorted((v for v in range(V) if v != blank), key=lambda v: (-lp[v], v))
        C = order[:K]
        if len(order) > K:
            gaps.append(lp[C[-1]] - lp[order[K]])
        pbn = [logadd(pb, pnb) + lp[blank] for (_, pb, pnb) in beam]
        pnbn = [pnb + lp[tok[n]] if n != 0 else NEG for (n, _, pnb) in beam]
        child = {(par[n], tok[n]): j for j, (n, _, _) in enumerate(beam) if n != 0}
        fresh = []                                            # (score, p, parent node, token, state, bias total)
        for (n, pb, pnb) in beam:
            tot = logadd(pb, pnb)
            for c in C:
                p = (pb if c == tok[n] else tot) + lp[c]
                j = child.get((n, c))
                if j is not None:
                    pnbn[j] = logadd(pnbn[j], p)
                elif p > NEG:
                    s2, b2 = 0, 0.0
                    if graph is not None:
                        s2 = graph.goto(st[n], c)
                        b2 = bn[n] + (float(graph.held[s2]) - float(graph.pend[st[n]]))
                    fresh.append((p + b2, p, n, c, s2, b2))
        items = [(logadd(pbn[j], pnbn[j]) + bn[n], j) for j, (n, _, _) in enumerate(beam)]
        items += [(f[0], len(beam) + k) for k, f in enumerate(fresh)]
        items = [it for it in items if it[0] > NEG]
        items.sort(key=lambda it: (-it[0], it[1]))
        keep = items[:W]
        for a, b in zip(keep[:-1], keep[1:]):
            gaps.append(a[0] - b[0])
        if len(items) > W:
            gaps.append(keep[-1][0] - items[W][0])
        new = []
        for score, idx in keep:
            if idx < len(beam):
                new.append((beam[idx][0], pbn[idx], pnbn[idx]))
            else:
                _, p, n, c, s2, b2 = fresh[idx - len(beam)]
                par.append(n); tok.append(c); frm.append(t); tlp.append(float(lp[c])); st.append(s2); bn.append(b2)
                new.append((len(par) - 1, NEG, p))
        beam = new
    hyps = []
    for (n, pb, pnb) in beam:
        ts, fs, ls = [], [], []
        k = n
        while k != 0:
            ts.append(tok[k]); fs.append(frm[k]); ls.append(tlp[k])
            k = par[k]
        hyps.append(Hyp(ts[::-1], fs[::-1], ls[::-1], logadd(pb, pnb) + bn[n]))
    margin = (min(gaps, default=np.inf), min((g for g in gaps if g != 0.0), default=np.inf))
    return hyps, margin, len(par)


# ---------------------------------------------------------------------------------------------------- shared cases
def bf16_round(z):
    """float32 -> the nearest bfloat16 (round to nearest even), as float32."""
    u = np.ascontiguousarray(z, dtype=np.float32).view(np.uint32)
    r = ((u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000).astype(np.uint32)
    return r.view(np.float32)


def make_logits(T, V, seed, bf16=False):
    """The input generator of the GPU tests: blank = 0."""
    z = (np.random.default_rng(seed).standard_normal((T, V)) * 3).astype(np.float32)
    z[:, 0] += 2
    return bf16_round(z) if bf16 else z


# (T, V, W, cand) -> seed, per dtype; every seed meets the 1e-3 margin (test_ctc_beam_host.py re-checks all of them)
# The last two fill the beam beyond 512 items per frame (32 x 33 = 1056 with a full beam of 32, 10 x 65 = 650): the
# kernel's selection then leaves the items in LDS instead of registers
SHAPES = [(5, 8, 1, 7), (6, 8, 2, 1), (10, 29, 4, 8), (47, 32, 10, 16), (65, 40, 10, 32), (33, 520, 10, 32),
          (16, 4096, 4, 64), (129, 16, 10, 15), (64, 33, 3, 32), (8, 40, 32, 32), (10, 80, 10, 64)]
SEEDS = {
    "f32": {(5, 8, 1, 7): 0, (6, 8, 2, 1): 0, (10, 29, 4, 8): 0, (47, 32, 10, 16): 1, (65, 40, 10, 32): 26,
            (33, 520, 10, 32): 14, (16, 4096, 4, 64): 2, (129, 16, 10, 15): 4, (64, 33, 3, 32): 0,
            (8, 40, 32, 32): 1, (10, 80, 10, 64): 0},
    "bf16": {(5, 8, 1, 7): 0, (6, 8, 2, 1): 0, (10, 29, 4, 8): 0, (47, 32, 10, 16): 1, (65, 40, 10, 32): 7,
             (33, 520, 10, 32): 0, (16, 4096, 4, 64): 0, (129, 16, 10, 15): 63, (64, 33, 3, 32): 2,
             (8, 40, 32, 32): 16, (10, 80, 10, 64): 11},
}
# bfloat16 shapes on which no seed below 300 avoids two equal logits around a decision (docstring, margin_nz): these
# meet the condition over the non-zero gaps, as do the 33-frame utterance of the bfloat16 ragged batch and the two
# bfloat16 bias cases (the same shapes); every other bfloat16 case meets it as it stands.  `python tests/ctc_beam_ref.py`
# repeats the search that filled these tables (first seed below 300 that meets the strict margin, else the first that
# meets it over the non-zero gaps) and prints what it finds beside what is stored.
BF16_TIED = {(47, 32, 10, 16), (65, 40, 10, 32), (33, 520, 10, 32), (16, 4096, 4, 64), (129, 16, 10, 15),
             (8, 40, 32, 32)}
SEED_LIMIT = 300
# the unpruned case (25 prefixes of V = 3, T = 5 fit W = 32: nothing is cut), also the W = 32 case
UNPRUNED = (5, 3, 32, 2)
UNPRUNED_SEED = {"f32": 0, "bf16": 0}
# ragged batch: (shape, T_b) per utterance; utterance 1 has no frames, utterance 2 one
RAGGED = dict(V=40, W=10, cand=32, T=(33, 0, 1), seeds={"f32": (1, 0, 0), "bf16": (7, 0, 0)})
# biasing: two of the shapes, three phrases drawn from the unbiased top-1
BIAS_SHAPES = [(47, 32, 10, 16), (65, 40, 10, 32)]
BIAS_SEEDS = {"f32": {(47, 32, 10, 16): 5, (65, 40, 10, 32): 56}, "bf16": {(47, 32, 10, 16): 31, (65, 40, 10, 32): 176}}
BIAS_BOOST = 1.5
MARGIN = 1e-3


@functools.lru_cache(maxsize=None)
def case(shape, dtype, seed=None):
    """(z [T, V] float32 as the kernel sees it, hyps, margin, nodes) of a table case."""
    T, V, W, cand = shape
    seed = SEEDS[dtype][shape] if seed is None else seed
    z = make_logits(T, V, seed, dtype == "bf16")
    hyps, margin, nodes = search_one(z, W, cand)
    return z, hyps, margin, nodes


def phrases_from(tokens):
    """Three phrases out of a token sequence: its first two tokens, a middle triple, a single late token."""
    n = len(tokens)
    assert n >= 6
    return [list(tokens[:2]), list(tokens[n // 2:n // 2 + 3]), [tokens[-2]]]


def find_seed(shape, dtype, accept=lambda hyps: True, limit=SEED_LIMIT):
    """``(strict, relaxed)``: the first seed below ``limit`` whose case meets MARGIN as the margin stands, and the first
    that meets it over the non-zero gaps (None: no such seed); ``accept(hyps)`` can ask more of a case."""
    strict = relaxed = None
    for seed in range(limit):
        hyps, m, _ = search_one(make_logits(shape[0], shape[1], seed, dtype == "bf16"), shape[2], shape[3])
        if not accept(hyps):
            continue
        if relaxed is None and m[1] >= MARGIN:
            relaxed = seed
        if m[0] >= MARGIN:
            strict = seed
            break
    return strict, relaxed


if __name__ == "__main__":
    # the bfloat16 tables (the float32 seeds are the issue's and the reviewer's, re-checked by test_ctc_beam_host.py);
    # a few minutes
    for shape in SHAPES + [(RAGGED["T"][0], RAGGED["V"], RAGGED["W"], RAGGED["cand"])]:
        strict, relaxed = find_seed(shape, "bf16")
        stored = SEEDS["bf16"].get(shape, RAGGED["seeds"]["bf16"][0])
        print("bf16", shape, "strict seed", strict, "relaxed seed", relaxed, "stored", stored,
              "(tied)" if strict is None else "", flush=True)
