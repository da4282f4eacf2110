"""Float64 restatement of the CTC prefix beam search WITH an n-gram LM (csrc/ctc_decode.hip, LM = true): the search of
tests/ctc_beam_ref.py with one more term, and the cases the n-gram tests share.

A node carries the LM state after its token and ``Ln = Ln(parent) + (weight * step(s(parent), token) + length_bonus)``;
the root has ``lm.start`` and 0.  A new candidate ranks by ``(p + Bn) + Ln``, a stay by ``(logadd(pb', pnb') + Bn) + Ln``,
the reported logp is ``(tot + Bn) + Ln`` (``Bn``: the bias total, 0.0 without a list).  ``pb`` / ``pnb`` stay pure CTC, an
extension that merges into an existing entry adds nothing, and the candidate cut stays ahead of both terms.  The LM is
read through ``NGramLM.step`` (plain Python tables).  The decision margins are ctc_beam_ref's, LM terms included.

``python tests/ngram_ref.py`` repeats the seed search that filled the tables below and prints what it finds beside what
is stored (a few minutes).
"""
import functools

import numpy as np

import ctc_beam_ref as BR

NEG = -np.inf
LM_WEIGHT, LENGTH_BONUS = 0.5, 0.3


def search_one(z, W, cand, lm, weight, bonus, blank=0, graph=None):
    """``ctc_beam_ref.search_one`` with the LM term; same return value."""
    z = np.asarray(z, dtype=np.float64)
    T, V = z.shape
    K = min(int(cand), V - 1)
    logadd = BR.logadd
    par, tok, frm, tlp, st, bn, sl, ln = [-1], [-1], [-1], [0.0], [0], [0.0], [lm.start], [0.0]
    beam = [(0, 0.0, NEG)]
    gaps = []
    for t in range(T):
        lp = BR.log_softmax(z[t])
        order = sorted((v for v in range(V) if v != blank), key=lambda v: (-lp[v], v))
        C = order[:K]
        if len(order) > K:
            gaps.append(lp[C[-1]] - lp[order[K]])
        pbn = [logadd(pb, pnb) + lp[blank] for (_, pb, pnb) in beam]
        pnbn = [pnb + lp[tok[n]] if n != 0 else NEG for (n, _, pnb) in beam]
        child = {(par[n], tok[n]): j for j, (n, _, _) in enumerate(beam) if n != 0}
        fresh = []
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
                    l, m2 = lm.step(sl[n], c)
                    l2 = ln[n] + (weight * l + bonus)
                    fresh.append(((p + b2) + l2, p, n, c, s2, b2, m2, l2))
        items = [((logadd(pbn[j], pnbn[j]) + bn[n]) + ln[n], j) for j, (n, _, _) in enumerate(beam)]
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
                _, p, n, c, s2, b2, m2, l2 = fresh[idx - len(beam)]
                par.append(n); tok.append(c); frm.append(t); tlp.append(float(lp[c]))
                st.append(s2); bn.append(b2); sl.append(m2); ln.append(l2)
                new.append((len(par) - 1, NEG, p))
        beam = new
    hyps = []
    for (n, pb, pnb) in beam:
        ts, fs, ls = [], [], []
        k = n
        while k != 0:
            ts.append(tok[k]); fs.append(frm[k]); ls.append(tlp[k])
            k = par[k]
        hyps.append(BR.Hyp(ts[::-1], fs[::-1], ls[::-1], (logadd(pb, pnb) + bn[n]) + ln[n]))
    margin = (min(gaps, default=np.inf), min((g for g in gaps if g != 0.0), default=np.inf))
    return hyps, margin, len(par)


# ---------------------------------------------------------------------------------------------------- the models
def corpus(V, sentences=200, seed=7):
    """The training corpus of every test model: ``sentences`` lists of 3 .. 11 ids from ``3 .. V-1``; with probability
    0.8 the next token is one of 3 fixed successors of the current one, else uniform - real back-off structure.
    tools/ctc_ngram_time.py carries a copy of this generator for the model it times; the stored seeds depend on THIS
    one only."""
    rng = np.random.default_rng(seed)
    succ = rng.integers(3, V, size=(V, 3))
    out = []
    for _ in range(sentences):
        n = int(rng.integers(3, 12))
        k = int(rng.integers(3, V))
        sent = [k]
        while len(sent) < n:
            k = int(succ[k, rng.integers(0, 3)]) if rng.random() < 0.8 else int(rng.integers(3, V))
            sent.append(k)
        out.append(sent)
    return out


@functools.lru_cache(maxsize=None)
def model(V, order):
    from edgedict_amd.ngram import NGramLM
    return NGramLM.train(corpus(V), order, V)


@functools.lru_cache(maxsize=None)
def wide_model():
    """V = 520 bigram whose token 3 precedes 140 distinct tokens: its row spans three 64-arc rounds.  Most ids never
    occur, and ``(3,)`` apart every context has a handful of arcs."""
    from edgedict_amd.ngram import NGramLM
    V = 520
    sents = [[3, k] for k in range(10, 150)] + [[5, 6, 7], [6, 7, 5], [200, 3, 519]]
    return NGramLM.train(sents, 2, V)


@functools.lru_cache(maxsize=None)
def closure_model():
    """An order-4 model read from ARPA text whose only trigram context is (5, 6, 7): the suffix closure adds (6, 7) and
    (7,), states without a single arc."""
    from edgedict_amd.ngram import NGramLM
    text = "\n".join(["\\data\\", "ngram 1=4", "ngram 2=0", "ngram 3=0", "ngram 4=1", "", "\\1-grams:", "-99\t<s>\t0",
                      "-0.5\t</s>", "-1.5\t<unk>", "-0.4\t5\t-0.25", "", "\\2-grams:", "", "\\3-grams:", "",
                      "\\4-grams:", "-0.125\t5 6 7 8", "", "\\end\\", ""])
    return NGramLM.from_arpa(text, None, 12)


# ---------------------------------------------------------------------------------------------------- shared cases
# (T, V, W, cand, order) -> seed, per dtype: the first seed below 300 whose fused search decides with a margin of at
# least 1e-3 AND whose fused top-1 differs from the plain top-1 (the LM is seen to act).  bf16: the first seed that meets
# the margin as it stands, else (BF16_TIED) the first that meets it over the non-zero gaps, as ctc_beam_ref does.
SHAPES = [(6, 8, 2, 3, 2), (10, 29, 4, 8, 3), (47, 32, 10, 16, 3), (65, 40, 10, 32, 4), (33, 520, 10, 32, 3),
          (8, 40, 32, 32, 3), (10, 80, 10, 64, 5)]
SEEDS = {
    "f32": {(6, 8, 2, 3, 2): 0, (10, 29, 4, 8, 3): 0, (47, 32, 10, 16, 3): 4, (65, 40, 10, 32, 4): 1,
            (33, 520, 10, 32, 3): 1, (8, 40, 32, 32, 3): 33, (10, 80, 10, 64, 5): 1},
    "bf16": {(6, 8, 2, 3, 2): 0, (10, 29, 4, 8, 3): 0, (47, 32, 10, 16, 3): 1, (65, 40, 10, 32, 4): 77,
             (33, 520, 10, 32, 3): 3, (8, 40, 32, 32, 3): 20, (10, 80, 10, 64, 5): 1},
}
# no bf16 seed below 300 avoids two equal logits around a decision at V = 520 (ctc_beam_ref docstring, margin_nz)
BF16_TIED = {(33, 520, 10, 32, 3)}
# ragged batch: utterance 1 has no frames, utterance 2 one; any decision (no top-1 condition)
RAGGED = dict(V=40, W=10, cand=32, order=3, T=(33, 0, 1), seeds={"f32": (1, 0, 0), "bf16": (1, 0, 0)}, tied=set())
# bias and LM together: three phrases from the PLAIN top-1 (ctc_beam_ref.phrases_from), boost 1.5; the list with both
# differs from the list with the LM alone
BOTH_SHAPE = (47, 32, 10, 16, 3)
BOTH_SEEDS = {"f32": 1, "bf16": 6}
BOTH_TIED = set()
MARGIN = BR.MARGIN
SEED_LIMIT = BR.SEED_LIMIT


def graph(phrases, boost, V):
    from edgedict_amd.bias import ContextGraph
    return ContextGraph(phrases, boost, V, blank=0, bos=-1)


@functools.lru_cache(maxsize=None)
def case(shape, dtype, seed=None, with_bias=False):
    """``(z, hyps, margin, nodes, plain hyps, graph or None)`` of a case: the fused search of the shape's model on
    ``ctc_beam_ref.make_logits`` of the seed."""
    T, V, W, cand, order = shape
    seed = SEEDS[dtype][shape] if seed is None else seed
    z = BR.make_logits(T, V, seed, dtype == "bf16")
    plain = BR.search_one(z, W, cand)[0]
    g = None
    if with_bias:
        if len(plain[0].tokens) < 6:
            return z, None, (NEG, NEG), 0, plain, None
        g = graph(BR.phrases_from(plain[0].tokens), BR.BIAS_BOOST, V)
    hyps, margin, nodes = search_one(z, W, cand, model(V, order), LM_WEIGHT, LENGTH_BONUS, graph=g)
    return z, hyps, margin, nodes, plain, g


def find_seed(shape, dtype, accept, with_bias=False, limit=SEED_LIMIT):
    """``(strict, relaxed)`` as ``ctc_beam_ref.find_seed``; ``accept(case)`` can ask more of a case."""
    strict = relaxed = None
    for seed in range(limit):
        c = case(shape, dtype, seed, with_bias)
        if c[1] is None or not accept(c):
            continue
        if relaxed is None and c[2][1] >= MARGIN:
            relaxed = seed
        if c[2][0] >= MARGIN:
            strict = seed
            break
    return strict, relaxed


def lm_acts(c):
    """The fused top-1 differs from the plain top-1."""
    return c[1][0].tokens != c[4][0].tokens


def both_act(c):
    """With the bias list the list differs from the LM-only list of the same seed and shape."""
    z, hyps, _, _, plain, g = c
    T, V, W, cand, order = BOTH_SHAPE
    only = search_one(z, W, cand, model(V, order), LM_WEIGHT, LENGTH_BONUS)[0]
    return [h.tokens for h in hyps] != [h.tokens for h in only]


def stored_margin(m, dtype, tied):
    return m[1] if dtype == "bf16" and tied else m[0]


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))     # the package, run as a script
    for dtype in ("f32", "bf16"):
        for shape in SHAPES:
            strict, relaxed = find_seed(shape, dtype, lm_acts)
            print(dtype, shape, "strict seed", strict, "relaxed seed", relaxed, "stored", SEEDS[dtype].get(shape),
                  "(tied)" if strict is None else "", flush=True)
        for i, Tb in enumerate(RAGGED["T"]):
            shape = (Tb, RAGGED["V"], RAGGED["W"], RAGGED["cand"], RAGGED["order"])
            strict, relaxed = find_seed(shape, dtype, lambda c: True)
            print(dtype, "ragged", shape, "strict seed", strict, "relaxed seed", relaxed, "stored",
                  RAGGED["seeds"][dtype][i], flush=True)
        strict, relaxed = find_seed(BOTH_SHAPE, dtype, both_act, with_bias=True)
        print(dtype, "bias + lm", BOTH_SHAPE, "strict seed", strict, "relaxed seed", relaxed, "stored",
              BOTH_SEEDS[dtype], flush=True)
