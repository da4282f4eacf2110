"""ORACLE glue (test infrastructure only): the back-off n-gram fused into the frame-synchronous beam search
(csrc/decode_sync.hip, sync_row_topw_ngram; decode.sync_beam_search*(lm=NGramLM)).  No new search: ``NGramAdapter`` gives
an ``edgedict_amd.ngram.NGramLM`` the interface ``sync_fusion_ref.Fusion.lm`` expects, and ``sync_fusion_ref.search``,
``ilme_ref.Fusion`` and the streaming ``StreamSearch`` are the oracle as they stand.  Their
``lm_weight * float(lp_lm[k]) + length_bonus`` is ``ngram_term``'s arithmetic (product rounded, then the bonus), on the
float64 value of ``NGramLM.step`` - which the kernel never rounds through fp32.

The oracle carries an LM state "from before the last token" and steps on the last token every frame; the adapter's
hidden value is the n-gram state BEFORE that token, so ``forward(tok, hidden)`` first moves to the state after it -
``start`` when ``hidden`` is None, the empty sequence, whatever ``lm_bos`` says - and returns that state's row.  The
kernel carries the state AFTER the sequence; the two are the same search.

The cases the host and the GPU tests share (``reference``) are here too, with their working points - found on the oracle
alone, on the CPU - so that tests/test_sync_ngram_host.py asserts every margin without a GPU."""
import functools

import torch

import ilme_ref as I
import ngram_ref as NR
import sync_fusion_ref as F
from bias_ref import BruteBias

MIN_MARGIN = 2e-3       # the project's value: ten times the 2e-4 score tolerance


class NGramAdapter:
    """``zero()`` / ``forward(tok, hidden) -> (float64 [1, V] log-probs, hidden)`` over an ``NGramLM``."""

    def __init__(self, lm):
        self.lm = lm

    def zero(self):
        return None

    def forward(self, tok, hidden):
        lm = self.lm
        s = lm.start if hidden is None else lm.step(hidden, int(torch.as_tensor(tok).reshape(-1)[0]))[1]
        row = [0.0 if k == lm.blank else lm.step(s, k)[0] for k in range(lm.V)]
        return torch.tensor([row], dtype=torch.float64), s


# ---------------------------------------------------------------------------------------------------- working points
# (config, mode, W) -> the n-gram's order (the model is ngram_ref.model(V, order)), lm_weight, length_bonus, ilm_weight,
# phrase list and boost.  For every case the first point of a small grid (order 3 / 2; weight 0.5 / 0.3 / 0.8; bonus
# 1 / 2 / 0.5 / 1.5 / 3 / 4 / 2.5 / 0; ilm_weight 0.2 / 0.1 / 0.3; test_sync_fusion_gpu's lists at 2.5 / 3.5 / 1.5) at
# which the ORACLE has margin and rank gap >= 3e-3, a merge at W > 1, tokens, and a best hypothesis that differs from the
# plain search's in at least one utterance.  The n-gram's log-probabilities are about -log V for an unseen token, so the
# LM alone empties the hypotheses unless the bonus pays for it - hence the larger bonuses of the "ngram" rows.
# Measured on the oracle, smallest margin / smallest rank gap / merges per utterance:
#   CFG   ngram          W = 1  8.2e-2 / - / 0 0 0    W = 4  6.5e-3 / 1.4e-2 / 1 1 2    W = 10 7.2e-3 / 4.6e-3 / 5 3 0
#         ngram+list     W = 1  3.1e-1 / - / 0 0 0    W = 4  2.5e-2 / 1.9e-1 / 4 4 2    W = 10 3.2e-3 / 4.2e-3 / 7 9 3
#         ngram+ilm      W = 1  1.3e-1 / - / 0 0 0    W = 4  2.0e-2 / 5.0e-3 / 2 1 0    W = 10 1.3e-2 / 8.0e-3 / 4 4 0
#         ngram+ilm+list W = 1  1.8e-1 / - / 0 0 0    W = 4  4.6e-2 / 4.1e-2 / 4 4 0    W = 10 2.2e-2 / 8.2e-3 / 7 8 4
#   CFG32 ngram          W = 1  2.8e-2 / - / 0 0 0    W = 4  9.5e-3 / 1.1e-2 / 2 1 0    W = 10 3.6e-3 / 4.1e-3 / 7 4 5
#         ngram+list     W = 1  3.8e-2 / - / 0 0 0    W = 4  9.5e-3 / 5.8e-1 / 4 4 4    W = 10 3.3e-3 / 7.4e-3 / 7 8 9 (retractions 2 0 0)
#         ngram+ilm      W = 1  5.9e-2 / - / 0 0 0    W = 4  2.1e-2 / 9.3e-2 / 1 0 0    W = 10 5.5e-3 / 3.7e-3 / 6 5 5
#         ngram+ilm+list W = 1  6.0e-1 / - / 0 0 0    W = 4  3.3e-2 / 5.1e-2 / 5 5 3    W = 10 7.7e-3 / 8.0e-3 / 7 10 9 (retractions 2 0 0)
#   CFGV  ngram          W = 1  1.4e-1 / - / 0 0 0    W = 4  2.1e-2 / 1.9e-2 / 2 0 0    W = 10 7.0e-3 / 5.0e-3 / 4 3 4
#         ngram+list     W = 1  2.6e-1 / - / 0 0 0    W = 4  3.9e-2 / 2.3e-1 / 3 3 4    W = 10 1.4e-2 / 4.1e-2 / 10 7 9
#         ngram+ilm      W = 1  6.5e-2 / - / 0 0 0    W = 4  1.9e-2 / 1.9e-2 / 0 0 2    W = 10 4.9e-3 / 5.9e-3 / 1 2 5
#         ngram+ilm+list W = 1  8.1e-2 / - / 0 0 0    W = 4  2.1e-2 / 9.3e-3 / 4 3 4    W = 10 3.2e-3 / 9.6e-3 / 8 5 7
MODES = ["ngram", "ngram+list", "ngram+ilm", "ngram+ilm+list"]
NAMES = ["CFG", "CFG32", "CFGV"]
WIDTHS = [1, 4, 10]


def _p(order, lm_weight, length_bonus, ilm_weight, phrases, boost):
    return dict(order=order, lm_weight=lm_weight, length_bonus=length_bonus, ilm_weight=ilm_weight, phrases=phrases,
                boost=boost)


POINTS = {
    ("CFG", "ngram", 1): _p(3, 0.5, 3.0, None, None, None),
    ("CFG", "ngram", 4): _p(3, 0.5, 3.0, None, None, None),
    ("CFG", "ngram", 10): _p(3, 0.5, 1.0, None, None, None),
    ("CFG", "ngram+list", 1): _p(3, 0.5, 1.0, None, ((17, 39),), 2.5),
    ("CFG", "ngram+list", 4): _p(3, 0.5, 1.0, None, ((17, 39),), 3.5),
    ("CFG", "ngram+list", 10): _p(3, 0.5, 1.0, None, ((17, 39),), 2.5),
    ("CFG", "ngram+ilm", 1): _p(3, 0.5, 1.0, 0.2, None, None),
    ("CFG", "ngram+ilm", 4): _p(3, 0.5, 1.0, 0.2, None, None),
    ("CFG", "ngram+ilm", 10): _p(3, 0.5, 1.0, 0.1, None, None),
    ("CFG", "ngram+ilm+list", 1): _p(3, 0.5, 1.0, 0.2, ((17, 39),), 2.5),
    ("CFG", "ngram+ilm+list", 4): _p(3, 0.5, 1.0, 0.2, ((17, 39),), 2.5),
    ("CFG", "ngram+ilm+list", 10): _p(3, 0.5, 1.0, 0.2, ((17, 39),), 2.5),
    ("CFG32", "ngram", 1): _p(3, 0.5, 2.0, None, None, None),
    ("CFG32", "ngram", 4): _p(3, 0.5, 1.0, None, None, None),
    ("CFG32", "ngram", 10): _p(3, 0.3, 0.0, None, None, None),
    ("CFG32", "ngram+list", 1): _p(3, 0.5, 1.0, None, ((10, 63),), 2.5),
    ("CFG32", "ngram+list", 4): _p(3, 0.5, 1.0, None, ((10, 63),), 2.5),
    ("CFG32", "ngram+list", 10): _p(3, 0.5, 2.0, None, ((10, 63),), 2.5),
    ("CFG32", "ngram+ilm", 1): _p(3, 0.5, 1.0, 0.3, None, None),
    ("CFG32", "ngram+ilm", 4): _p(3, 0.5, 1.0, 0.1, None, None),
    ("CFG32", "ngram+ilm", 10): _p(3, 0.5, 1.0, 0.2, None, None),
    ("CFG32", "ngram+ilm+list", 1): _p(3, 0.5, 1.0, 0.2, ((10, 63),), 2.5),
    ("CFG32", "ngram+ilm+list", 4): _p(3, 0.5, 1.0, 0.2, ((10, 63),), 2.5),
    ("CFG32", "ngram+ilm+list", 10): _p(3, 0.5, 1.0, 0.2, ((10, 63),), 2.5),
    ("CFGV", "ngram", 1): _p(3, 0.5, 4.0, None, None, None),
    ("CFGV", "ngram", 4): _p(2, 0.5, 4.0, None, None, None),
    ("CFGV", "ngram", 10): _p(3, 0.5, 3.0, None, None, None),
    ("CFGV", "ngram+list", 1): _p(3, 0.5, 1.0, None, ((1391, 1506),), 3.5),
    ("CFGV", "ngram+list", 4): _p(3, 0.5, 1.0, None, ((1391, 1506),), 2.5),
    ("CFGV", "ngram+list", 10): _p(3, 0.5, 2.0, None, ((1391, 1506),), 3.5),
    ("CFGV", "ngram+ilm", 1): _p(3, 0.5, 2.0, 0.3, None, None),
    ("CFGV", "ngram+ilm", 4): _p(3, 0.5, 1.0, 0.2, None, None),
    ("CFGV", "ngram+ilm", 10): _p(3, 0.5, 1.0, 0.3, None, None),
    ("CFGV", "ngram+ilm+list", 1): _p(3, 0.5, 1.0, 0.2, ((1391, 1506),), 2.5),
    ("CFGV", "ngram+ilm+list", 4): _p(3, 0.5, 1.0, 0.2, ((1391, 1506),), 3.5),
    ("CFGV", "ngram+ilm+list", 10): _p(3, 0.5, 1.0, 0.2, ((1391, 1506),), 2.5),
}


def point(name, mode, W):
    return POINTS[(name, mode, W)]


def ngram_of(name, order):
    from test_sync_beam_gpu import CFGS
    return NR.model(CFGS[name][0]["vocab_size"], order)


def fusion_of(sd, lm, lm_weight, length_bonus, ilm_weight=None, phrases=None, boost=None):
    """The oracle's fusion object of a point (``lm`` an ``NGramLM`` or None)."""
    return I.Fusion(ilm=I.model_ilm(sd) if ilm_weight is not None else None, ilm_weight=ilm_weight,
                    lm=NGramAdapter(lm) if lm is not None else None, lm_weight=lm_weight, length_bonus=length_bonus,
                    bias=BruteBias(list(phrases), boost) if phrases else None)


@functools.lru_cache(maxsize=None)
def reference(name, mode, W):
    """(ranked lists, info dicts) of the oracle per utterance on ``test_sync_beam_gpu._inputs(name)``: computed once,
    read only."""
    from test_sync_beam_gpu import _inputs
    sd, xs, xlen = _inputs(name)
    p = point(name, mode, W)
    fusion = fusion_of(sd, ngram_of(name, p["order"]), p["lm_weight"], p["length_bonus"], p.get("ilm_weight"),
                       p.get("phrases"), p.get("boost"))
    return F.search(sd, xs, xlen, W, fusion)


def search_with(sd, xs, xlen, W, lm, lm_weight, length_bonus, **kw):
    """The oracle on any inputs with any ``NGramLM``: the back-off edge cases."""
    return F.search(sd, xs, xlen, W, fusion_of(sd, lm, lm_weight, length_bonus, **kw))


def assert_decisive(infos, W, ref, merges=True):
    """The condition on the INPUTS every comparison with the oracle rests on: no selection and no final rank is a
    near-tie, something merges at W > 1 (the folded pair's state is exercised), some hypothesis holds tokens."""
    print("margin / gap / merges / retractions:",
          [(i["margin"], i["rank_gap"], i["merges"], i["retractions"]) for i in infos])
    for info in infos:
        assert info["margin"] >= MIN_MARGIN and info["rank_gap"] >= MIN_MARGIN, info
    assert W == 1 or not merges or sum(i["merges"] for i in infos) >= 1
    assert any(len(h["tokens"]) > 0 for r in ref for h in r)


def device_kwargs(name, mode, W, lm=None):
    """The keywords of the device call of a point."""
    from edgedict_amd.bias import ContextGraph
    from test_sync_beam_gpu import CFGS
    p = point(name, mode, W)
    kw = dict(lm=ngram_of(name, p["order"]) if lm is None else lm, lm_weight=p["lm_weight"],
              length_bonus=p["length_bonus"])
    if p.get("ilm_weight") is not None:
        kw["ilm_weight"] = p["ilm_weight"]
    if p.get("phrases"):
        kw["bias"] = ContextGraph([list(q) for q in p["phrases"]], p["boost"], CFGS[name][0]["vocab_size"])
    return kw


# ---------------------------------------------------------------------------------------------------- back-off edges
# A token present in the bigram row of (17,) AND in the trigram row of the reachable context (17, 17), with clearly
# different values (log10 -2.0 against -0.1): the longest context must win.  A fill without its barrier between levels,
# or with the levels in reverse order, leaves the bigram's value in the column.
LONGEST_WINS_ARPA = "\n".join([
    "\\data\\", "ngram 1=4", "ngram 2=2", "ngram 3=1", "",
    "\\1-grams:", "-99\t<s>\t-0.1", "-1.2\t</s>", "-1.5\t<unk>", "-1.0\t17\t-0.3", "",
    "\\2-grams:", "-0.5\t<s> 17\t-0.2", "-2.0\t17 17\t-0.2", "",
    "\\3-grams:", "-0.1\t17 17 17", "", "\\end\\", ""])


@functools.lru_cache(maxsize=None)
def edge_lm(edge):
    from edgedict_amd.ngram import NGramLM
    if edge == "order1":
        return NR.model(40, 1)
    if edge == "order6":
        return NR.model(40, 6)
    if edge == "wide":
        return NR.wide_model()
    if edge == "closure":
        return NR.closure_model()
    assert edge == "longest"
    return NGramLM.from_arpa(LONGEST_WINS_ARPA, None, 40)


# edge -> (base config name, vocab_size, W, lm_weight, length_bonus): the first point of weight 0.5 / 0.8 / 0.3 x bonus
# 1 / 2 / 3 / ... at which the oracle is decisive (>= 3e-3), merges, differs from the plain search and does what the
# edge is about.  Measured on the oracle, smallest margin / rank gap / merges per utterance:
#   order1   1.3e-2 / 2.3e-2 / 2 0 0     a model without arcs: only the unigram level
#   order6   6.1e-3 / 4.7e-3 / 1 1 2     hypotheses of up to 5 tokens: chains up to the model's longest
#   wide     3.1e-2 / 4.2e-1 / 4 4 4     V = 520 on CFG32; the beams hold [3, 111] and [3, 427]: rows on the 140-arc context
#   closure  9.8e-3 / 2.7e-2 / 4 2 4     V = 12; rows end on 5, whose state has a back-off weight and no arc
#   longest  4.6e-3 / 1.4e-1 / 3 4 0     the beams hold [17, 17, 17] and [17, 17, 17, 17]
EDGES = {"order1": ("CFG", 40, 4, 0.5, 1.0), "order6": ("CFG", 40, 4, 0.5, 3.0), "wide": ("CFG32", 520, 4, 0.5, 1.0),
         "closure": ("CFG", 12, 4, 0.5, 1.0), "longest": ("CFG", 40, 4, 0.8, 3.0)}


@functools.lru_cache(maxsize=None)
def edge_inputs(edge):
    """(cfg, sd, xs, xlen) of an edge's small transducer: the base config with the n-gram's vocabulary, sharpened as
    ``test_sync_beam_gpu._inputs`` does."""
    import sync_beam_ref as S
    from oracle import models_ref as M
    from test_sync_beam_gpu import CFGS
    base, V = EDGES[edge][:2]
    cfg = dict(CFGS[base][0], vocab_size=V)
    sd = S.sharpened(M.make_state_dict(cfg, CFGS[base][1]), blank_bias=3.0)
    xs, _, xlen, _ = M.make_batch(cfg, 4, 3, 9, 4, ragged=False)
    return cfg, sd, xs, xlen


@functools.lru_cache(maxsize=None)
def edge_reference(edge):
    _, sd, xs, xlen = edge_inputs(edge)
    _, _, W, w, lb = EDGES[edge]
    return search_with(sd, xs, xlen, W, edge_lm(edge), w, lb)
