"""CPU: the CTC prefix beam search's host side.  The float64 restatement tests/ctc_beam_ref.py that the GPU tests compare
against is pinned here - unpruned, its scores are the CTC likelihoods of tests/ctc_ref.py for every prefix - with its tie
rule and its biasing; the new C symbols and every argument error (raised before anything is launched); and the margin
condition of every case tests/test_ctc_beam_gpu.py runs, so that no GPU test has to skip or hunt for a seed."""
import ctypes

import numpy as np
import pytest
import torch

import ctc_beam_ref as BR
import ctc_ref as CR


def _graph(phrases, boost, V):
    from edgedict_amd.bias import ContextGraph
    return ContextGraph(phrases, boost, V, blank=0, bos=-1)


def _favouring(path, V=3, strength=4.0):
    """Logits whose frame t favours symbol path[t]."""
    z = np.zeros((len(path), V))
    for t, k in enumerate(path):
        z[t, k] = strength
    return z


def test_unpruned_search_scores_every_prefix_with_its_ctc_likelihood():
    """V = 3, T <= 5, W = 64, cand = 2: nothing is cut, so the list is every prefix with a path, each logp the CTC
    log-likelihood of the prefix as a transcript (1e-12), and the probabilities sum to 1.  Random rows, rows that favour
    a repeated token with a blank between (1 _ 1) and without (1 1 1: one token; 1 1 _ 2 2), and all-equal rows."""
    rng = np.random.default_rng(0)
    sets = [2.0 * rng.normal(size=(T, 3)) for T in (1, 2, 3, 4, 5, 5)]
    sets += [_favouring([1, 0, 1]), _favouring([1, 0, 1, 0, 1]), _favouring([1, 1, 1, 1]), _favouring([1, 1, 0, 2, 2]),
             _favouring([2, 2, 2, 1, 1]), np.zeros((5, 3))]
    feasible = {1: 3, 2: 5, 3: 9, 4: 15, 5: 25}          # prefixes y over {1, 2} with len(y) + repeats(y) <= T
    worst = 0.0
    for z in sets:
        hyps, _, nodes = BR.search_one(z, 64, 2)
        assert len(hyps) == feasible[z.shape[0]] == nodes
        assert len({tuple(h.tokens) for h in hyps}) == len(hyps)
        assert all(a.logp >= b.logp for a, b in zip(hyps[:-1], hyps[1:]))
        for h in hyps:
            want = -CR.ctc_one(z, h.tokens)[0]
            worst = max(worst, abs(h.logp - want))
            assert abs(h.logp - want) <= 1e-12, (h.tokens, h.logp, want)
            lp = CR.log_softmax(z)
            assert h.token_lp == [lp[t, k] for t, k in zip(h.frames, h.tokens)]
            assert all(a < b for a, b in zip(h.frames[:-1], h.frames[1:]))
        assert abs(sum(np.exp(h.logp) for h in hyps) - 1.0) <= 1e-12
    print("unpruned: max |logp - ctc| %.3g" % worst)
    # the favoured readings win
    assert BR.search_one(_favouring([1, 0, 1]), 64, 2)[0][0].tokens == [1, 1]
    assert BR.search_one(_favouring([1, 1, 1, 1]), 64, 2)[0][0].tokens == [1]
    assert BR.search_one(_favouring([1, 1, 0, 2, 2]), 64, 2)[0][0].tokens == [1, 2]


def test_tie_rule_on_all_zero_logits():
    """Equal scores go to the lower canonical index: the stays first, then the new candidates in (entry, candidate)
    order, candidates by token id."""
    z = np.zeros((3, 3))
    assert [h.tokens for h in BR.search_one(z[:1], 1, 2)[0]] == [[]]
    assert [h.tokens for h in BR.search_one(z[:1], 2, 2)[0]] == [[], [1]]
    assert [h.tokens for h in BR.search_one(z[:1], 3, 2)[0]] == [[], [1], [2]]
    # three frames, W = 2.  Frame 0: root, [1], [2] at 1/3 each, the stay and the first candidate survive.  Frame 1: [1]
    # 3/9, then root, [2] and [1, 2] at 1/9: the stay again.  Frame 2: [1] 6/27, [1, 2] 3/27, the rest 1/27.
    hyps, margin, _ = BR.search_one(z, 2, 2)
    assert [h.tokens for h in hyps] == [[1], [1, 2]]
    assert margin[0] == 0.0
    assert abs(hyps[0].logp - np.log(6.0 / 27.0)) <= 1e-12 and abs(hyps[1].logp - np.log(3.0 / 27.0)) <= 1e-12
    # candidates: ties to the lower token id, the blank is never one
    hyps, _, _ = BR.search_one(np.zeros((1, 5)), 5, 2, blank=2)
    assert [h.tokens for h in hyps] == [[], [0], [1]]


def test_bias_changes_the_top_and_adds_exactly_the_graph_score():
    """A hand-built case: frames favour 1 _ 2 but 3 is close behind 2 on the last frame; boosting the phrase [1, 3]
    makes [1, 3] the answer.  Every reported logp minus graph.score(tokens) is the unbiased score of that prefix."""
    z = np.array([[0.0, 3.0, 0.0, 0.0], [3.0, 0.0, 0.0, 0.0], [0.0, 0.0, 2.0, 1.6]])
    plain, _, _ = BR.search_one(z, 64, 3)
    g = _graph([[1, 3], [2, 2, 1]], 0.5, 4)
    biased, _, _ = BR.search_one(z, 64, 3, graph=g)
    assert plain[0].tokens == [1, 2] and biased[0].tokens == [1, 3]
    base = {tuple(h.tokens): h.logp for h in plain}
    assert {tuple(h.tokens) for h in biased} == set(base)          # unpruned: the same set, re-ranked
    assert any(g.score(h.tokens) > 0 for h in biased)
    for h in biased:
        assert abs((h.logp - g.score(h.tokens)) - base[tuple(h.tokens)]) <= 1e-12, h.tokens
    assert all(a.logp >= b.logp for a, b in zip(biased[:-1], biased[1:]))
    # a partial match that breaks gives its bonus back: [2, 2] holds 1.0 of [2, 2, 1], [2, 2, 3] nothing
    assert g.score([2, 2]) == 1.0 and g.score([2, 2, 3]) == 0.0
    # pruning happens before the bias is seen: with cand = 1 token 3 is no candidate on the last frame
    cut, _, _ = BR.search_one(z, 64, 1, graph=_graph([[1, 3]], 50.0, 4))
    assert all(3 not in h.tokens for h in cut)


def test_new_symbols_are_declared_and_exported(hip_lib):
    from edgedict_amd import _lib
    want = {"edgedict_ctc_beam_workspace_bytes", "edgedict_ctc_beam_search"}
    assert want <= set(_lib.declared_symbols())
    for name in want:
        assert hasattr(hip_lib, name), name
    assert hip_lib.edgedict_abi_version() == 2
    f = hip_lib.edgedict_ctc_beam_workspace_bytes
    assert f.restype is ctypes.c_size_t
    assert f(0, 5, 4, 8) == 0 and f(2, 0, 4, 8) == 0
    assert f(2, 5, 0, 8) == 0 and f(2, 5, 33, 8) == 0 and f(2, 5, 4, 0) == 0 and f(2, 5, 4, 65) == 0
    n = f(2, 5, 4, 8)
    # the candidate lists, and 1 + T W nodes of 16 bytes per utterance
    assert n >= 2 * 5 * 8 * 8 + 2 * (1 + 5 * 4) * 16 and n % 256 == 0
    assert f(64, 201, 32, 64) > f(64, 201, 10, 32) > n


def test_argument_errors_are_raised_before_any_launch(hip_lib):
    """A null pointer, W = 0 / 33, cand = 0 / 65, V = 1, a bad blank, a bad dtype code, a bias list of another
    vocabulary: -1 with a message naming the argument; no device needed."""
    buf = ctypes.create_string_buffer(64)
    fake = ctypes.cast(buf, ctypes.c_void_p)

    def run(logits=fake, dtype=0, al=fake, V=16, blank=0, W=4, cand=8, bias=None, tokens=fake, frames=fake, tlp=fake,
            ntok=fake, nhyp=fake, logp=fake, ws=fake):
        return hip_lib.edgedict_ctc_beam_search(logits, dtype, al, 2, 5, V, blank, W, cand, bias, tokens, frames, tlp,
                                                ntok, nhyp, logp, ws, None)

    for name in ("logits", "al", "tokens", "frames", "tlp", "ntok", "nhyp", "logp", "ws"):
        assert run(**{name: None}) == -1, name
        assert b"null pointer" in hip_lib.edgedict_last_error(), name
    for kw, word in ((dict(W=0), b"W = 0"), (dict(W=33), b"W = 33"), (dict(cand=0), b"cand = 0"),
                     (dict(cand=65), b"cand = 65"), (dict(V=1), b"V = 1"), (dict(blank=16), b"blank"),
                     (dict(blank=-1), b"blank"), (dict(dtype=7), b"dtype")):
        assert run(**kw) == -1, kw
        assert word in hip_lib.edgedict_last_error(), kw
    from edgedict_amd.bias import BeamBias
    bad = BeamBias()
    bad.S, bad.V, bad.n_exc = 1, 12, 0
    assert run(bias=ctypes.byref(bad)) == -1
    assert b"vocabulary" in hip_lib.edgedict_last_error()
    bad.V = 16
    assert run(bias=ctypes.byref(bad)) == -1
    assert b"null bias table" in hip_lib.edgedict_last_error()
    assert run(ws=ctypes.c_void_p(fake.value + 4)) == -1
    assert b"aligned" in hip_lib.edgedict_last_error()


def test_python_wrapper_refuses_cpu_tensors_and_bad_arguments():
    from edgedict_amd.loss import ctc_prefix_beam
    z = torch.zeros(2, 5, 8)
    al = torch.tensor([5, 4], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ctc_prefix_beam(z, al)
    with pytest.raises(TypeError, match="float32 or bfloat16"):
        ctc_prefix_beam(z.double(), al)
    with pytest.raises(TypeError, match="act_lens must be int32"):
        ctc_prefix_beam(z, al.long())
    with pytest.raises(ValueError, match="3 dimensions"):
        ctc_prefix_beam(z[0], al)
    with pytest.raises(ValueError, match="contiguous"):
        ctc_prefix_beam(z.transpose(1, 2), al)
    with pytest.raises(ValueError, match="length per example"):
        ctc_prefix_beam(z, al[:1])
    for kw, word in ((dict(W=0), "W = 0"), (dict(W=33), "W = 33"), (dict(cand=0), "cand = 0"),
                     (dict(cand=65), "cand = 65"), (dict(blank=8), "blank"), (dict(blank=-1), "blank")):
        with pytest.raises(ValueError, match=word):
            ctc_prefix_beam(z, al, **kw)
    with pytest.raises(ValueError, match="T = 0"):
        ctc_prefix_beam(z[:, :0].contiguous(), al)
    with pytest.raises(ValueError, match="B = 0"):
        ctc_prefix_beam(z[:0].contiguous(), al[:0].contiguous())
    with pytest.raises(ValueError, match="V = 1"):
        ctc_prefix_beam(z[:, :, :1].contiguous(), al)
    with pytest.raises(ValueError, match="ContextGraph"):
        ctc_prefix_beam(z, al, bias=[[1, 2]])
    with pytest.raises(ValueError, match="vocabulary"):
        ctc_prefix_beam(z, al, bias=_graph([[1, 2]], 1.0, 9))


def test_model_without_a_head_raises_what_greedy_raises():
    from edgedict_amd.models import Transducer
    kw = dict(vocab_embed_size=8, vocab_size=12, input_size=16, enc_hidden_size=16, enc_layers=2, enc_dropout=0.0,
              enc_proj_size=12, dec_hidden_size=8, dec_layers=1, dec_dropout=0.0, dec_proj_size=8, joint_size=16)
    plain = Transducer(**kw)
    with pytest.raises(RuntimeError, match="no CTC head"):
        plain.ctc_beam_search(torch.zeros(1, 4, 16), torch.tensor([4]))


# ------------------------------------------------------------------------------------------------ the margin condition
def _margin(m, strict):
    return m[0] if strict else m[1]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_every_gpu_case_meets_the_margin_condition(dtype):
    """Every case of tests/test_ctc_beam_gpu.py decides with a margin of at least 1e-3, ten times the absolute score
    bound of the GPU tests, so no GPU test skips and a seed that fails is replaced HERE.  float32: the margin as the
    oracle defines it, on every case.  bfloat16: the same on the cases whose logits do not repeat around a decision;
    on the others (ctc_beam_ref.BF16_TIED, the 33-frame utterance of the ragged batch, the two biased shapes) the margin
    over the non-zero gaps - a zero gap there is between two tokens with the same logit, which both sides decide by
    token id whatever their arithmetic error (ctc_beam_ref docstring)."""
    strict = lambda shape: dtype == "f32" or shape not in BR.BF16_TIED
    worst = np.inf
    for shape in BR.SHAPES:
        z, hyps, m, nodes = BR.case(shape, dtype)
        assert len(hyps) == min(shape[2], nodes)
        worst = min(worst, _margin(m, strict(shape)))
        assert _margin(m, strict(shape)) >= BR.MARGIN, (shape, m)
    assert BR.case((129, 16, 10, 15), "f32")[3] == 968
    z, hyps, m, _ = BR.case(BR.UNPRUNED, dtype, BR.UNPRUNED_SEED[dtype])
    assert len(hyps) == 25 and m[0] >= BR.MARGIN
    for Tb, seed in zip(BR.RAGGED["T"], BR.RAGGED["seeds"][dtype]):
        shape = (Tb, BR.RAGGED["V"], BR.RAGGED["W"], BR.RAGGED["cand"])
        m = BR.case(shape, dtype, seed)[2]
        assert _margin(m, dtype == "f32" or Tb <= 1) >= BR.MARGIN, (shape, m)
    for shape in BR.BIAS_SHAPES:
        z, hyps, m, _ = BR.case(shape, dtype, BR.BIAS_SEEDS[dtype][shape])
        g = _graph(BR.phrases_from(hyps[0].tokens), BR.BIAS_BOOST, shape[1])
        biased, mb, _ = BR.search_one(z, shape[2], shape[3], graph=g)
        assert _margin(m, dtype == "f32") >= BR.MARGIN and _margin(mb, dtype == "f32") >= BR.MARGIN
        assert [h.tokens for h in biased] != [h.tokens for h in hyps]       # the bias list decides something
        worst = min(worst, _margin(mb, dtype == "f32"))
    print("margin", dtype, "smallest %.3g" % worst)
