"""GPU: the CTC prefix beam search with an n-gram LM (csrc/ctc_decode.hip, LM = true) against the float64 restatement
tests/ngram_ref.py.  test_ngram_host.py checks on the CPU that every case here decides with a margin of at least 1e-3
(LM terms included) and that the LM changes the top-1, so tokens, frames and the order of the lists are compared
EXACTLY; logp within the bounds of tests/test_ctc_beam_gpu.py (fp32 rtol 1e-5 / atol 1e-4, bf16 rtol 1e-4)."""
import ctypes

import numpy as np
import pytest
import torch

import ctc_beam_ref as BR
import ngram_ref as NR
from test_ctc_beam_gpu import _TORCH, _compare, _tiny

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dtype", ["f32", "bf16"])
FUSED = dict(lm_weight=NR.LM_WEIGHT, length_bonus=NR.LENGTH_BONUS)


def _batch(zs, dtype):
    V = zs[0].shape[1]
    T = max(1, max(z.shape[0] for z in zs))
    batch = np.full((len(zs), T, V), np.nan, dtype=np.float32)       # NaN rows: a read past T_b shows
    for b, z in enumerate(zs):
        batch[b, :z.shape[0]] = z
    tz = torch.tensor(batch, device="cuda").to(_TORCH[dtype])
    act = torch.tensor([z.shape[0] for z in zs], dtype=torch.int32, device="cuda")
    return tz, act


def _search(zs, dtype, W, cand, **kw):
    from edgedict_amd.loss import ctc_prefix_beam
    tz, act = _batch(zs, dtype)
    return ctc_prefix_beam(tz, act, W=W, blank=0, cand=cand, **kw)


@pytest.mark.parametrize("shape", NR.SHAPES, ids=["%dx%dx%dx%d-o%d" % s for s in NR.SHAPES])
@DTYPES
def test_shapes_against_the_oracle_and_run_to_run(hip_lib, shape, dtype):
    """Every shape with an utterance of no frames beside it: the lists are the oracle's, the LM moved the top-1, the
    empty utterance gives the empty prefix with logp 0, two runs are bit-identical."""
    T, V, W, cand, order = shape
    z, hyps, margin, nodes, plain, _ = NR.case(shape, dtype)
    lm = NR.model(V, order)
    out = _search([z, z[:0]], dtype, W, cand, lm=lm, **FUSED)
    e_logp, e_tlp = _compare(out, 0, hyps, dtype, shape)
    _compare(out, 1, [BR.Hyp([], [], [], 0.0)], dtype, (shape, "empty"))
    assert out[5][1, 0].item() == 0.0
    n0 = int(out[3][0, 0])
    assert out[0][0, 0, :n0].tolist() == hyps[0].tokens != plain[0].tokens
    print("ctc beam ngram", shape, dtype, "states %d arcs %d nodes %d, margin %.3g / %.3g: max logp err %.3g (|logp| %.4g), "
          "max token_lp err %.3g" % (lm.n_states, lm.n_arcs, nodes, margin[0], margin[1], e_logp, abs(hyps[0].logp), e_tlp))
    again = _search([z, z[:0]], dtype, W, cand, lm=lm, **FUSED)
    for a, b in zip(out, again):
        assert torch.equal(a, b)


@DTYPES
def test_ragged_batch_with_an_empty_and_a_one_frame_utterance(hip_lib, dtype):
    r = NR.RAGGED
    zs, want = [], []
    for Tb, seed in zip(r["T"], r["seeds"][dtype]):
        c = NR.case((Tb, r["V"], r["W"], r["cand"], r["order"]), dtype, seed)
        zs.append(c[0])
        want.append(c[1])
    assert [len(h) for h in want] == [r["W"], 1, r["W"]]
    out = _search(zs, dtype, r["W"], r["cand"], lm=NR.model(r["V"], r["order"]), **FUSED)
    errs = [_compare(out, b, want[b], dtype, ("ragged", b)) for b in range(len(zs))]
    print("ctc beam ngram ragged", dtype, "max logp err %.3g, max token_lp err %.3g" % tuple(np.max(errs, axis=0)))


@DTYPES
def test_bias_and_lm_together(hip_lib, dtype):
    """Both terms on one shape: the list is the oracle's, whose logp is (tot + Bn) + Ln, and differs from the LM-only
    list (test_ngram_host.py); the reported logp minus both totals is the same prefix' plain CTC score."""
    shape = NR.BOTH_SHAPE
    T, V, W, cand, order = shape
    z, hyps, margin, _, plain, g = NR.case(shape, dtype, NR.BOTH_SEEDS[dtype], True)
    lm = NR.model(V, order)
    out = _search([z, z[:0]], dtype, W, cand, bias=g, lm=lm, **FUSED)
    e_logp, e_tlp = _compare(out, 0, hyps, dtype, (shape, "bias + lm"))
    _compare(out, 1, [BR.Hyp([], [], [], 0.0)], dtype, (shape, "bias + lm", "empty"))
    assert max(g.score(h.tokens) for h in hyps) > 0
    print("ctc beam bias + ngram", shape, dtype, "margin %.3g / %.3g, max logp err %.3g" % (margin[0], margin[1], e_logp))


@DTYPES
def test_zero_weight_and_no_lm_are_the_plain_search_bit_for_bit(hip_lib, dtype):
    """lm_weight = 0 with length_bonus = 0 runs the LM kernel and returns the plain call's tensors, every one of them;
    lm=None IS the plain call: on the shapes of tests/test_ctc_beam_gpu.py it returns what the plain entry point
    returns when called directly, as does the fused entry point with no options and with empty options.  All of these
    reach the same LM = false launch, so this second half checks the routing; the comparison with the oracle
    (tokens and frames exact, logp within its bound) is what ties that launch to the search as it was."""
    from edgedict_amd import _lib
    from edgedict_amd.loss import ctc_prefix_beam
    from edgedict_amd.ngram import CtcBeamOpts
    for shape in NR.SHAPES:
        T, V, W, cand, order = shape
        z = NR.case(shape, dtype)[0]
        base = _search([z, z[:0]], dtype, W, cand)
        zero = _search([z, z[:0]], dtype, W, cand, lm=NR.model(V, order), lm_weight=0.0, length_bonus=0.0)
        for a, b in zip(base, zero):
            assert torch.equal(a, b), shape
    for shape in BR.SHAPES:
        T, V, W, cand = shape
        z, hyps, _, _ = BR.case(shape, dtype)
        tz, act = _batch([z, z[:0]], dtype)
        out = ctc_prefix_beam(tz, act, W=W, blank=0, cand=cand, lm=None)
        _compare(out, 0, hyps, dtype, shape)
        ws = torch.empty(hip_lib.edgedict_ctc_beam_workspace_bytes(2, T, W, cand), dtype=torch.uint8, device="cuda")
        for name, opts in (("ctc_beam_search", None), ("ctc_beam_search_fused", None),
                           ("ctc_beam_search_fused", ctypes.byref(CtcBeamOpts()))):
            raw = [torch.full_like(t, -5) for t in out]
            _lib.call(name, tz, _lib.dtype_code(tz.dtype), act, 2, T, V, 0, W, cand, opts, *raw, ws)
            for a, b in zip(out, raw):
                assert torch.equal(a, b), (shape, name)


# --------------------------------------------------------------------------------------------------- model level
@pytest.mark.parametrize("cd", ["fp32", "bf16"])
def test_model_search_with_an_lm_is_the_search_of_its_own_head_logits(hip_lib, cd):
    """Transducer.ctc_beam_search(..., lm=) on the tiny model with a head = loss.ctc_prefix_beam(..., lm=) on the model's
    own head logits, with and without a bias list beside it; the LM changes some list."""
    from edgedict_amd.bias import ContextGraph
    from edgedict_amd.loss import ctc_prefix_beam
    from edgedict_amd.models import Transducer
    cfg, sd, (xs, ys, xlen, ylen) = _tiny()
    torch.manual_seed(11)
    m = Transducer(enc_dropout=0.0, dec_dropout=0.0, ctc_weight=0.3, **cfg)
    m.load_state_dict(sd, strict=False)
    m = m.cuda().eval()
    m.compute_dtype = cd
    V = cfg["vocab_size"]
    lm = NR.model(V, 3)
    with torch.no_grad():
        h_enc, _ = m.encoder(xs[:, :int(xlen.max())].contiguous().cuda())
        act = m.scale_length(h_enc, xlen).to(device="cuda", dtype=torch.int32).contiguous()
        logits = m._ctc_logits(h_enc).contiguous()
    plain = m.ctc_beam_search(xs.cuda(), xlen, W=4, cand=8)
    moved = False
    for bias in (None, ContextGraph([[5, 6], [7]], 1.0, V, blank=0, bos=-1)):
        res = m.ctc_beam_search(xs.cuda(), xlen, W=4, cand=8, bias=bias, lm=lm, lm_weight=2.0, length_bonus=0.5)
        tokens, frames, tlp, ntok, nhyp, logp = [t.cpu().numpy() for t in ctc_prefix_beam(
            logits, act, 4, m.blank, 8, bias, lm=lm, lm_weight=2.0, length_bonus=0.5)]
        assert len(res) == xs.shape[0]
        for b, r in enumerate(res):
            assert len(r) == int(nhyp[b]) >= 1
            assert (r.logp == logp[b, :len(r)]).all() and (np.diff(r.logp) <= 0).all()
            for h in range(len(r)):
                n = int(ntok[b, h])
                assert r.tokens[h].tolist() == tokens[b, h, :n].tolist()
                assert r.frames[h].tolist() == frames[b, h, :n].tolist()
                assert (r.token_logp[h] == tlp[b, h, :n].astype(np.float64)).all()
            moved = moved or [t.tolist() for t in r.tokens] != [t.tolist() for t in plain[b].tokens]
    assert moved


def test_lm_rescore_against_a_numpy_restatement(hip_lib):
    """decode.lm_rescore on the lists of a fused-free search: lm_logp is the host score of every hypothesis bit for bit,
    logp is logp + (weight * lm_logp + length_bonus * ntok), the order its stable descending sort; ctc_logp travels."""
    from edgedict_amd.decode import NBestResult, lm_rescore
    shape = (47, 32, 10, 16, 3)
    T, V, W, cand, order = shape
    lm = NR.model(V, order)
    results = []
    for seed in (4, 5):
        plain = NR.case(shape, "f32", seed)[4]
        results.append(NBestResult([np.array(h.tokens, dtype=np.int64) for h in plain],
                                   [np.array(h.frames, dtype=np.int32) for h in plain],
                                   [np.array(h.token_lp) for h in plain], np.array([h.logp for h in plain]),
                                   np.arange(len(plain), dtype=np.float64)))
    results.append(NBestResult([], [], [], np.zeros(0)))
    for eos in (False, True):
        out = lm_rescore(results, lm, 0.7, length_bonus=0.2, eos=eos)
        assert len(out) == 3 and len(out[2]) == 0
        changed = False
        for r, o in zip(results[:2], out[:2]):
            lp = np.array([lm.score(t, bos=True, eos=eos) for t in r.tokens])
            combined = r.logp + (0.7 * lp + 0.2 * np.array([len(t) for t in r.tokens], dtype=np.float64))
            order_ = np.argsort(-combined, kind="stable")
            assert (o.logp == combined[order_]).all() and (o.lm_logp == lp[order_]).all()
            assert (o.ctc_logp == order_).all()
            assert [t.tolist() for t in o.tokens] == [r.tokens[i].tolist() for i in order_]
            assert [f.tolist() for f in o.frames] == [r.frames[i].tolist() for i in order_]
            changed = changed or order_.tolist() != list(range(len(r)))
        assert changed
    same = lm_rescore(results[:1], lm, 0.0)[0]
    assert (same.logp == results[0].logp).all() and same.lm_logp is not None
