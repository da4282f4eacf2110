"""GPU: the CTC prefix beam search (csrc/ctc_decode.hip) against the float64 restatement tests/ctc_beam_ref.py, which
test_ctc_beam_host.py pins on the CPU together with the margin condition of every case here: each case decides with a
margin of at least 1e-3, so tokens, frames and the order of the list are compared EXACTLY.

Bounds: logp within the CTC cost bounds of tests/test_ctc_gpu.py (fp32 rtol 1e-5 / atol 1e-4, bf16 rtol 1e-4 - the
same arithmetic: fp32 log-sum-exp, fp64 carry with an fp32 correction term), token_lp within 1e-5 (fp32) / 1e-3 (bf16).
Every batch is padded to its longest utterance with NaN rows: a NaN in any output proves a read past T_b.  Every test
prints its maximum errors."""
import functools

import numpy as np
import pytest
import torch

import ctc_beam_ref as BR

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dtype", ["f32", "bf16"])
_TORCH = {"f32": torch.float32, "bf16": torch.bfloat16}


def _graph(phrases, boost, V):
    from edgedict_amd.bias import ContextGraph
    return ContextGraph(phrases, boost, V, blank=0, bos=-1)


def _search(zs, dtype, W, cand, bias=None, blank=0):
    """Run the batch of utterances ``zs`` (list of [T_b, V] float32, already rounded for bf16), NaN-padded.  Returns the
    six output tensors (device)."""
    from edgedict_amd.loss import ctc_prefix_beam
    V = zs[0].shape[1]
    T = max(1, max(z.shape[0] for z in zs))
    batch = np.full((len(zs), T, V), np.nan, dtype=np.float32)
    for b, z in enumerate(zs):
        batch[b, :z.shape[0]] = z
    tz = torch.tensor(batch, device="cuda").to(_TORCH[dtype])
    act = torch.tensor([z.shape[0] for z in zs], dtype=torch.int32, device="cuda")
    return ctc_prefix_beam(tz, act, W=W, blank=blank, cand=cand, bias=bias)


def _compare(out, b, hyps, dtype, what):
    """Utterance b of ``out`` against the oracle's list: counts, tokens and frames exact and in order, logp and token_lp
    within the bounds, nothing behind the counts.  Returns (max |logp err|, max |token_lp err|)."""
    tokens, frames, tlp, ntok, nhyp, logp = [t[b].cpu().numpy() for t in out]
    W, T = tokens.shape
    assert int(nhyp) == len(hyps), (what, int(nhyp), len(hyps))
    assert not np.isnan(tlp).any() and not np.isnan(logp).any(), what
    e_logp = e_tlp = 0.0
    for h, hyp in enumerate(hyps):
        n = len(hyp.tokens)
        assert int(ntok[h]) == n, (what, h)
        assert tokens[h, :n].tolist() == hyp.tokens, (what, h)
        assert frames[h, :n].tolist() == hyp.frames, (what, h)
        assert (tokens[h, n:] == -1).all() and (frames[h, n:] == -1).all() and (tlp[h, n:] == 0).all(), (what, h)
        if dtype == "f32":
            np.testing.assert_allclose(logp[h], hyp.logp, rtol=1e-5, atol=1e-4, err_msg=str((what, h)))
        else:
            np.testing.assert_allclose(logp[h], hyp.logp, rtol=1e-4, atol=0, err_msg=str((what, h)))
        e_logp = max(e_logp, abs(logp[h] - hyp.logp))
        if n:
            err = np.abs(tlp[h, :n].astype(np.float64) - np.array(hyp.token_lp)).max()
            assert err <= (1e-5 if dtype == "f32" else 1e-3), (what, h, err)
            e_tlp = max(e_tlp, err)
    for h in range(len(hyps), W):
        assert int(ntok[h]) == 0 and logp[h] == -np.inf and (tokens[h] == -1).all() and (frames[h] == -1).all()
    assert (np.diff(logp[:len(hyps)]) <= 0).all(), what
    return e_logp, e_tlp


@pytest.mark.parametrize("shape", BR.SHAPES, ids=["%dx%dx%dx%d" % s for s in BR.SHAPES])
@DTYPES
def test_shapes_against_the_oracle_and_run_to_run(hip_lib, shape, dtype):
    """Every shape of the table, with an utterance of no frames (all rows NaN) beside it: the lists are the oracle's,
    the empty utterance gives the empty prefix with logp 0, and two runs are bit-identical."""
    z, hyps, margin, nodes = BR.case(shape, dtype)
    T, V, W, cand = shape
    out = _search([z, z[:0]], dtype, W, cand)
    e_logp, e_tlp = _compare(out, 0, hyps, dtype, shape)
    _compare(out, 1, [BR.Hyp([], [], [], 0.0)], dtype, (shape, "empty"))
    assert out[5][1, 0].item() == 0.0
    print("ctc beam", shape, dtype, "nodes %d, margin %.3g / %.3g: max logp err %.3g (|logp| %.4g), max token_lp err %.3g"
          % (nodes, margin[0], margin[1], e_logp, abs(hyps[0].logp), e_tlp))
    again = _search([z, z[:0]], dtype, W, cand)
    for a, b in zip(out, again):
        assert torch.equal(a, b)


@DTYPES
def test_ragged_batch_with_an_empty_and_a_one_frame_utterance(hip_lib, dtype):
    r = BR.RAGGED
    zs, want = [], []
    for Tb, seed in zip(r["T"], r["seeds"][dtype]):
        z, hyps, _, _ = BR.case((Tb, r["V"], r["W"], r["cand"]), dtype, seed)
        zs.append(z)
        want.append(hyps)
    assert [len(h) for h in want] == [r["W"], 1, r["W"]]
    out = _search(zs, dtype, r["W"], r["cand"])
    errs = [_compare(out, b, want[b], dtype, ("ragged", b)) for b in range(len(zs))]
    print("ctc beam ragged", dtype, "max logp err %.3g, max token_lp err %.3g" % tuple(np.max(errs, axis=0)))


@DTYPES
def test_unpruned_w32_equals_the_oracle_and_the_loss_kernel(hip_lib, dtype):
    """V = 3, T = 5, W = 32, cand = 2: nothing is cut, the list is all 25 prefixes with a path.  -logp of every returned
    prefix equals CTCLoss(reduction='none') on the same logits with that prefix as labels, within the cost bound."""
    from edgedict_amd.loss import CTCLoss
    shape = BR.UNPRUNED
    z, hyps, _, _ = BR.case(shape, dtype, BR.UNPRUNED_SEED[dtype])
    assert len(hyps) == 25
    out = _search([z], dtype, shape[2], shape[3])
    e_logp, e_tlp = _compare(out, 0, hyps, dtype, "unpruned")
    tokens, ntok, logp = out[0][0].cpu().numpy(), out[3][0].cpu().numpy(), out[5][0].cpu().numpy()
    n, U = 25, int(ntok.max())
    labels = np.where(tokens[:n, :U] < 0, 1, tokens[:n, :U]).astype(np.int32)
    tz = torch.tensor(z, device="cuda").to(_TORCH[dtype])[None].expand(n, -1, -1).contiguous()
    costs = CTCLoss(blank=0, reduction="none", check_lengths=False)(
        tz, torch.tensor(labels, device="cuda"), torch.full((n,), shape[0], dtype=torch.int32, device="cuda"),
        torch.tensor(ntok[:n].astype(np.int32), device="cuda")).cpu().numpy()
    err = np.abs(costs + logp[:n]).max()
    print("ctc beam unpruned", dtype, "max logp err %.3g, vs CTCLoss %.3g, sum p %.9f" % (e_logp, err, np.exp(logp[:n]).sum()))
    if dtype == "f32":
        np.testing.assert_allclose(-logp[:n], costs, rtol=1e-5, atol=1e-4)
    else:
        np.testing.assert_allclose(-logp[:n], costs, rtol=1e-4, atol=0)


@DTYPES
def test_ties_go_to_the_lower_canonical_index(hip_lib, dtype):
    """z = 0, V = 3, T = 1: the stay of the empty prefix, [1] and [2] have bit-equal scores by symmetry."""
    z = np.zeros((1, 3), dtype=np.float32)
    for W, want in ((1, [[]]), (2, [[], [1]]), (3, [[], [1], [2]])):
        hyps = BR.search_one(z, W, 2)[0]
        assert [h.tokens for h in hyps] == want
        out = _search([z], dtype, W, 2)
        _compare(out, 0, hyps, dtype, ("tie", W))
        assert len(set(out[5][0, :W].tolist())) == 1                   # bit-equal scores on the device too


@pytest.mark.parametrize("shape", BR.BIAS_SHAPES, ids=["%dx%dx%dx%d" % s for s in BR.BIAS_SHAPES])
@DTYPES
def test_biasing_on_the_device(hip_lib, shape, dtype):
    """A three-phrase graph drawn from the oracle's unbiased top-1 tokens: the biased lists are the oracle's (its margin
    with the bias on is re-checked in test_ctc_beam_host.py), logp includes graph.score(tokens); an empty graph and
    bias=None run the plain kernel: torch.equal."""
    T, V, W, cand = shape
    z, plain, _, _ = BR.case(shape, dtype, BR.BIAS_SEEDS[dtype][shape])
    g = _graph(BR.phrases_from(plain[0].tokens), BR.BIAS_BOOST, V)
    biased, mb, _ = BR.search_one(z, W, cand, graph=g)
    assert mb[0 if dtype == "f32" else 1] >= BR.MARGIN
    assert [h.tokens for h in biased] != [h.tokens for h in plain]
    out = _search([z, z[:0]], dtype, W, cand, bias=g)
    e_logp, e_tlp = _compare(out, 0, biased, dtype, (shape, "bias"))
    _compare(out, 1, [BR.Hyp([], [], [], 0.0)], dtype, (shape, "bias", "empty"))
    assert max(g.score(h.tokens) for h in biased) > 0
    print("ctc beam bias", shape, dtype, "max logp err %.3g, max token_lp err %.3g, top bias %.3g"
          % (e_logp, e_tlp, g.score(biased[0].tokens)))
    base = _search([z, z[:0]], dtype, W, cand)
    _compare(base, 0, plain, dtype, (shape, "plain"))
    for other in (_search([z, z[:0]], dtype, W, cand, bias=_graph([], 1.0, V)),
                  _search([z, z[:0]], dtype, W, cand, bias=None)):
        for a, b in zip(base, other):
            assert torch.equal(a, b)
    # boosts of 0: the bias kernel, the plain decisions
    zero = _search([z, z[:0]], dtype, W, cand, bias=_graph(BR.phrases_from(plain[0].tokens), 0.0, V))
    for a, b in zip(base, zero):
        assert torch.equal(a, b)


# --------------------------------------------------------------------------------------------------- model level
@functools.lru_cache(maxsize=None)
def _tiny():
    from oracle import models_ref as M
    from oracle.make_golden import CASES
    cfg, B, T0, U, seed = CASES["tiny"]
    return cfg, M.make_state_dict(cfg, seed), M.make_batch(cfg, seed + 1, B, T0, U)


@pytest.mark.parametrize("cd", ["fp32", "bf16"])
def test_model_search_is_the_search_of_its_own_head_logits(hip_lib, cd):
    """The tiny LSTM model with a head: Transducer.ctc_beam_search = loss.ctc_prefix_beam on the model's own head logits
    (tokens, frames, token_logp, logp, ranked), with and without a bias list; a model without a head raises."""
    from edgedict_amd.loss import ctc_prefix_beam
    from edgedict_amd.models import Transducer
    cfg, sd, (xs, ys, xlen, ylen) = _tiny()
    torch.manual_seed(11)
    m = Transducer(enc_dropout=0.0, dec_dropout=0.0, ctc_weight=0.3, **cfg)
    m.load_state_dict(sd, strict=False)
    m = m.cuda().eval()
    m.compute_dtype = cd
    V = cfg["vocab_size"]
    with torch.no_grad():
        h_enc, _ = m.encoder(xs[:, :int(xlen.max())].contiguous().cuda())
        act = m.scale_length(h_enc, xlen).to(device="cuda", dtype=torch.int32).contiguous()
        logits = m._ctc_logits(h_enc).contiguous()
    for bias in (None, _graph([[5, 6], [7]], 1.0, V)):
        res = m.ctc_beam_search(xs.cuda(), xlen, W=4, cand=8, bias=bias)
        tokens, frames, tlp, ntok, nhyp, logp = [t.cpu().numpy() for t in ctc_prefix_beam(logits, act, 4, m.blank, 8, bias)]
        assert len(res) == xs.shape[0]
        for b, r in enumerate(res):
            assert len(r) == int(nhyp[b]) >= 1
            assert (r.logp == logp[b, :len(r)]).all() and (np.diff(r.logp) <= 0).all()
            for h in range(len(r)):
                n = int(ntok[b, h])
                assert r.tokens[h].dtype == np.int64 and r.tokens[h].tolist() == tokens[b, h, :n].tolist()
                assert r.frames[h].tolist() == frames[b, h, :n].tolist()
                assert (r.token_logp[h] == tlp[b, h, :n].astype(np.float64)).all()
                assert (r.frames[h] < int(act[b])).all()
    plain = Transducer(enc_dropout=0.0, dec_dropout=0.0, **cfg).cuda().eval()
    with pytest.raises(RuntimeError, match="no CTC head"):
        plain.ctc_beam_search(xs.cuda(), xlen)
