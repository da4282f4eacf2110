"""GPU: contextual biasing in the batched, N-best and streaming beam searches (csrc/decode.hip beam_pop[_detail]_bias,
beam_expand[_lm]_bias) against the CPU oracle tests/bias_ref.py, whose automaton is a brute-force restatement
(pinned against ``ContextGraph`` by tests/test_bias_host.py).  fp32 compute dtype throughout (the token-exact mode).

Models: the trained tiny model of tests/golden/beam_tiny.npz in the two configurations tests/test_lm_fusion_gpu.py
uses - ``CFG`` (V = 40: the composed step kernels) as stored, and ``CFG32`` (V = 64, every width a multiple of 32: the
fused step kernels), which is the same trained model zero-padded to the wider shapes (``_widen``: padded LSTM units
stay at h = c = 0, padded joint units at tanh(0) = 0, the 24 new tokens get logit -30), so that both have a peaked
output.  (A random model of either shape is nearly flat: every token costs about log V, so any boost large enough to
change the output pays for a token outright and the search never stops.)

Phrases (``_phrases``): token bigrams of the plain search's own W = 3 N-best list on the fixture that are not its best
hypothesis' end - [12 38 5 34] (utterance 0, rank 2), [26 36 22] (utterance 1, rank 2), [21 8 27] (utterance 2, rank
3) - and two phrases that match only partially ([26 36 22 V-1], [12 38 5 V-1 1]).  On the CPU oracle alone (asserted
in ``_cap`` before any GPU result is looked at): at ``BIG`` = 2.0 utterance 2 returns [21 8 27] instead of [21 8]; at
``SMALL`` = 0.75 utterance 1 pops hypotheses that gave a pending bonus back (11 of them without an LM, 4 with).
Scores are compared at the fp32 tolerance of tests/test_lm_fusion_gpu.py (2e-4); tokens and expansion counts exactly."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import bias_ref as R                                     # noqa: E402
import test_lm_fusion_gpu as F                           # noqa: E402

pytestmark = pytest.mark.gpu
G = F.G
CFGS = {"composed": F.CFG, "fused": F.CFG32}
XLEN = torch.tensor([21, 13, 19], dtype=torch.int32)     # ragged
BIG, SMALL = 2.0, 0.75
TOL = dict(rtol=2e-4, atol=2e-4)
LM_KW = dict(lm_weight=0.3, length_bonus=0.0)
EM = 64


def _pad(t, shape, fill=0.0):
    out = torch.full(shape, fill, dtype=t.dtype)
    out[tuple(slice(0, n) for n in t.shape)] = t
    return out


def _gates(t, H2, in2=None):
    """An LSTM parameter [4H, in] / [4H] padded per gate block to [4 H2, in2] / [4 H2]."""
    H = t.shape[0] // 4
    if t.dim() == 1:
        return _pad(t.reshape(4, H), (4, H2)).reshape(4 * H2)
    return _pad(t.reshape(4, H, t.shape[1]), (4, H2, in2)).reshape(4 * H2, in2)


def _widen(sd, cfg):
    """The CFG model as a CFG32 model computing the same function (module docstring)."""
    V, E, P, H, P2, J = (cfg["vocab_size"], cfg["vocab_embed_size"], cfg["enc_proj_size"], cfg["dec_hidden_size"],
                         cfg["dec_proj_size"], cfg["joint_size"])
    out = {k: v.clone() for k, v in sd.items()}
    out["encoder.proj.weight"] = _pad(sd["encoder.proj.weight"], (P, sd["encoder.proj.weight"].shape[1]))
    out["encoder.proj.bias"] = _pad(sd["encoder.proj.bias"], (P,))
    out["decoder.embed.weight"] = _pad(sd["decoder.embed.weight"], (V, E))
    for l, width in ((0, E), (1, H)):
        out["decoder.lstm.weight_ih_l%d" % l] = _gates(sd["decoder.lstm.weight_ih_l%d" % l], H, width)
        out["decoder.lstm.weight_hh_l%d" % l] = _gates(sd["decoder.lstm.weight_hh_l%d" % l], H, H)
        out["decoder.lstm.bias_ih_l%d" % l] = _gates(sd["decoder.lstm.bias_ih_l%d" % l], H)
        out["decoder.lstm.bias_hh_l%d" % l] = _gates(sd["decoder.lstm.bias_hh_l%d" % l], H)
    out["decoder.proj.weight"] = _pad(sd["decoder.proj.weight"], (P2, H))
    out["decoder.proj.bias"] = _pad(sd["decoder.proj.bias"], (P2,))
    w0 = sd["joint.joint.0.weight"]
    p0, j0 = sd["encoder.proj.weight"].shape[0], w0.shape[0]
    j = torch.zeros(J, P + P2)
    j[:j0, :p0] = w0[:, :p0]
    j[:j0, P:P + w0.shape[1] - p0] = w0[:, p0:]
    out["joint.joint.0.weight"] = j
    out["joint.joint.0.bias"] = _pad(sd["joint.joint.0.bias"], (J,))
    out["joint.joint.2.weight"] = _pad(sd["joint.joint.2.weight"], (V, J))
    out["joint.joint.2.bias"] = _pad(sd["joint.joint.2.bias"], (V,), -30.0)
    return out


@functools.lru_cache(None)
def _sd(path):
    sd = F._golden_sd()
    return sd if path == "composed" else _widen(sd, F.CFG32)


@functools.lru_cache(None)
def _model(path):
    return F._engine(_sd(path), "fp32", CFGS[path])


@functools.lru_cache(None)
def _lm_sd(path):
    return F._lm_sd(*((40, 16, 32, 2) if path == "composed" else (64, 32, 64, 2)), seed=11, scale=3.0)


@functools.lru_cache(None)
def _lm(path):
    return F._lm(_lm_sd(path))


def _phrases(V):
    return [[12, 38], [38, 5], [5, 34], [26, 36], [36, 22], [21, 8], [8, 27], [26, 36, 22, V - 1],
            [12, 38, 5, V - 1, 1]]


def _edge_phrases(V):
    """The shapes at which the kernels can go wrong: state [21] has exceptions at token 1 (next to blank) and V - 1;
    a phrase longer than any utterance's token count; more than 256 states (more than one pass of a 256-thread
    block over a table would be needed if anything were per state); leaves whose exception row is empty."""
    rng = np.random.default_rng(5)
    fill = [[int(k) for k in rng.integers(4, V, size=3)] for _ in range(140)]
    return (_phrases(V) + [[21, 1], [21, V - 1], [21, 8, 1], [12, 38, 5, 34, 20] + [4, 5, 6, 7] * 5] + fill)


def _xs():
    return torch.from_numpy(G["xs"])


@functools.lru_cache(None)
def _ref(path, W, boost, with_lm, edge=False):
    """The oracle, once per case: (per-utterance results, total expansions, BruteBias or None)."""
    V = CFGS[path]["vocab_size"]
    bb = None if boost is None else R.BruteBias(_edge_phrases(V) if edge else _phrases(V), boost)
    kw = dict(lm=F.RefLM(_lm_sd(path)), **LM_KW) if with_lm else {}
    res, n = R.bias_beam(_sd(path), _xs(), XLEN, W, bb, **kw)
    return res, n, bb


def _graph(path, boost, edge=False):
    from edgedict_amd.bias import ContextGraph
    V = CFGS[path]["vocab_size"]
    return ContextGraph(_edge_phrases(V) if edge else _phrases(V), boost, V)


def _cap(path, with_lm):
    """What keeps the comparisons from being vacuous, asserted on the ORACLE ALONE: the big boost changes the tokens
    of at least one utterance, the small one makes popped hypotheses give a pending bonus back, and two utterances
    are in different automaton states at the same lockstep iteration."""
    plain = R.best(_ref(path, 3, None, with_lm)[0])[0]
    big = _ref(path, 3, BIG, with_lm)[0]
    assert any(not np.array_equal(a, b) for a, b in zip(R.best(big)[0], plain))
    small = _ref(path, 3, SMALL, with_lm)[0]
    assert sum(r["retractions"] for r in small) > 0
    keys = set(big[0]["trace"]) & set(big[1]["trace"])
    assert any(big[0]["trace"][k] != big[1]["trace"][k] for k in keys)


def _fuse(path, with_lm):
    return dict(lm=_lm(path), **LM_KW) if with_lm else {}


def _search(path, W, with_lm, bias):
    from edgedict_amd import decode
    m = _model(path)
    with torch.no_grad():
        seqs, sc = m.beam_search(_xs().cuda(), XLEN, W=W, max_expansions=EM, bias=bias, **_fuse(path, with_lm))
    return seqs, sc, decode.beam_search_batch.last_expansions


# ---------------------------------------------------------------------------------------------------- (a) no bias
@pytest.mark.parametrize("with_lm", [False, True])
@pytest.mark.parametrize("path", ["composed", "fused"])
def test_no_list_empty_list_and_zero_boosts_are_bit_equal_to_the_plain_search(hip_lib, path, with_lm):
    from edgedict_amd.bias import ContextGraph
    V = CFGS[path]["vocab_size"]
    m = _model(path)
    for W in (1, 3):
        with torch.no_grad():
            s0, c0 = m.beam_search(_xs().cuda(), XLEN, W=W, max_expansions=EM, **_fuse(path, with_lm))
        from edgedict_amd import decode
        e0 = decode.beam_search_batch.last_expansions
        zero = ContextGraph(_phrases(V), 0.0, V)
        assert not zero.empty
        for bias in (None, ContextGraph([], 1.0, V), zero):
            s1, c1, e1 = _search(path, W, with_lm, bias)
            F._same(s1, c1, s0, c0)
            assert e1 == e0


# ---------------------------------------------------------------------------------------------------- (b) offline
@pytest.mark.parametrize("boost", [BIG, SMALL])
@pytest.mark.parametrize("W", [1, 3])
@pytest.mark.parametrize("with_lm", [False, True])
@pytest.mark.parametrize("path", ["composed", "fused"])
def test_offline_biased_search_matches_the_oracle(hip_lib, path, with_lm, W, boost):
    _cap(path, with_lm)
    res, rexp, _ = _ref(path, W, boost, with_lm)
    rs, rsc = R.best(res)
    seqs, sc, nexp = _search(path, W, with_lm, _graph(path, boost))
    print("oracle", [a.tolist() for a in rs], rsc, rexp, "gpu", [a.tolist() for a in seqs], sc.numpy(), nexp)
    for a, b in zip(seqs, rs):
        assert np.array_equal(a, b), (a, b)
    np.testing.assert_allclose(sc.numpy(), rsc, **TOL)
    assert nexp == rexp


# ---------------------------------------------------------------------------------------------------- (c) N-best
@pytest.mark.parametrize("with_lm", [False, True])
@pytest.mark.parametrize("path", ["composed", "fused"])
def test_nbest_entry_zero_is_the_search_and_increments_add_up(hip_lib, path, with_lm):
    _cap(path, with_lm)
    W = 3
    for boost in (BIG, SMALL):
        res, rexp, bb = _ref(path, W, boost, with_lm)
        g = _graph(path, boost)
        seqs, sc, nexp = _search(path, W, with_lm, g)
        with torch.no_grad():
            nb = _model(path).beam_search_nbest(_xs().cuda(), XLEN, W=W, max_expansions=EM, bias=g,
                                                **_fuse(path, with_lm))
        for b, (r, want) in enumerate(zip(nb, res)):
            assert np.array_equal(r.tokens[0], seqs[b]) and r.logp[0] == -sc[b].item()       # bit for bit
            assert len(r) == len(want["B"])
            for i, h in enumerate(want["B"]):
                assert np.array_equal(r.tokens[i], np.asarray(h["tokens"], dtype=np.int64))
                assert np.array_equal(r.frames[i], np.asarray(h["frames"], dtype=np.int32))
                np.testing.assert_allclose(r.logp[i], h["logp"], **TOL)
                np.testing.assert_allclose(r.token_logp[i], np.asarray(h["token_logp"], dtype=np.float64), **TOL)
                blanks = h["logp"] - float(np.sum(h["token_logp"]))
                np.testing.assert_allclose(r.token_logp[i].sum() + blanks, r.logp[i], **TOL)
                assert bb.score(h["tokens"]) == g.score(h["tokens"])


# ---------------------------------------------------------------------------------------------------- (d) streaming
def _offline_rows(m, rows, P, lens, W, **kw):
    from edgedict_amd import decode
    S = rows[0].shape[0]
    E1 = torch.cat(rows, dim=1).reshape(-1, rows[0].shape[2]).contiguous()
    return decode.beam_search_rows(m, E1, S, E1.shape[0] // S, P, lens, W=W, max_expansions=EM, **kw)


def _offline_nbest_rows(m, rows, P, lens, W, **kw):
    from edgedict_amd import decode
    S = rows[0].shape[0]
    E1 = torch.cat(rows, dim=1).reshape(-1, rows[0].shape[2]).contiguous()
    return decode.beam_search_nbest_rows(m, E1, S, E1.shape[0] // S, P, lens, W=W, max_expansions=EM, **kw)


@pytest.mark.parametrize("detail", [False, True])
@pytest.mark.parametrize("with_lm", [False, True])
@pytest.mark.parametrize("path", ["composed", "fused"])
def test_streaming_equals_the_offline_biased_search_after_every_chunk(hip_lib, path, with_lm, detail):
    """Chunks of 1, 2 and 3 frames over ragged streams (stream 1 ends after 13 frames, an odd count: the settle path;
    a chunk of 2 or 3 leaves odd counts on the way), a node capacity that makes compaction commit tokens while
    partial matches are pending, and a reset in mid-utterance with ``set_bias`` to another list."""
    from edgedict_amd import decode
    _cap(path, with_lm)
    m = _model(path)
    fuse = _fuse(path, with_lm)
    with torch.no_grad():
        enc, _ = m.encoder(_xs().cuda())
    enc = enc.contiguous()
    S, T, P = enc.shape
    lens_all = np.asarray(R.M.scale_length(T, XLEN), dtype=np.int64)
    W = 3
    first, second = _graph(path, BIG), _graph(path, SMALL)
    V = CFGS[path]["vocab_size"]
    brute = (R.BruteBias(_phrases(V), BIG), R.BruteBias(_phrases(V), SMALL))
    committed_early = pending_at_commit = 0
    for chunk in (1, 2, 3):
        NC = 3 * EM + 64
        sb = decode.StreamingBeamSearch(m, S, W=W, max_expansions=EM, node_capacity=NC, detail=detail, bias=first,
                                        **fuse)
        for phase, g, t_end in ((0, first, 7), (1, second, T)):
            if phase == 1:
                with pytest.raises(ValueError, match="frames"):
                    sb.set_bias(second)
                sb.reset()
                sb.set_bias(second)
            rows, done, before = [], np.zeros(S, dtype=np.int64), [0] * S
            for t in range(0, t_end, chunk):
                n = min(chunk, t_end - t)
                nf = np.clip(lens_all - t, 0, n).astype(np.int32)
                piece = enc[:, t:t + n].contiguous()
                rows.append(sb.joint_rows(piece).reshape(S, n, -1))
                sb.advance(piece, nf)
                done += nf
                got, gsc = sb.best()
                want, wsc = _offline_rows(m, rows, P, done.astype(np.int32), W, bias=g, **fuse)
                F._same(got, gsc, want, wsc)
                assert int(sb.expansions().sum()) == decode.beam_search_batch.last_expansions
                # compaction committed tokens in this advance while, by the oracle's automaton, the stream's first
                # survivor is in the middle of a phrase (a non-root state): the pending bonus rides on the survivor
                ncom = [len(c) for c in sb.committed()]
                for st in range(S):
                    if nf[st] and ncom[st] > before[st]:
                        committed_early += 1
                        if brute[phase].state(got[st].tolist()) != () and brute[phase].held_pend(
                                brute[phase].state(got[st].tolist()))[1] > 0:
                            pending_at_commit += 1
                before = ncom
                if detail:
                    nb = sb.nbest()
                    wnb = _offline_nbest_rows(m, rows, P, done.astype(np.int32), W, bias=g, **fuse)
                    for a, b in zip(nb, wnb):
                        assert len(a) == len(b) and np.array_equal(a.logp, b.logp)
                        for i in range(len(a)):
                            assert np.array_equal(a.tokens[i], b.tokens[i])
                            assert np.array_equal(a.frames[i], b.frames[i])
                            assert np.array_equal(a.token_logp[i], b.token_logp[i])
    assert committed_early > 0 and pending_at_commit > 0


def test_set_bias_turns_biasing_on_and_off_between_utterances(hip_lib):
    from edgedict_amd import decode
    path = "composed"
    m = _model(path)
    with torch.no_grad():
        enc, _ = m.encoder(_xs().cuda())
    enc = enc.contiguous()
    S, T, P = enc.shape
    g = _graph(path, BIG)
    sb = decode.StreamingBeamSearch(m, S, W=3, max_expansions=EM)
    plain, psc = decode.beam_search_enc(m, enc, None, W=3, max_expansions=EM)
    biased, bsc = decode.beam_search_enc(m, enc, None, W=3, max_expansions=EM, bias=g)
    assert any(not np.array_equal(a, b) for a, b in zip(plain, biased))
    for want, wsc, graph in ((plain, psc, None), (biased, bsc, g), (plain, psc, None), (biased, bsc, g)):
        sb.reset()
        sb.set_bias(graph)
        sb.advance(enc)
        got, gsc = sb.best()
        F._same(got, gsc, want, wsc)


# ---------------------------------------------------------------------------------------------------- (e) edge shapes
@pytest.mark.parametrize("path", ["composed", "fused"])
def test_edge_shapes_match_the_oracle(hip_lib, path):
    V = CFGS[path]["vocab_size"]
    g = _graph(path, BIG, edge=True)
    rows = np.diff(g.row_ptr)
    assert g.n_states > 256
    assert (rows[1:] == 0).any()                                             # a non-root state with an empty row
    s21 = g.goto(0, 21)
    toks = g.exc_tok[g.row_ptr[s21]:g.row_ptr[s21 + 1]].tolist()
    assert toks[0] == 1 and toks[-1] == V - 1                                # next to blank, and the last token
    assert max(len(p) for p in g.phrases) > 21                               # longer than any utterance can emit here
    for W in (1, 3):
        res, rexp, bb = _ref(path, W, BIG, False, True)
        if W == 3:
            visited = set().union(*[set(r["trace"].values()) for r in res])
            assert () in visited and (21,) in visited                        # the empty row and the row above are used
            keys = set(res[0]["trace"]) & set(res[2]["trace"])
            assert any(res[0]["trace"][k] != res[2]["trace"][k] for k in keys)
        rs, rsc = R.best(res)
        seqs, sc, nexp = _search(path, W, False, g)
        for a, b in zip(seqs, rs):
            assert np.array_equal(a, b), (a, b)
        np.testing.assert_allclose(sc.numpy(), rsc, **TOL)
        assert nexp == rexp
