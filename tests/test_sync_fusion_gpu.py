"""GPU: LM shallow fusion and contextual biasing in the frame-synchronous beam search (csrc/decode_sync.hip, the
sync_row_topw_fused / sync_select_fused kernels; decode.sync_beam_search*(lm=, bias=)) against the fp64 oracle
tests/sync_fusion_ref.py (pinned by tests/test_sync_fusion_host.py), against the plain search, and against itself.

Inputs are tests/test_sync_beam_gpu.py's: ``_inputs(name)`` (3 utterances, sharpened state dicts) on CFG (V = 40, composed
prediction and LM steps), CFG32 (V = 64, fused steps) and CFGV (V = 2112, the re-reading top-W).  As there, every
input compared with the oracle first has its smallest selection margin and rank gap asserted >= 2e-3 ON THE ORACLE, ten
times the 2e-4 tolerance.  The working points, found on the oracle alone:
  LM    ``_lm_sd(V, E, H, 2, seed=2, scale=4.0)``, lm_weight 0.6, length_bonus 0.3.  At W = 1 that LM empties every best
        hypothesis, so the LM-only W = 1 cases raise the bonus (CFG 2.5, CFG32 4.0) and hold tokens.
  list  CFG (17, 39) at 2.5;  CFG32 (10, 63) at 2.5;  CFGV (1391, 1506) at 3.5
Measured on the oracle, smallest margin / smallest rank gap / merges per utterance (retractions 0 unless said):
  CFG    LM    W = 1 1.9e-1 / - / 0 0 0     W = 4 2.1e-2 / 6.2e-2 / 2 1 0    W = 10 1.3e-2 / 1.4e-2 / 7 7 0
         list  W = 1 2.1e-2 / - / 0 0 0     W = 4 2.4e-2 / 4.8e-2 / 3 3 0    W = 10 2.06e-3 / 3.3e-2 / 9 8 5
         both  W = 1 3.6e-2 / - / 0 0 0     W = 4 3.1e-3 / 1.9e-1 / 4 4 2    W = 10 1.5e-2 / 5.5e-3 / 7 9 3
  CFG32  LM    W = 1 3.8e-2 / - / 0 0 0     W = 4 2.5e-2 / 1.9e-2 / 2 1 0    W = 10 7.5e-3 / 1.9e-2 / 6 6 2
         list  W = 1 2.3e-3 / - / 0 0 0     W = 4 6.4e-2 / 4.0e-2 / 3 4 3    W = 10 3.9e-3 / 5.3e-2 / 8 8 7
         both  W = 1 1.5e-1 / - / 0 0 0     W = 4 2.8e-2 / 4.4e-1 / 4 4 4    W = 10 7.5e-3 / 1.9e-2 / 9 10 7
  CFGV   LM    W = 4 8.7e-3 / 3.8e-3 / 2 0 0    W = 10 6.3e-3 / 3.8e-3 / 3 0 1
         list  W = 4 1.8e-2 / 1.3e-1 / 4 3 4    W = 10 1.4e-2 / 2.3e-2 / 6 5 7
         both  W = 4 1.1e-2 / 1.2e-1 / 4 4 4    W = 10 2.8e-3 / 1.1e-2 / 8 7 6
  retraction case: CFG32, W = 4, (10, 63) at 1.0: 3.7e-2 / 4.7e-2 / 3 1 4, retractions 1 1 0
The bit equalities run fp32 and bf16; CFG32's kernels work on 16-row tiles and are row-independent."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import sync_fusion_ref as F
from bias_ref import BruteBias
from test_lm_fusion_gpu import RefLM, _lm, _lm_sd
from test_sync_beam_gpu import CFG, CFG32, CFGS, MIN_MARGIN, TOL, _engine, _inputs, _rows, _same_bits

pytestmark = pytest.mark.gpu
LM_DIMS = {"CFG": (40, 16, 32, 2), "CFG32": (64, 32, 64, 2), "CFGV": (2112, 32, 64, 2)}      # ntoken, ninp, nhid, layers
LISTS = {"CFG": ([(17, 39)], 2.5), "CFG32": ([(10, 63)], 2.5), "CFGV": ([(1391, 1506)], 3.5)}
W1_BONUS = {"CFG": 2.5, "CFG32": 4.0}
MODES = ["lm", "list", "both"]


@functools.lru_cache(maxsize=None)
def _lm_state(name):
    return _lm_sd(*LM_DIMS[name], seed=2, scale=4.0)


def _point(name, mode, W, boost=None, lm_bos=1):
    """What a case fuses: (LM keywords or None, (phrases, boost) or None)."""
    lm = None
    if mode in ("lm", "both"):
        bonus = W1_BONUS[name] if (W == 1 and mode == "lm") else 0.3
        lm = dict(lm_weight=0.6, length_bonus=bonus, lm_bos=lm_bos)
    lst = None
    if mode in ("list", "both"):
        lst = (LISTS[name][0], LISTS[name][1] if boost is None else boost)
    return lm, lst


@functools.lru_cache(maxsize=None)
def _reference(name, mode, W, boost=None, lm_bos=1):
    """(ranked lists, info dicts) of the oracle per utterance: computed once, read only."""
    sd, xs, xlen = _inputs(name)
    lm, lst = _point(name, mode, W, boost, lm_bos)
    fusion = F.Fusion(lm=RefLM(_lm_state(name)) if lm else None, bias=BruteBias(*lst) if lst else None, **(lm or {}))
    return F.search(sd, xs, xlen, W, fusion)


def _device_kwargs(name, mode, W, dtype="fp32", boost=None, lm_bos=1):
    from edgedict_amd.bias import ContextGraph
    lm, lst = _point(name, mode, W, boost, lm_bos)
    kw = {}
    if lm:
        kw.update(lm=_lm(_lm_state(name), dtype), **lm)
    if lst:
        kw.update(bias=ContextGraph([list(p) for p in lst[0]], lst[1], CFGS[name][0]["vocab_size"]))
    return kw


def _assert_oracle_is_decisive(infos, W, ref):
    print("margin / gap / merges / retractions:",
          [(i["margin"], i["rank_gap"], i["merges"], i["retractions"]) for i in infos])
    for info in infos:
        assert info["margin"] >= MIN_MARGIN and info["rank_gap"] >= MIN_MARGIN, info
    assert W == 1 or sum(i["merges"] for i in infos) >= 1
    assert any(len(h["tokens"]) > 0 for r in ref for h in r)


def _assert_matches(res, ref):
    assert len(res) == len(ref)
    for b, (r, want) in enumerate(zip(res, ref)):
        assert len(r) == len(want), (b, len(r), len(want))
        for i, h in enumerate(want):
            assert np.array_equal(r.tokens[i], h["tokens"]), (b, i, r.tokens[i], h["tokens"])
            assert np.array_equal(r.frames[i], h["frames"]), (b, i, r.frames[i], h["frames"])
            np.testing.assert_allclose(r.token_logp[i], np.asarray(h["token_logp"], dtype=np.float64), **TOL)
        np.testing.assert_allclose(r.logp, [h["logp"] for h in want], **TOL)


# ------------------------------------------------------------------------------------------- 1. against the oracle
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,W", [("CFG", 1), ("CFG32", 1), ("CFG", 4), ("CFG32", 4), ("CFG", 10), ("CFG32", 10),
                                    ("CFGV", 4), ("CFGV", 10)])
def test_fused_nbest_matches_the_oracle(hip_lib, name, W, mode):
    from edgedict_amd import decode
    cfg = CFGS[name][0]
    sd, xs, xlen = _inputs(name)
    ref, infos = _reference(name, mode, W)
    _assert_oracle_is_decisive(infos, W, ref)
    m = _engine(sd, cfg)
    kw = _device_kwargs(name, mode, W)
    res = m.sync_beam_search_nbest(xs.cuda(), xlen, W=W, **kw)
    _assert_matches(res, ref)
    seqs, scores = decode.sync_beam_search_fusion(m, xs.cuda(), xlen, W=W, **kw)
    for b, r in enumerate(res):
        assert np.array_equal(seqs[b], r.tokens[0]) and scores[b].item() == -r.logp[0]


# ------------------------------------------------------------------------------------------- 2. fusion acts
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["CFG", "CFG32"])
def test_fusion_changes_the_best_hypothesis_as_the_oracle_says(hip_lib, name, mode):
    W = 4
    sd, xs, xlen = _inputs(name)
    ref, infos = _reference(name, mode, W)
    _assert_oracle_is_decisive(infos, W, ref)
    m = _engine(sd, CFGS[name][0])
    plain, _ = m.sync_beam_search(xs.cuda(), xlen, W=W)
    fused, score = m.sync_beam_search(xs.cuda(), xlen, W=W, **_device_kwargs(name, mode, W))
    assert sum(not np.array_equal(a, b) for a, b in zip(plain, fused)) >= 1
    for b, r in enumerate(ref):
        assert np.array_equal(fused[b], r[0]["tokens"]), (b, fused[b], r[0]["tokens"])
    np.testing.assert_allclose(-score.numpy(), [r[0]["logp"] for r in ref], **TOL)


# ------------------------------------------------------------------------------------------- 3. a retraction
def test_a_broken_partial_match_gives_its_bonus_back(hip_lib):
    name, W, boost = "CFG32", 4, 1.0
    sd, xs, xlen = _inputs(name)
    ref, infos = _reference(name, "list", W, boost)
    _assert_oracle_is_decisive(infos, W, ref)
    assert sum(i["retractions"] for i in infos) >= 1
    m = _engine(sd, CFG32)
    _assert_matches(m.sync_beam_search_nbest(xs.cuda(), xlen, W=W, **_device_kwargs(name, "list", W, boost=boost)), ref)


# ------------------------------------------------------------------------------------------- 4. the LM's root token
def test_lm_bos_is_the_lm_root_token(hip_lib):
    name, W = "CFG32", 4
    sd, xs, xlen = _inputs(name)
    m = _engine(sd, CFG32)
    got = {}
    for bos in (1, 5):
        ref, infos = _reference(name, "lm", W, None, bos)
        _assert_oracle_is_decisive(infos, W, ref)
        got[bos] = m.sync_beam_search_nbest(xs.cuda(), xlen, W=W, **_device_kwargs(name, "lm", W, lm_bos=bos))
        _assert_matches(got[bos], ref)
    assert any(not np.array_equal(a.logp, b.logp) for a, b in zip(got[1], got[5]))


# ------------------------------------------------------------------------------------------- 5. bit equalities
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["CFG", "CFG32", "CFGV"])
def test_zero_weight_and_an_empty_list_are_the_plain_search(hip_lib, name, dtype):
    from edgedict_amd.bias import ContextGraph
    cfg = CFGS[name][0]
    sd, xs, xlen = _inputs(name)
    m = _engine(sd, cfg, dtype)
    W = 10
    plain = m.sync_beam_search_nbest(xs.cuda(), xlen, W=W)
    lm = _lm(_lm_state(name), dtype)
    zero = m.sync_beam_search_nbest(xs.cuda(), xlen, W=W, lm=lm, lm_weight=0.0, length_bonus=0.0)
    empty = m.sync_beam_search_nbest(xs.cuda(), xlen, W=W, bias=ContextGraph([], 2.5, cfg["vocab_size"]))
    free = m.sync_beam_search_nbest(xs.cuda(), xlen, W=W, bias=ContextGraph([[5, 6]], 0.0, cfg["vocab_size"]))
    for a, b, c, d in zip(plain, zero, empty, free):
        _same_bits(a, b)
        _same_bits(a, c)
        _same_bits(a, d)            # (a list whose boost is 0 runs the fused kernels and adds 0.0)
    assert sum(len(t) for r in plain for t in r.tokens) > 0


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("B,W", [(3, 10), (1, 32), (2, 4)])
def test_fused_utterance_alone_in_a_batch_behind_a_length_and_again(hip_lib, B, W, dtype):
    """B x W rows 30 (no multiple of the 16-row tile), 32 and 8, with LM and list together."""
    from edgedict_amd import decode
    sd, xs, _ = _inputs("CFG32", 3.0, 5, 17)
    m = _engine(sd, CFG32, dtype)
    kw = _device_kwargs("CFG32", "both", W, dtype)
    E1, T, P = _rows(m, xs[:B])
    lens = np.asarray([T, T - 4, T - 1][:B], dtype=np.int32)
    batch = decode.sync_beam_search_nbest_rows(m, E1.reshape(B * T, -1), B, T, P, lens, W, **kw)
    again = decode.sync_beam_search_nbest_rows(m, E1.reshape(B * T, -1), B, T, P, lens, W, **kw)
    n_tokens = 0
    for b in range(B):
        n = int(lens[b])
        alone = decode.sync_beam_search_nbest_rows(m, E1[b, :n].contiguous(), 1, n, P, None, W, **kw)
        _same_bits(batch[b], alone[0])
        _same_bits(batch[b], again[b])
        assert all((f < n).all() for f in batch[b].frames)
        n_tokens += sum(len(t) for t in batch[b].tokens)
    assert n_tokens > 0


# ------------------------------------------------------------------------------------------- 6. errors
def test_fusion_argument_errors_launch_nothing(hip_lib):
    from edgedict_amd.bias import ContextGraph
    from test_sync_fusion_host import _fake, _structs
    sd, xs, xlen = _inputs("CFG")
    m = _engine(sd, CFG)
    lm40, lm64 = _lm(_lm_state("CFG")), _lm(_lm_state("CFG32"))
    x = xs.cuda()
    with pytest.raises(ValueError, match="ntoken = 64"):
        m.sync_beam_search_nbest(x, xlen, W=4, lm=lm64, lm_weight=0.5)
    with pytest.raises(ValueError, match="needs lm_weight"):
        m.sync_beam_search_nbest(x, xlen, W=4, lm=lm40)
    with pytest.raises(ValueError, match="vocab_size = 64"):
        m.sync_beam_search_nbest(x, xlen, W=4, bias=ContextGraph([[10, 63]], 2.5, 64))
    with pytest.raises(ValueError, match="outside \\[1, 32\\]"):
        m.sync_beam_search_nbest(x, xlen, W=33, lm=lm40, lm_weight=0.5, bias=ContextGraph([[17, 39]], 2.5, 40))
    # null tables through the C ABI: a status and a message
    buf, fake = _fake()
    keep, lm, bias = _structs(fake, null_bias="held")
    from search_abi import make_opts
    assert hip_lib.edgedict_sync_stream_reset(ctypes.byref(make_opts(bias=bias)), 2, 2, 32, 4, 64, 2, None, 0, fake,
                                              None) == -1
    assert b"null bias table pointer" in hip_lib.edgedict_last_error()
    # the search still runs after the refusals
    assert len(m.sync_beam_search_nbest(x, xlen, W=4, lm=lm40, lm_weight=0.5)) == xs.shape[0]
