"""GPU: internal-LM estimation (ILME) in the frame-synchronous beam search (csrc/decode_sync.hip sync_row_topw_ilm,
csrc/decode_fused.hip dec_joint_hidden_ilm; decode.sync_beam_search*(ilm_weight=)) and the internal LM as a scorer
(csrc/ilm_score.hip; Transducer.ilm_logprobs / ilm_score) against the oracle tests/ilme_ref.py (pinned by
tests/test_ilme_host.py), against the search without ILME, and against itself.

Inputs are tests/test_sync_beam_gpu.py's ``_inputs(name)`` on CFG (V = 40, composed step: the internal LM's logits come
from the general kernels on a zero encoder row), CFG32 (V = 64, fused step: one dual-epilogue joint-hidden kernel and the
logits kernel on 2 B W rows) and CFGV (V = 2112, the re-reading top-W).  Every case compared with the oracle first
asserts, ON THE ORACLE, selection margin and rank gap >= 2e-3, ten times the 2e-4 tolerance.  LM and lists are
tests/test_sync_fusion_gpu.py's working points (lm_weight 0.6, length_bonus 0.3; at W = 1 with the LM alone its raised
bonus, CFG 2.5 and CFG32 4.0, without which that LM empties every best hypothesis).  The ILM weights were found on the
oracle alone, on the CPU; ``ILM_W`` holds them.  On CFGV with ILME alone a weight of 0.02 or more removes every merge at
W = 4 (the term is about weight x log V, and 2111 symbols then crowd the blank children out) and no weight from 0.015 to
0.3 keeps the rank gap at W = 10, hence 0.01 there.
Measured on the oracle, smallest margin / smallest rank gap / merges per utterance (no retractions anywhere):
  CFG    ilm          W = 1 3.4e-1 / - / 0 0 0    W = 4 9.3e-3 / 2.5e-2 / 2 1 0    W = 10 9.6e-3 / 4.1e-3 / 4 2 0
         lm+ilm       W = 1 3.3e-1 / - / 0 0 0    W = 4 1.6e-2 / 4.7e-2 / 2 1 0    W = 10 4.3e-3 / 9.9e-3 / 3 4 0
         lm+ilm+list  W = 1 1.2e-1 / - / 0 0 0    W = 4 2.2e-2 / 6.7e-2 / 3 2 0    W = 10 4.2e-3 / 4.8e-2 / 9 8 5
  CFG32  ilm          W = 1 4.3e-2 / - / 0 0 0    W = 4 3.1e-3 / 2.4e-2 / 1 1 0    W = 10 1.0e-2 / 3.2e-3 / 3 1 0
         lm+ilm       W = 1 3.6e-2 / - / 0 0 0    W = 4 2.1e-2 / 2.7e-2 / 1 1 0    W = 10 5.9e-3 / 8.3e-3 / 4 4 1
         lm+ilm+list  W = 1 6.1e-2 / - / 0 0 0    W = 4 7.2e-2 / 1.3e-1 / 4 4 4    W = 10 1.9e-2 / 7.2e-3 / 8 10 8
  CFGV   ilm          W = 4 6.1e-3 / 1.5e-2 / 1 0 0    W = 10 9.7e-3 / 3.2e-3 / 2 0 1
         lm+ilm       W = 4 9.6e-3 / 1.5e-2 / 1 0 0    W = 10 5.9e-3 / 2.4e-3 / 3 0 1
         lm+ilm+list  W = 4 9.1e-2 / 2.4e-2 / 4 4 3    W = 10 1.1e-2 / 9.0e-3 / 10 8 10
Against the LM alone, lm+ilm at W = 4 and weight 0.6 changes the best hypothesis of 3 (CFG) and 2 (CFG32) utterances.
The bit equalities run fp32 and bf16; the fused step's kernels work on 16-row tiles and are row-independent, and with
B W = 12 or 20 rows the internal LM's half of the stacked rows starts inside a tile of the logits kernel."""
import functools

import numpy as np
import pytest
import torch

import ilme_ref as I
import sync_fusion_ref as F
from bias_ref import BruteBias
from oracle import models_ref as M
from test_lm_fusion_gpu import RefLM, _lm
from test_sync_beam_gpu import CFG32, CFGS, TOL, _engine, _inputs, _rows, _same_bits
from test_sync_fusion_gpu import LISTS, W1_BONUS, _assert_matches, _assert_oracle_is_decisive, _lm_state
from test_sync_stream_gpu import _check_best, _check_committed, _chunk, _ragged_chunk

pytestmark = pytest.mark.gpu
MODES = ["ilm", "lm+ilm", "lm+ilm+list"]
ILM_W = {"CFG": {"ilm": {1: 0.3, 4: 0.15, 10: 0.15}, "lm+ilm": {1: 0.2, 4: 0.6, 10: 0.45},
                 "lm+ilm+list": {1: 0.3, 4: 0.6, 10: 0.4}},
         "CFG32": {"ilm": {1: 0.2, 4: 0.15, 10: 0.15}, "lm+ilm": {1: 0.2, 4: 0.6, 10: 0.45},
                   "lm+ilm+list": {1: 0.3, 4: 0.6, 10: 0.4}},
         "CFGV": {"ilm": {4: 0.01, 10: 0.01}, "lm+ilm": {4: 0.1, 10: 0.3}, "lm+ilm+list": {4: 0.3, 10: 0.3}}}


def _point(name, mode, W):
    """What a case fuses: (ILM weight, LM keywords or None, (phrases, boost) or None)."""
    lm = None
    if "lm" in mode.split("+"):
        lm = dict(lm_weight=0.6, length_bonus=W1_BONUS[name] if (W == 1 and mode == "lm+ilm") else 0.3, lm_bos=1)
    return ILM_W[name][mode][W], lm, (LISTS[name] if "list" in mode else None)


@functools.lru_cache(maxsize=None)
def _reference(name, mode, W, ilme=True):
    """(ranked lists, info dicts) of the oracle per utterance: computed once, read only.  ``ilme=False``: the same
    point without the ILM term."""
    sd, xs, xlen = _inputs(name)
    w, lm, lst = _point(name, mode, W)
    fusion = I.Fusion(ilm=I.model_ilm(sd), ilm_weight=w if ilme else None,
                      lm=RefLM(_lm_state(name)) if lm else None, bias=BruteBias(*lst) if lst else None, **(lm or {}))
    return F.search(sd, xs, xlen, W, fusion)


def _device_kwargs(name, mode, W, dtype="fp32", ilme=True):
    from edgedict_amd.bias import ContextGraph
    w, lm, lst = _point(name, mode, W)
    kw = dict(ilm_weight=w) if ilme else {}
    if lm:
        kw.update(lm=_lm(_lm_state(name), dtype), **lm)
    if lst:
        kw.update(bias=ContextGraph([list(p) for p in lst[0]], lst[1], CFGS[name][0]["vocab_size"]))
    return kw


def _assert_route(hip_lib, name, dtype="fp32"):
    """CFG takes the composed step, CFG32 and CFGV the fused one: both routes to the internal LM's logits are covered."""
    cfg = CFGS[name][0]
    code = 0 if dtype == "fp32" else 1
    fused = hip_lib.edgedict_decode_fused_ok(code, 0, cfg["joint_size"], cfg["vocab_size"], cfg["vocab_embed_size"],
                                             cfg["dec_hidden_size"], cfg["dec_proj_size"])
    assert fused == (0 if name == "CFG" else 1)


# ------------------------------------------------------------------------------------------- 1. against the oracle
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,W", [("CFG", 1), ("CFG32", 1), ("CFG", 4), ("CFG32", 4), ("CFG", 10), ("CFG32", 10),
                                    ("CFGV", 4), ("CFGV", 10)])
def test_ilme_nbest_matches_the_oracle(hip_lib, name, W, mode):
    from edgedict_amd import decode
    _assert_route(hip_lib, name)
    sd, xs, xlen = _inputs(name)
    ref, infos = _reference(name, mode, W)
    _assert_oracle_is_decisive(infos, W, ref)
    m = _engine(sd, CFGS[name][0])
    kw = _device_kwargs(name, mode, W)
    res = m.sync_beam_search_nbest(xs.cuda(), xlen, W=W, **kw)
    _assert_matches(res, ref)
    seqs, scores = decode.sync_beam_search_fusion(m, xs.cuda(), xlen, W=W, **kw)
    for b, r in enumerate(res):
        assert np.array_equal(seqs[b], r.tokens[0]) and scores[b].item() == -r.logp[0]


# ------------------------------------------------------------------------------------------- 2. ILME acts
@pytest.mark.parametrize("name", ["CFG", "CFG32"])
def test_ilme_changes_the_best_hypothesis_as_the_oracle_says(hip_lib, name):
    W, mode = 4, "lm+ilm"
    _assert_route(hip_lib, name)
    sd, xs, xlen = _inputs(name)
    ref, infos = _reference(name, mode, W)
    _assert_oracle_is_decisive(infos, W, ref)
    lm_ref, lm_infos = _reference(name, mode, W, False)
    _assert_oracle_is_decisive(lm_infos, W, lm_ref)
    m = _engine(sd, CFGS[name][0])
    lm_only, _ = m.sync_beam_search(xs.cuda(), xlen, W=W, **_device_kwargs(name, mode, W, ilme=False))
    ilme, score = m.sync_beam_search(xs.cuda(), xlen, W=W, **_device_kwargs(name, mode, W))
    assert sum(not np.array_equal(a, b) for a, b in zip(lm_only, ilme)) >= 1
    for b, (r, q) in enumerate(zip(ref, lm_ref)):
        assert np.array_equal(ilme[b], r[0]["tokens"]), (b, ilme[b], r[0]["tokens"])
        assert np.array_equal(lm_only[b], q[0]["tokens"]), (b, lm_only[b], q[0]["tokens"])
    np.testing.assert_allclose(-score.numpy(), [r[0]["logp"] for r in ref], **TOL)


# ------------------------------------------------------------------------------------------- 3. bit equalities
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["CFG", "CFG32", "CFGV"])
def test_weight_zero_runs_the_ilme_kernels_and_changes_no_bit(hip_lib, name, dtype):
    """c - 0 * finite == c: the dual-epilogue hidden kernel (CFG32, CFGV) and the logits kernel on twice the rows leave
    the RNN-T half untouched, and so does the ILM pass of the row kernel."""
    from edgedict_amd.bias import ContextGraph
    _assert_route(hip_lib, name, dtype)
    cfg = CFGS[name][0]
    sd, xs, xlen = _inputs(name)
    m = _engine(sd, cfg, dtype)
    W = 10
    x = xs.cuda()
    forms = [{}, dict(lm=_lm(_lm_state(name), dtype), lm_weight=0.6, length_bonus=0.3),
             dict(bias=ContextGraph([list(p) for p in LISTS[name][0]], LISTS[name][1], cfg["vocab_size"]))]
    n_tokens = 0
    for kw in forms:
        without = m.sync_beam_search_nbest(x, xlen, W=W, **kw)
        zero = m.sync_beam_search_nbest(x, xlen, W=W, ilm_weight=0.0, **kw)
        for a, b in zip(without, zero):
            _same_bits(a, b)
        n_tokens += sum(len(t) for r in without for t in r.tokens)
    assert n_tokens > 0
    acts = m.sync_beam_search_nbest(x, xlen, W=W, ilm_weight=0.3)
    assert any(not np.array_equal(a.logp, b.logp) for a, b in zip(acts, m.sync_beam_search_nbest(x, xlen, W=W)))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("B,W", [(3, 4), (4, 4), (5, 4), (1, 32)])
def test_ilme_utterance_alone_in_a_batch_behind_a_length_and_again(hip_lib, B, W, dtype):
    """B x W = 12, 16, 20 and 32 rows - below, on and above the 16-row tile; at 12 and 20 the internal LM's half of the
    stacked rows starts inside a tile - with LM, list and ILME together, ragged lengths."""
    from edgedict_amd import decode
    sd, xs, _ = _inputs("CFG32", 3.0, 5, 17)
    m = _engine(sd, CFG32, dtype)
    kw = _device_kwargs("CFG32", "lm+ilm+list", 4, dtype)
    E1, T, P = _rows(m, xs[:B])
    lens = np.asarray([T, T - 4, T - 1, T - 2, T - 6][:B], dtype=np.int32)
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


# ------------------------------------------------------------------------------------------- 4. streaming
PAUSES = [[2, 0, 3], [1, 3, 0], [0, 2, 1], [3, 0, 2], [3, 3, 3], [0, 1, 0]]      # tests/test_sync_stream_fusion_gpu.py's


@pytest.mark.parametrize("mode", ["ilm", "lm+ilm+list"])
def test_streaming_ilme_equals_the_offline_search_after_every_chunk(hip_lib, mode):
    from edgedict_amd import decode
    from edgedict_amd.decode import StreamingSyncFusionBeamSearch
    _assert_route(hip_lib, "CFG32")
    W = 4
    sd, xs, _ = _inputs("CFG32", 1.5, 3, 17)
    m = _engine(sd, CFG32)
    kw = _device_kwargs("CFG32", mode, W)
    E1, T, P = _rows(m, xs)
    assert T == 9 and np.sum(PAUSES, axis=0).tolist() == [T] * 3

    def offline(rows, n):
        Sn = rows.shape[0]
        return decode.sync_beam_search_nbest_rows(m, rows[:, :n].contiguous().reshape(Sn * n, rows.shape[2]), Sn, n, P,
                                                  None, W, **kw)

    want = {n: offline(E1, n) for n in range(1, T + 1)}            # computed once, read only
    without = decode.sync_beam_search_nbest_rows(m, E1.reshape(3 * T, -1), 3, T, P, None, W,
                                                 **{k: v for k, v in kw.items() if k != "ilm_weight"})
    assert any(not np.array_equal(a.logp, b.logp) for a, b in zip(want[T], without))       # ILME does something
    assert sum(len(t) for r in want[T] for t in r.tokens) > 0
    sb = StreamingSyncFusionBeamSearch(m, 3, W=W, **kw)
    for split in ([1] * T, [3, 3, 3], [T]):
        sb.reset()
        t = 0
        for n in split:
            sb.advance_rows(_chunk(E1, t, n), P)
            t += n
            res = sb.nbest()
            for s in range(3):
                _same_bits(res[s], want[t][s])
            _check_best(sb, res)
            _check_committed(sb, res)
    # ragged chunks: every stream sits a chunk out while the others take an odd number of frames
    sb.reset()
    pos = [0, 0, 0]
    for nf in PAUSES:
        sb.advance_rows(_ragged_chunk(E1, pos, nf), P, np.asarray(nf, dtype=np.int32))
        pos = [p + n for p, n in zip(pos, nf)]
        res = sb.nbest()
        for s in range(3):
            if pos[s]:
                _same_bits(res[s], want[pos[s]][s])
            else:
                assert len(res[s]) == 1 and len(res[s].tokens[0]) == 0 and res[s].logp[0] == 0.0
        _check_committed(sb, res)
    # a masked reset between utterances: stream 1 starts over, the others are left alone
    mask = torch.tensor([False, True, False])
    sb.reset(mask)
    assert len(sb.nbest()[1].tokens[0]) == 0
    sb.advance_rows(_ragged_chunk(E1, [0, 0, 0], [0, 5, 0]), P, np.asarray([0, 5, 0], dtype=np.int32))
    res = sb.nbest()
    _same_bits(res[1], want[5][1])
    _same_bits(res[0], want[T][0])
    _same_bits(res[2], want[T][2])


# ------------------------------------------------------------------------------------------- 5. the scorer
@functools.lru_cache(maxsize=None)
def _labels(name, U):
    """(state dict, state dict with b2[blank] raised by 10, ys [4, U], ylen): ragged lengths, one of them 0."""
    sd, _, _ = _inputs(name)
    raised = dict(sd)
    raised["joint.joint.2.bias"] = sd["joint.joint.2.bias"].clone()
    raised["joint.joint.2.bias"][M.NUL] += 10.0
    g = torch.Generator().manual_seed(U)
    ys = torch.randint(4, CFGS[name][0]["vocab_size"], (4, U), generator=g, dtype=torch.int32)
    ylen = torch.tensor([U, 0, max(U - 2, 1), 1], dtype=torch.int32)
    return sd, raised, ys, ylen


@pytest.mark.parametrize("name,U,raise_blank", [("CFG", 1, False), ("CFG", 5, False), ("CFG", 5, True),
                                                ("CFG32", 1, False), ("CFG32", 5, False), ("CFG32", 5, True)])
def test_ilm_logprobs_and_score_match_the_oracle(hip_lib, name, U, raise_blank):
    from edgedict_amd import decode
    _assert_route(hip_lib, name)
    sd, raised, ys, ylen = _labels(name, U)
    sd = raised if raise_blank else sd
    want = np.asarray(I.ilm_logprobs(sd, ys, ylen), dtype=np.float64)
    m = _engine(sd, CFGS[name][0])
    got = m.ilm_logprobs(ys, ylen)
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == (4, U)
    again = m.ilm_logprobs(ys.cuda(), ylen.cuda())
    score = m.ilm_score(ys, ylen)
    assert score.is_cuda and tuple(score.shape) == (4,)
    g = got.cpu().numpy()
    assert np.array_equal(g, again.cpu().numpy())                   # no atomics: the same bits every run
    behind = np.arange(U)[None, :] >= ylen.numpy()[:, None]
    assert (g[behind] == 0.0).all() and (g[~behind] < 0.0).all()
    np.testing.assert_allclose(g, want, **TOL)
    np.testing.assert_allclose(score.cpu().numpy(), want.sum(axis=1), rtol=2e-4, atol=2e-4 * U)
    # the raw kernel call: rows of prediction-network output in, fp32 logits [R, V] out; their blank-excluded
    # log-softmax at the labels is what ilm_logprobs returned, up to the three fp32 roundings of
    # (z - m) - log(s) on values below 32 in size (3 x 2^-24 x 32 = 6e-6)
    with torch.no_grad():
        h_dec, _ = m.decoder(ys.cuda())
    z = decode.ilm_logits(m, h_dec[:, :U].reshape(4 * U, -1))
    assert z.dtype == torch.float32 and tuple(z.shape) == (4 * U, CFGS[name][0]["vocab_size"])
    zz = z.double().cpu()
    zz[:, M.NUL] = -float("inf")
    lp = torch.log_softmax(zz, dim=1).gather(1, ys.reshape(-1, 1).long()).reshape(4, U).numpy()
    np.testing.assert_allclose(g[~behind], lp[~behind], rtol=1e-5, atol=1e-5)
    if raise_blank:
        assert (z.argmax(dim=1) == M.NUL).all()                    # the blank owns the maximum of every raw row
