"""GPU: the frame-synchronous beam search (csrc/decode_sync.hip; decode.sync_beam_search*) against its fp64 oracle
tests/sync_beam_ref.py (pinned by tests/test_sync_beam_host.py), against the greedy search at W = 1, and against
itself: an utterance inside a batch / behind its length / in a second run gives the same bits as alone.

Whole-list equality between an fp32 search on the device and the oracle holds only where no choice is a near-tie, so
every input compared exactly has its smallest selection margin (kept W-th candidate minus the first dropped one, over
all frames) and its smallest gap between adjacent final ranks measured on the oracle and asserted >= 2e-3, ten times the
2e-4 score tolerance.  Measured on make_batch(cfg, 4, 3, 9, 4, ragged=False) with the output layer scaled by 6 and the
blank raised by 3 (sync_beam_ref.sharpened), margin / gap / merges per utterance:
    CFG   (V = 40, composed step), state dict seed 4:   W = 1  6.8e-3 / -      / 0 0 0
                                                        W = 4  9.4e-3 / 7.9e-3 / 1 1 0    W = 10  5.3e-3 / 5.6e-3 / 4 4 0
    CFG32 (V = 64, fused step),    state dict seed 0:   W = 1  5.3e-2 / -      / 0 0 0
                                                        W = 4  1.4e-2 / 5.4e-3 / 2 0 0    W = 10  3.9e-3 / 2.6e-3 / 5 4 3
    CFGV  (CFG32 with V = 2112: the top-W kernel's form for V > 2048), state dict seed 5:
                                                        W = 4  1.1e-2 / 1.5e-2 / 1 0 0    W = 10  2.2e-3 / 3.9e-3 / 2 0 1
(W = 1 keeps one candidate per frame: nothing can merge, so a merge is asserted for W > 1 only.)
The bit-equality tests run the fused step (CFG32), whose kernels work on 16-row tiles and are row-independent."""
import functools
import os

import numpy as np
import pytest
import torch

import sync_beam_ref as S
from oracle import models_ref as M

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(os.path.dirname(__file__), "golden", "beam_tiny.npz"))
CFG = dict(vocab_embed_size=16, vocab_size=40, input_size=24, enc_hidden_size=32, enc_layers=2,
           enc_proj_size=24, dec_hidden_size=32, dec_layers=2, dec_proj_size=24, joint_size=32)
# every prediction-network and joint width a multiple of 32: the fused step kernels run
CFG32 = dict(vocab_embed_size=32, vocab_size=64, input_size=24, enc_hidden_size=32, enc_layers=2,
             enc_proj_size=32, dec_hidden_size=64, dec_layers=2, dec_proj_size=32, joint_size=64)
# V = 2112 > 2048: sync_row_topw reads the logits again in every pass instead of keeping a row in registers
CFGV = dict(CFG32, vocab_size=2112)
CFGS = {"CFG": (CFG, 4), "CFG32": (CFG32, 0), "CFGV": (CFGV, 5)}       # config, pinned state dict seed
TOL = dict(rtol=2e-4, atol=2e-4)
MIN_MARGIN = 2e-3


def _engine(sd, cfg, dtype="fp32"):
    from edgedict_amd.models import Transducer
    m = Transducer(enc_dropout=0.0, dec_dropout=0.0, output_loss=False, **cfg)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    m.compute_dtype = dtype
    return m


@functools.lru_cache(maxsize=None)
def _inputs(name, blank_bias=3.0, B=3, T0=9):
    cfg, seed = CFGS[name]
    sd = S.sharpened(M.make_state_dict(cfg, seed), blank_bias=blank_bias)
    xs, _, xlen, _ = M.make_batch(cfg, 4, B, T0, 4, ragged=False)
    return sd, xs, xlen


@functools.lru_cache(maxsize=None)
def _reference(name, W, blank_bias=3.0, T0=9):
    """(ranked lists, info dicts) of the oracle per utterance: computed once, read only."""
    sd, xs, xlen = _inputs(name, blank_bias, 3, T0)
    return S.search(sd, xs, xlen, W)


def _same_bits(a, b):
    assert len(a) == len(b), (len(a), len(b))
    for i in range(len(a)):
        assert np.array_equal(a.tokens[i], b.tokens[i]), (i, a.tokens[i], b.tokens[i])
        assert np.array_equal(a.frames[i], b.frames[i]), (i, a.frames[i], b.frames[i])
        assert np.array_equal(a.token_logp[i], b.token_logp[i]), (i, a.token_logp[i], b.token_logp[i])
    assert np.array_equal(a.logp, b.logp), (a.logp, b.logp)


def _rows(m, xs):
    """(E1 [B, T, J], T, P): the joint's encoder rows of the batch, computed once, so that every search compared bit by
    bit reads the same rows."""
    from edgedict_amd import decode
    with torch.no_grad():
        enc, _ = m.encoder(xs.cuda())
        enc = enc.contiguous()
        B, T, P = enc.shape
        return decode.joint_rows(m, enc).reshape(B, T, -1), T, P


# ------------------------------------------------------------------------------------------- 1. against the oracle
@pytest.mark.parametrize("name,W", [("CFG", 1), ("CFG32", 1), ("CFG", 4), ("CFG32", 4), ("CFG", 10), ("CFG32", 10),
                                    ("CFGV", 4), ("CFGV", 10)])
def test_nbest_matches_the_oracle(hip_lib, name, W):
    from edgedict_amd import decode
    cfg = CFGS[name][0]
    sd, xs, xlen = _inputs(name)
    ref, infos = _reference(name, W)
    print("margin / gap / merges:", [(i["margin"], i["rank_gap"], i["merges"]) for i in infos])
    for info in infos:
        assert info["margin"] >= MIN_MARGIN and info["rank_gap"] >= MIN_MARGIN, info
    assert W == 1 or sum(i["merges"] for i in infos) >= 1
    assert any(len(r[0]["tokens"]) > 0 for r in ref)
    m = _engine(sd, cfg)
    fused = all(cfg[k] % 32 == 0 for k in ("joint_size", "dec_proj_size", "vocab_embed_size", "dec_hidden_size"))
    assert fused == (name != "CFG")         # CFG takes the composed step, the other two the fused one
    res = m.sync_beam_search_nbest(xs.cuda(), xlen, W=W)
    assert len(res) == xs.shape[0]
    for b, (r, want) in enumerate(zip(res, ref)):
        assert len(r) == len(want), (b, len(r), len(want))
        for i, h in enumerate(want):
            assert r.tokens[i].dtype == np.int64 and r.frames[i].dtype == np.int32
            assert np.array_equal(r.tokens[i], h["tokens"]), (b, i, r.tokens[i], h["tokens"])
            assert np.array_equal(r.frames[i], h["frames"]), (b, i, r.frames[i], h["frames"])
            np.testing.assert_allclose(r.token_logp[i], np.asarray(h["token_logp"], dtype=np.float64), **TOL)
        np.testing.assert_allclose(r.logp, [h["logp"] for h in want], **TOL)
    seqs, scores = decode.sync_beam_search(m, xs.cuda(), xlen, W=W)
    assert scores.dtype == torch.float64
    for b, r in enumerate(res):
        assert seqs[b].dtype == np.int64 and np.array_equal(seqs[b], r.tokens[0])
        assert scores[b].item() == -r.logp[0]


# ------------------------------------------------------------------------------------------- 2. W = 1 is greedy
@pytest.mark.parametrize("name", ["CFG", "CFG32"])
def test_width_one_is_greedy_decode_without_blanks(hip_lib, name):
    """Full-length batch, the blank raised by 2 so that the greedy path holds blanks and tokens.  The oracle's margin at
    W = 1 is the greedy search's own gap between the best and the second symbol of a frame."""
    cfg = CFGS[name][0]
    sd, xs, xlen = _inputs(name, 2.0, 3, 12)
    _, infos = _reference(name, 1, 2.0, 12)
    print("margins:", [i["margin"] for i in infos])
    assert all(i["margin"] >= MIN_MARGIN for i in infos), infos
    m = _engine(sd, cfg)
    want, wscore = m.greedy_decode(xs.cuda(), xlen)
    seqs, scores = m.sync_beam_search(xs.cuda(), xlen, W=1)
    assert sum(int((w != M.NUL).sum()) for w in want) > 0 and sum(int((w == M.NUL).sum()) for w in want) > 0
    for b in range(xs.shape[0]):
        assert np.array_equal(seqs[b], want[b][want[b] != M.NUL]), (b, seqs[b], want[b])
    np.testing.assert_allclose(scores.numpy(), wscore.double().cpu().numpy(), **TOL)


# ------------------------------------------------------------------------------------------- 3. row-tile edges
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("B,W", [(3, 4), (4, 4), (5, 4), (1, 32), (2, 10)])
def test_utterance_in_a_batch_equals_the_utterance_alone(hip_lib, B, W, dtype):
    """B x W rows below, on and above the step kernels' 16-row tile: 12, 16, 20, 32, 20."""
    from edgedict_amd import decode
    sd, xs, _ = _inputs("CFG32", 3.0, 5, 9)
    m = _engine(sd, CFG32, dtype)
    E1, T, P = _rows(m, xs[:B])
    batch = decode.sync_beam_search_nbest_rows(m, E1.reshape(B * T, -1), B, T, P, None, W)
    assert len(batch) == B
    n_tokens = 0
    for b in range(B):
        alone = decode.sync_beam_search_nbest_rows(m, E1[b].contiguous(), 1, T, P, None, W)
        _same_bits(batch[b], alone[0])
        n_tokens += sum(len(t) for t in batch[b].tokens)
    assert n_tokens > 0


# ------------------------------------------------------------------------------------------- 4. ragged lengths
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_utterance_behind_its_length_equals_its_frames_alone(hip_lib, dtype):
    from edgedict_amd import decode
    sd, xs, _ = _inputs("CFG32", 3.0, 5, 17)
    xlen = torch.tensor([17, 9, 17, 3, 12], dtype=torch.int32)
    m = _engine(sd, CFG32, dtype)
    E1, T, P = _rows(m, xs)
    lens = m.scale_length(E1, xlen).numpy().astype(np.int32)
    assert lens.max() == T and len(set(lens.tolist())) >= 4
    W = 4
    batch = decode.sync_beam_search_nbest_rows(m, E1.reshape(5 * T, -1), 5, T, P, lens, W)
    for b in range(5):
        n = int(lens[b])
        alone = decode.sync_beam_search_nbest_rows(m, E1[b, :n].contiguous(), 1, n, P, None, W)
        _same_bits(batch[b], alone[0])
        assert all((f < n).all() for f in batch[b].frames)
    # the public entry point applies the same lengths
    res = m.sync_beam_search_nbest(xs.cuda(), xlen, W=W)
    for b in range(5):
        _same_bits(res[b], batch[b])


# ------------------------------------------------------------------------------------------- 5. determinism
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["CFG", "CFG32"])
def test_two_runs_give_the_same_bits(hip_lib, name, dtype):
    cfg = CFGS[name][0]
    sd, xs, xlen = _inputs(name)
    m = _engine(sd, cfg, dtype)
    first = m.sync_beam_search_nbest(xs.cuda(), xlen, W=10)
    second = m.sync_beam_search_nbest(xs.cuda(), xlen, W=10)
    for a, b in zip(first, second):
        _same_bits(a, b)


# ------------------------------------------------------------------------------------------- 6. the N-best's shape
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_nbest_shape(hip_lib, dtype):
    import types
    from edgedict_amd import decode
    sd, xs, _ = _inputs("CFG32", 3.0, 5, 17)
    xlen = torch.tensor([17, 9, 17, 3, 12], dtype=torch.int32)
    m = _engine(sd, CFG32, dtype)
    W = 10
    res = m.sync_beam_search_nbest(xs.cuda(), xlen, W=W)
    seqs, scores = m.sync_beam_search(xs.cuda(), xlen, W=W)
    with torch.no_grad():
        enc, _ = m.encoder(xs.cuda())
    lens = m.scale_length(enc, xlen).numpy()
    for b, r in enumerate(res):
        assert 1 <= len(r) <= W and r.logp.dtype == np.float64 and r.logp.shape == (len(r),)
        assert len({tuple(t.tolist()) for t in r.tokens}) == len(r)             # distinct sequences
        assert (np.diff(r.logp) <= 0).all() and np.isfinite(r.logp).all()
        for t, f, l in zip(r.tokens, r.frames, r.token_logp):
            assert t.dtype == np.int64 and f.dtype == np.int32 and l.dtype == np.float64
            assert len(t) == len(f) == len(l) <= lens[b]
            assert ((t > 0) & (t < CFG32["vocab_size"])).all()
            assert (np.diff(f) >= 0).all() and ((f >= 0) & (f < lens[b])).all()
            assert (l <= 0).all()
        assert np.array_equal(seqs[b], r.tokens[0]) and scores[b].item() == -r.logp[0]
    flags = types.SimpleNamespace(hop_length=200, downsample=3, sample_rate=16000)
    times = decode.emission_times(res[0].frames[0], flags)               # 75 ms per encoder frame
    assert times.tolist() == [0.075 * int(f) for f in res[0].frames[0]]


# ------------------------------------------------------------------------------------------- 7. the old search
@pytest.mark.parametrize("W", [4, 10])
def test_best_first_search_is_untouched(hip_lib, W):
    from edgedict_amd import decode
    sd = {k[3:]: torch.from_numpy(G[k]) for k in G.files if k.startswith("sd/")}
    m = _engine(sd, CFG)
    with torch.no_grad():
        seqs, scores = m.beam_search(torch.from_numpy(G["xs"]).cuda(), torch.from_numpy(G["xlen"]), W=W)
    for b, s in enumerate(seqs):
        assert np.array_equal(s, G["W%d_seq%d" % (W, b)]), (W, b, s)
    np.testing.assert_allclose(scores.numpy(), G["W%d_score" % W], **TOL)
    assert decode.beam_search_batch.last_expansions == int(G["W%d_expansions" % W][0])
