"""GPU: the back-off n-gram fused into the frame-synchronous beam search (csrc/decode_sync.hip: sync_row_topw_ngram builds a
row's n-gram image in LDS, sync_select_fused carries the per-row state; decode.sync_beam_search*(lm=NGramLM), offline and
streaming) against the fp64 oracle - tests/sync_fusion_ref.py / ilme_ref.py through tests/sync_ngram_ref.py's adapter -,
against the plain search, and against itself.

Inputs are tests/test_sync_beam_gpu.py's ``_inputs(name)`` on CFG (V = 40, composed steps), CFG32 (V = 64, fused steps)
and CFGV (V = 2112: the re-reading top-W, an LDS image filled over 9 strides of 256 threads), with the n-grams of
``ngram_ref.model(V, order)``.  Every comparison with the oracle first asserts, ON THE ORACLE, selection margin and rank
gap >= 2e-3, ten times the 2e-4 tolerance: a condition on the inputs.  The working points (lm_weight, length_bonus, order,
phrase list, ilm_weight) and their measured margins are tests/sync_ngram_ref.py's ``POINTS`` and ``EDGES`` tables, found on
the oracle alone on the CPU; tests/test_sync_ngram_host.py asserts the same margins without a GPU.

The n-gram term is fp64 on both sides and bit-equal to the host's, so the tolerance is the RNN-T log-softmax's alone, as in
the plain search's test.  The streaming comparisons are bit equalities against the offline search on the device."""
import numpy as np
import pytest
import torch

import ngram_ref as NR
import sync_ngram_ref as R
from oracle import models_ref as M
from test_lm_fusion_gpu import STREAM_CFG
from test_sync_beam_gpu import CFG32, CFGS, _engine, _inputs, _rows, _same_bits
from test_sync_fusion_gpu import _assert_matches
from test_sync_stream_fusion_gpu import PAUSES, _offline, _search
from test_sync_stream_gpu import BIAS, _check_best, _check_committed, _chunk, _ragged_chunk, _random_split

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------- 1. against the oracle
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("W", R.WIDTHS)
@pytest.mark.parametrize("name", R.NAMES)
def test_ngram_nbest_matches_the_oracle(hip_lib, name, W, mode):
    from edgedict_amd import decode
    sd, xs, xlen = _inputs(name)
    ref, infos = R.reference(name, mode, W)
    R.assert_decisive(infos, W, ref)
    m = _engine(sd, CFGS[name][0])
    kw = R.device_kwargs(name, mode, W)
    res = m.sync_beam_search_nbest(xs.cuda(), xlen, W=W, **kw)
    _assert_matches(res, ref)
    seqs, scores = decode.sync_beam_search_fusion(m, xs.cuda(), xlen, W=W, **kw)
    for b, r in enumerate(res):
        assert np.array_equal(seqs[b], r.tokens[0]) and scores[b].item() == -r.logp[0]
    # the fusion acts: the best hypothesis of at least one utterance is not the plain search's
    plain, _ = m.sync_beam_search(xs.cuda(), xlen, W=W)
    assert sum(not np.array_equal(a, b) for a, b in zip(plain, seqs)) >= 1


# ------------------------------------------------------------------------------------------- 2. back-off edges
@pytest.mark.parametrize("edge", list(R.EDGES))
def test_back_off_edges_match_the_oracle(hip_lib, edge):
    """order1: no arcs, only the unigram level;  order6: the longest chain;  wide: a context of 140 arcs (V = 520);
    closure: states without arcs;  longest: one token in the bigram row AND the trigram row of a reachable context with
    clearly different values - the longest context must win (a missing barrier or a reversed level order fails here)."""
    cfg, sd, xs, xlen = R.edge_inputs(edge)
    W, w, lb = R.EDGES[edge][2:]
    ref, infos = R.edge_reference(edge)
    R.assert_decisive(infos, W, ref)
    m = _engine(sd, cfg)
    res = m.sync_beam_search_nbest(xs.cuda(), xlen, W=W, lm=R.edge_lm(edge), lm_weight=w, length_bonus=lb)
    _assert_matches(res, ref)


# ------------------------------------------------------------------------------------------- 3. zero weight, zero bonus
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", R.NAMES)
def test_zero_weight_and_zero_bonus_are_the_plain_search(hip_lib, name, dtype):
    """``NGramLM.train`` gives finite unigrams everywhere: 0 * lp + 0 adds 0.0 to every candidate."""
    cfg = CFGS[name][0]
    sd, xs, xlen = _inputs(name)
    m = _engine(sd, cfg, dtype)
    lm = NR.model(cfg["vocab_size"], 3)
    assert np.isfinite(np.delete(lm.uni_lp, lm.blank)).all()
    W = 10
    plain = m.sync_beam_search_nbest(xs.cuda(), xlen, W=W)
    zero = m.sync_beam_search_nbest(xs.cuda(), xlen, W=W, lm=lm, lm_weight=0.0, length_bonus=0.0)
    zero_ilm = m.sync_beam_search_nbest(xs.cuda(), xlen, W=W, lm=lm, lm_weight=0.0, length_bonus=0.0, ilm_weight=0.0)
    for a, b, c in zip(plain, zero, zero_ilm):
        _same_bits(a, b)
        _same_bits(a, c)
    assert sum(len(t) for r in plain for t in r.tokens) > 0


# ------------------------------------------------------------------------------------------- 4. determinism
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("B,W", [(3, 10), (1, 32), (2, 4)])
def test_ngram_utterance_alone_in_a_batch_behind_a_length_and_again(hip_lib, B, W, dtype):
    """B x W rows 30 (no multiple of the 16-row tile), 32 and 8, with the n-gram, ILME and a list together."""
    from edgedict_amd import decode
    sd, xs, _ = _inputs("CFG32", 3.0, 5, 17)
    m = _engine(sd, CFG32, dtype)
    kw = R.device_kwargs("CFG32", "ngram+ilm+list", 4)
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


# ------------------------------------------------------------------------------------------- 5. streaming
STREAM_CASES = [("CFG", 4, "ngram"), ("CFG32", 4, "ngram"), ("CFG32", 10, "ngram"), ("CFG32", 4, "ngram+list"),
                ("CFG32", 4, "ngram+ilm"), ("CFG", 4, "ngram+ilm+list"), ("CFG32", 10, "ngram+ilm+list"),
                ("CFGV", 4, "ngram")]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name,W,mode", STREAM_CASES)
def test_every_chunking_equals_the_offline_ngram_search_after_every_chunk(hip_lib, name, W, mode, dtype):
    """One frame at a time, a random split, and ragged chunks in which every stream sits some chunk out."""
    cfg = CFGS[name][0]
    sd, xs, _ = _inputs(name, BIAS, 3, 17)
    m = _engine(sd, cfg, dtype)
    kw = R.device_kwargs(name, mode, W)
    E1, T, P = _rows(m, xs)
    assert T == 9 and np.sum(PAUSES, axis=0).tolist() == [T] * 3
    want = {n: _offline(m, E1, n, P, W, **kw) for n in range(1, T + 1)}        # computed once, read only
    plain = _offline(m, E1, T, P, W)
    assert any(not np.array_equal(a.logp, b.logp) for a, b in zip(want[T], plain))     # the fusion does something
    assert sum(len(t) for r in want[T] for t in r.tokens) > 0
    for split in ([1] * T, _random_split(T, 3)):
        sb = _search(m, 3, W, **kw)
        t = 0
        for n in split:
            sb.advance_rows(_chunk(E1, t, n), P)
            t += n
            res = sb.nbest()
            for s in range(3):
                _same_bits(res[s], want[t][s])
            _check_best(sb, res)
            _check_committed(sb, res)
    sb, pos = _search(m, 3, W, **kw), [0, 0, 0]
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


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("mode", ["ngram", "ngram+ilm+list"])
def test_masked_reset_puts_one_stream_back_on_start(hip_lib, mode, dtype):
    Sn, W = 3, 4
    sd, xs, _ = _inputs("CFG32", BIAS, Sn, 33)
    m = _engine(sd, CFG32, dtype)
    kw = R.device_kwargs("CFG32", mode, W)
    E1, T, P = _rows(m, xs)
    assert T == 17
    sb, untouched = _search(m, Sn, W, **kw), _search(m, Sn, W, **kw)
    mask = torch.tensor([False, True, False])
    t = 0
    for k, n in enumerate((4, 5, 3, 5)):
        if k == 2:
            sb.reset(mask)
            assert len(sb.committed()[1]) == 0 and len(sb.nbest()[1].tokens[0]) == 0
        sb.advance_rows(_chunk(E1, t, n), P)
        untouched.advance_rows(_chunk(E1, t, n), P)
        t += n
        got, ref = sb.nbest(), untouched.nbest()
        for s in range(Sn):
            if k >= 2 and mask[s]:      # a fresh stream over the frames since the reset, counted from it
                _same_bits(got[s], _offline(m, E1[s:s + 1, 9:], t - 9, P, W, **kw)[0])
            else:
                _same_bits(got[s], ref[s])
        _check_committed(sb, got)
    for s, r in enumerate(_offline(m, E1, T, P, W, **kw)):
        if not mask[s]:
            _same_bits(got[s], r)
    assert sum(len(t) for r in got for t in r.tokens) > 0


def test_long_ngram_stream_with_a_small_tree_equals_the_offline_search(hip_lib):
    """200 frames through node_capacity 64 in chunks of 1 .. 3 frames: the tree is compacted on every advance and the
    n-gram states, which compaction does not touch, still belong to the rows.  Trigram at weight 0.5, bonus 1.5: on the
    oracle (sync_fusion_ref.StreamSearch in chunks of 2) the two streams commit 72 and 73 tokens and peak at 8 and 6 live
    nodes; with bonus 0.5 nothing is committed, with 3.0 the live tree passes 64."""
    Sn, W, NC = 2, 4, 64
    sd, xs, _ = _inputs("CFG32", 3.0, Sn, 399)
    m = _engine(sd, CFG32, "fp32")
    kw = dict(lm=NR.model(64, 3), lm_weight=0.5, length_bonus=1.5)
    E1, T, P = _rows(m, xs)
    assert T == 200 and NC < T * W          # the offline tree of T W nodes would not fit
    sb = _search(m, Sn, W, node_capacity=NC, **kw)
    t = 0
    for n in _random_split(T, 0, 3):
        sb.advance_rows(_chunk(E1, t, n), P)
        t += n
    print("live nodes:", sb.live_nodes(), "committed:", [len(c) for c in sb.committed()])
    assert sum(len(c) for c in sb.committed()) > 0
    res = sb.nbest()
    for s, r in enumerate(_offline(m, E1, T, P, W, **kw)):
        _same_bits(res[s], r)
    plain = _offline(m, E1, T, P, W)
    assert any(not np.array_equal(a.logp, b.logp) for a, b in zip(res, plain))
    _check_committed(sb, res)
    _check_best(sb, res)


def test_audio_level_decoder_with_an_ngram_equals_the_offline_search(hip_lib):
    from edgedict_amd import decode
    from edgedict_amd.bias import ContextGraph
    from edgedict_amd.flags import make_flags
    from edgedict_amd.stream import BatchedStreamSyncFusionBeamDecoder, chunk_geometry
    flags = make_flags("E6D2")
    sd = M.make_state_dict(STREAM_CFG, 5)
    sd["joint.joint.2.bias"][0] += 1.0
    m = _engine(sd, STREAM_CFG, "fp32")
    kw = dict(lm=NR.model(64, 3), lm_weight=0.5, length_bonus=1.0, ilm_weight=0.2,
              bias=ContextGraph([[10, 63], [21, 40, 5]], 2.0, 64))
    Sn, W = 3, 4
    win, hop = chunk_geometry(flags, 2)
    g = torch.Generator().manual_seed(0)
    wave = (0.1 * torch.randn(Sn, win + 5 * hop, generator=g)).cuda()
    dec = BatchedStreamSyncFusionBeamDecoder(m, flags, Sn, W=W, dither=0, **kw)
    L, H = len(m.encoder.lstm.lstms), m.encoder.lstm.hidden_size
    h = torch.zeros(L, Sn, H, device="cuda")
    c = torch.zeros(L, Sn, H, device="cuda")
    rows = []
    with torch.no_grad():
        for k in range(6):
            chunk = wave[:, k * hop:k * hop + win].contiguous()
            got, gsc = dec.decode(chunk.clone())
            xs, _ = dec.transform(chunk.clone())
            enc, (h, c) = m.encoder(xs, (h, c))
            enc = enc.contiguous()
            rows.append(decode.joint_rows(m, enc).reshape(Sn, enc.shape[1], -1))
            all_rows = torch.cat(rows, dim=1)
            offline = _offline(m, all_rows, all_rows.shape[1], enc.shape[2], W, **kw)
            res = dec.nbest()
            for s in range(Sn):
                _same_bits(res[s], offline[s])
                assert np.array_equal(got[s], offline[s].tokens[0]) and gsc[s].item() == -offline[s].logp[0]
            _check_best(dec, res)
    plain = _offline(m, all_rows, all_rows.shape[1], enc.shape[2], W)
    assert any(not np.array_equal(a.logp, b.logp) for a, b in zip(offline, plain))


# ------------------------------------------------------------------------------------------- 6. pass-through
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_skip_blank_one_with_the_ngram_is_the_call_without_it(hip_lib, dtype):
    """On a model with a CTC head: a threshold of 1.0 keeps every frame."""
    from test_frame_skip_gpu import _setup
    s = _setup(dtype)
    kw = dict(lm=NR.model(40, 3), lm_weight=0.5, length_bonus=1.0)
    with torch.no_grad():
        got = s.m.sync_beam_search_nbest(s.xs, s.xlen, W=4, skip_blank=1.0, **kw)
        want = s.m.sync_beam_search_nbest(s.xs, s.xlen, W=4, **kw)
        plain = s.m.sync_beam_search_nbest(s.xs, s.xlen, W=4)
    for b in range(len(want)):
        _same_bits(got[b], want[b])
    assert any(not np.array_equal(g.logp, p.logp) for g, p in zip(got, plain))
    assert sum(len(t) for r in got for t in r.tokens) > 0
