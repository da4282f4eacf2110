"""GPU: the streaming frame-synchronous beam search (csrc/decode_sync.hip ``edgedict_sync_stream_*``;
decode.StreamingSyncBeamSearch, stream.BatchedStreamSyncBeamDecoder) against the offline search over the same frames.

Every comparison is a bit equality (tests/test_sync_beam_gpu._same_bits: tokens, frames, token_logp, logp) against
``decode.sync_beam_search_nbest_rows``: the streaming form runs the offline search's kernels on the same rows, so
nothing here needs a tolerance.  The joint's encoder rows are computed once per test with ``decode.joint_rows`` and
sliced per chunk (tests/test_stream_beam_gpu.py shows that they do not depend on the row count).

Inputs: the configs and pinned state-dict seeds of tests/test_sync_beam_gpu.py, sharpened (scale 6) with the blank
raised by 1.5, 17 input frames = 9 encoder frames.  The commit rule depends on the data: with that file's own inputs
(blank raised by 3, 9 input frames) the empty hypothesis never leaves a beam of W > 1 (tests/sync_stream_ref.py on them:
no commit on any frame), and with the blank raised by 2 or 2.5 some (config, W, dtype) still commit nothing before the
last frame; raised by 1.5, every config, W in 4, 10, 32 and both dtypes commit in at least one stream after 8 of the 9
frames (1 .. 9 tokens over the three streams, 15 .. 23 tokens in the final best hypotheses)."""
import numpy as np
import pytest
import torch

import sync_beam_ref as S
from edgedict_amd.decode import StreamingSyncBeamSearch
from edgedict_amd.stream import BatchedStreamSyncBeamDecoder
from oracle import models_ref as M
from test_sync_beam_gpu import CFG, CFG32, CFGS, G, MIN_MARGIN, TOL, _engine, _inputs, _rows, _same_bits

pytestmark = pytest.mark.gpu
BIAS = 1.5


def _offline(m, E1, n, P, W):
    """The offline search over the first n frames of E1 [S, T, J]; n = 0: the empty hypothesis."""
    from edgedict_amd import decode
    Sn = E1.shape[0]
    return decode.sync_beam_search_nbest_rows(m, E1[:, :n].contiguous().reshape(Sn * n, E1.shape[2]), Sn, n, P, None, W)


def _chunk(E1, t0, n):
    return E1[:, t0:t0 + n].contiguous().reshape(E1.shape[0] * n, E1.shape[2])


def _search(m, Sn, W, **kw):
    return StreamingSyncBeamSearch(m, Sn, W=W, **kw)


def _check_committed(sb, results):
    """The committed log is a prefix of every hypothesis, in tokens, frames and token_logp; returns the log lengths."""
    detail, plain = sb.committed_detail(), sb.committed()
    for s, (r, (ct, cf, cl)) in enumerate(zip(results, detail)):
        assert ct.dtype == np.int64 and cf.dtype == np.int32 and cl.dtype == np.float64
        assert np.array_equal(plain[s], ct)
        k = len(ct)
        assert len(cf) == k and len(cl) == k
        for i in range(len(r)):
            assert np.array_equal(r.tokens[i][:k], ct), (s, i, r.tokens[i], ct)
            assert np.array_equal(r.frames[i][:k], cf), (s, i, r.frames[i], cf)
            assert np.array_equal(r.token_logp[i][:k], cl), (s, i)
    return [len(ct) for ct, _, _ in detail]


def _check_best(sb, results):
    seqs, scores = sb.best()
    assert scores.dtype == torch.float64
    for s, r in enumerate(results):
        assert seqs[s].dtype == np.int64 and np.array_equal(seqs[s], r.tokens[0])
        assert scores[s].item() == -r.logp[0]


def _random_split(T, seed, hi=4):
    rng = np.random.default_rng(seed)
    out, t = [], 0
    while t < T:
        out.append(min(int(rng.integers(1, hi + 1)), T - t))
        t += out[-1]
    return out


# ------------------------------------------------------------------------------------------- 1. chunking invariance
CASES = [("CFG", 1), ("CFG32", 1), ("CFG", 4), ("CFG32", 4), ("CFG", 10), ("CFG32", 10), ("CFG", 32), ("CFG32", 32),
         ("CFGV", 4)]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name,W", CASES)
def test_every_chunking_equals_the_offline_search_after_every_chunk(hip_lib, name, W, dtype):
    cfg = CFGS[name][0]
    sd, xs, _ = _inputs(name, BIAS, 3, 17)
    m = _engine(sd, cfg, dtype)
    E1, T, P = _rows(m, xs)
    assert T == 9
    want = {n: _offline(m, E1, n, P, W) for n in range(0, T + 1)}        # computed once, read only
    assert sum(len(r.tokens[0]) for r in want[T]) > 0
    early = 0
    for split in ([1] * T, [T], [1, 3, 5], _random_split(T, 3)):
        assert sum(split) == T
        sb = _search(m, 3, W)
        res = sb.nbest()
        for s in range(3):
            _same_bits(res[s], want[0][s])          # no frames yet: one empty hypothesis, logp 0
            assert len(res[s]) == 1 and len(res[s].tokens[0]) == 0 and res[s].logp[0] == 0.0
        t = 0
        for n in split:
            sb.advance_rows(_chunk(E1, t, n), P)
            t += n
            res = sb.nbest()
            for s in range(3):
                _same_bits(res[s], want[t][s])
            _check_best(sb, res)
            ncom = _check_committed(sb, res)
            assert (sb.live_nodes() <= t * W).all()
            if t < T:
                early += sum(ncom)
    assert W == 1 or early > 0, "no split committed a token before the last frame"


# ------------------------------------------------------------------------------------------- 2. row-tile edges
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("Sn,W", [(3, 4), (4, 4), (5, 4), (1, 32), (2, 10)])
def test_stream_in_a_batch_equals_the_stream_alone(hip_lib, Sn, W, dtype):
    """S x W rows below, on and above the step kernels' 16-row tile: 12, 16, 20, 32, 20."""
    sd, xs, _ = _inputs("CFG32", BIAS, 5, 17)
    m = _engine(sd, CFG32, dtype)
    E1, T, P = _rows(m, xs[:Sn])
    batch = _search(m, Sn, W)
    alone = [_search(m, 1, W) for _ in range(Sn)]
    t, n_tokens = 0, 0
    for n in (2, 3, 4):
        batch.advance_rows(_chunk(E1, t, n), P)
        res = batch.nbest()
        for s in range(Sn):
            alone[s].advance_rows(_chunk(E1[s:s + 1], t, n), P)
            _same_bits(res[s], alone[s].nbest()[0])
            assert np.array_equal(batch.committed()[s], alone[s].committed()[0])
        t += n
    assert t == T
    for s, r in enumerate(_offline(m, E1, T, P, W)):
        _same_bits(res[s], r)
        n_tokens += sum(len(x) for x in r.tokens)
    assert n_tokens > 0


# ------------------------------------------------------------------------------------------- 3. ragged chunks
# frames per chunk and stream.  Streams pause (0) while the others run an ODD number of frames - stream 0 over chunks 1-2
# (3 frames), stream 1 over chunk 3 (3), stream 2 over chunk 0 (3) and chunk 4 (3), stream 3 over chunk 3, stream 4 over
# chunks 1-2 and chunk 4 - so a state left in the wrong one of the two buffers would be read; chunk 2 has no frames at all;
# inside a chunk streams stop an odd and an even number of frames before the longest one
RAGGED = [[3, 1, 0, 2, 3], [0, 2, 1, 3, 0], [0, 0, 0, 0, 0], [1, 0, 3, 0, 2], [2, 3, 0, 1, 0], [0, 1, 2, 0, 3],
          [3, 0, 1, 2, 1]]


def _ragged_plan(T):
    plan, pos = [list(c) for c in RAGGED], np.sum(RAGGED, axis=0)
    assert (pos <= T).all()
    while (pos < T).any():
        nf = np.minimum(T - pos, 4)
        plan.append(nf.tolist())
        pos = pos + nf
    return plan


def _ragged_chunk(E1, pos, nf):
    """[S * Tc, J]: stream s' next frames from pos[s], zero behind its nf[s] (never read)."""
    Sn, T, J = E1.shape
    Tc = int(max(nf))
    out = torch.zeros(Sn, Tc, J, dtype=E1.dtype, device=E1.device)
    for s in range(Sn):
        out[s, :nf[s]] = E1[s, pos[s]:pos[s] + nf[s]]
    return out.reshape(Sn * Tc, J)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_ragged_chunks_and_pauses_equal_independent_streams(hip_lib, dtype):
    Sn, W = 5, 4
    sd, xs, _ = _inputs("CFG32", BIAS, Sn, 33)
    m = _engine(sd, CFG32, dtype)
    E1, T, P = _rows(m, xs)
    assert T == 17
    batch = _search(m, Sn, W)
    alone = [_search(m, 1, W) for _ in range(Sn)]
    pos = [0] * Sn
    for nf in _ragged_plan(T):
        batch.advance_rows(_ragged_chunk(E1, pos, nf), P, np.asarray(nf, dtype=np.int32))
        for s in range(Sn):
            if nf[s]:
                alone[s].advance_rows(_chunk(E1[s:s + 1], pos[s], nf[s]), P)
            pos[s] += nf[s]
        res = batch.nbest()
        for s in range(Sn):
            _same_bits(res[s], alone[s].nbest()[0])
            _same_bits(res[s], _offline(m, E1[s:s + 1], pos[s], P, W)[0])
            assert all((f < pos[s]).all() for f in res[s].frames)
        _check_committed(batch, res)
    assert pos == [T] * Sn
    assert sum(len(r.tokens[0]) for r in res) > 0


# ------------------------------------------------------------------------------------------- 4. masked reset
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_masked_reset_restarts_two_streams_and_leaves_the_others_alone(hip_lib, dtype):
    Sn, W = 5, 4
    sd, xs, _ = _inputs("CFG32", BIAS, Sn, 33)
    m = _engine(sd, CFG32, dtype)
    E1, T, P = _rows(m, xs)
    sb, plain = _search(m, Sn, W), _search(m, Sn, W)
    mask = torch.tensor([False, True, False, True, False])
    t = 0
    for k, n in enumerate((4, 5, 3, 5)):
        if k == 2:
            sb.reset(mask)
            for s in (1, 3):
                assert len(sb.committed()[s]) == 0 and len(sb.nbest()[s].tokens[0]) == 0
        sb.advance_rows(_chunk(E1, t, n), P)
        plain.advance_rows(_chunk(E1, t, n), P)
        t += n
        got, ref = sb.nbest(), plain.nbest()
        for s in range(Sn):
            if k >= 2 and mask[s]:      # a fresh stream over the frames since the reset, counted from it
                fresh = _offline(m, E1[s:s + 1, 9:], t - 9, P, W)[0]
                _same_bits(got[s], fresh)
                assert all((f < t - 9).all() for f in got[s].frames)
            else:
                _same_bits(got[s], ref[s])
                assert np.array_equal(sb.committed()[s], plain.committed()[s])
        _check_committed(sb, got)
    assert t == T
    for s, r in enumerate(_offline(m, E1, T, P, W)):
        if not mask[s]:
            _same_bits(got[s], r)


# ------------------------------------------------------------------------------------------- 5. long stream
def test_long_stream_keeps_a_bounded_tree_and_loses_nothing(hip_lib):
    """The blank raised by 3 here (tests/test_sync_beam_gpu.py's default): on the oracle the two streams then peak at 12
    and 9 live nodes over 200 frames and commit 9 of 9 and 4 of 5 tokens.  (With the blank raised by 2 the same streams
    emit about 100 tokens each, sequences are pruned and created again all the time, and the tree's common ancestor lags
    far behind the common token prefix: 6 and 27 tokens committed, 209 and 264 live nodes at the peak.)"""
    Sn, W, NC = 2, 4, 64
    sd, xs, _ = _inputs("CFG32", 3.0, Sn, 399)
    m = _engine(sd, CFG32, "fp32")
    E1, T, P = _rows(m, xs)
    assert T == 200 and NC < T * W          # the offline tree of T W nodes would not fit
    sb = _search(m, Sn, W, node_capacity=NC)
    t, sizes, peak = 0, [], 0
    for n in _random_split(T, 0, 3):
        sb.advance_rows(_chunk(E1, t, n), P)
        t += n
        peak = max(peak, int(sb.live_nodes().max()))
        assert (sb.live_nodes() < NC).all()
        sizes.append([len(c) for c in sb.committed()])
    print("peak live nodes:", peak, "committed:", sizes[-1])
    sizes = np.asarray(sizes)
    assert (np.diff(sizes, axis=0) >= 0).all()                  # the log only grows ...
    assert (sizes[-1] > 0).all() and (np.diff(sizes.sum(axis=1)) > 0).sum() >= 2              # ... and does grow
    res = sb.nbest()
    for s, r in enumerate(_offline(m, E1, T, P, W)):
        _same_bits(res[s], r)
    _check_committed(sb, res)
    _check_best(sb, res)


# ------------------------------------------------------------------------------------------- 6. capacity
def test_too_small_a_tree_is_an_error_before_the_advance_runs(hip_lib):
    Sn, W, NC = 2, 4, 16
    sd, xs, _ = _inputs("CFG32", BIAS, 5, 17)
    m = _engine(sd, CFG32, "fp32")
    E1, T, P = _rows(m, xs[:Sn])
    sb = _search(m, Sn, W, node_capacity=NC)
    sb.advance_rows(_chunk(E1, 0, 3), P)
    before, live = sb.nbest(), sb.live_nodes()
    assert (live + 1 * W <= NC).all()
    with pytest.raises(RuntimeError, match="node_capacity"):
        sb.advance_rows(_chunk(E1, 3, 5), P)                    # live + 5 W > 16 whatever the tree holds
    with pytest.raises(RuntimeError, match="node_capacity"):
        sb.advance_rows(_chunk(E1, 3, 5), P, np.asarray([0, 5], dtype=np.int32))
    after = sb.nbest()
    for s in range(Sn):
        _same_bits(before[s], after[s])
    assert np.array_equal(sb.live_nodes(), live)
    sb.advance_rows(_chunk(E1, 3, 1), P)                        # the state is as it was: a legal advance still matches
    for s, r in enumerate(_offline(m, E1, 4, P, W)):
        _same_bits(sb.nbest()[s], r)


# ------------------------------------------------------------------------------------------- 7. determinism
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["CFG", "CFG32"])
def test_two_runs_over_the_same_chunks_give_the_same_bits(hip_lib, name, dtype):
    cfg = CFGS[name][0]
    sd, xs, _ = _inputs(name, BIAS, 3, 17)
    m = _engine(sd, cfg, dtype)
    E1, T, P = _rows(m, xs)
    runs = []
    for _ in range(2):
        sb, t, out = _search(m, 3, 10), 0, []
        for n in (2, 1, 4, 2):
            sb.advance_rows(_chunk(E1, t, n), P)
            t += n
            out.append((sb.nbest(), sb.committed_detail()))
        runs.append(out)
    for (ra, ca), (rb, cb) in zip(*runs):
        for a, b in zip(ra, rb):
            _same_bits(a, b)
        for x, y in zip(ca, cb):
            assert all(np.array_equal(u, v) for u, v in zip(x, y))


# ------------------------------------------------------------------------------------------- 8. audio-level decoder
@pytest.mark.parametrize("geometry", ["native", "hop640", "one_frame"])
def test_audio_level_decoder_equals_the_search_over_the_module_path(hip_lib, geometry):
    """native: 2 stacked frames of 240 features per chunk; hop640: 3 of 160, the odd count zero-padded by the time
    reduction in every chunk; one_frame: a lone frame of 240 (oracle.make_golden_stream.GEOMETRIES)."""
    from edgedict_amd import decode
    from edgedict_amd.stream import chunk_geometry
    from oracle.make_golden_stream import GEOMETRIES, geometry_flags
    from test_stream_beam_gpu import STREAM_CFG
    geo, flags = GEOMETRIES[geometry], geometry_flags(geometry)
    cfg = dict(STREAM_CFG, input_size=geo.I0)
    sd = M.make_state_dict(cfg, 5)
    sd["joint.joint.2.bias"][0] += 1.0
    m = _engine(sd, cfg, "fp32")
    Sn, W = 3, 4
    win, hop = chunk_geometry(flags, geo.step_n_frame)
    assert (win, hop) == (geo.win, geo.hop)
    g = torch.Generator().manual_seed(0)
    wave = (0.1 * torch.randn(Sn, win + 5 * hop, generator=g)).cuda()
    dec = BatchedStreamSyncBeamDecoder(m, flags, Sn, W=W, dither=0)
    sb = _search(m, Sn, W)
    L, H = len(m.encoder.lstm.lstms), m.encoder.lstm.hidden_size
    h = torch.zeros(L, Sn, H, device="cuda")
    c = torch.zeros(L, Sn, H, device="cuda")
    rows = []
    with torch.no_grad():
        for k in range(6):
            chunk = wave[:, k * hop:k * hop + win].contiguous()
            got, gsc = dec.decode(chunk.clone())
            xs, _ = dec.transform(chunk.clone())
            assert tuple(xs.shape) == (Sn, geo.T0, geo.I0)
            enc, (h, c) = m.encoder(xs, (h, c))
            enc = enc.contiguous()
            assert enc.shape[1] == geo.T_out
            sb.advance(enc)
            rows.append(decode.joint_rows(m, enc).reshape(Sn, enc.shape[1], -1))
            all_rows = torch.cat(rows, dim=1)
            offline = _offline(m, all_rows, all_rows.shape[1], enc.shape[2], W)
            res = dec.nbest()
            for s in range(Sn):
                _same_bits(res[s], sb.nbest()[s])
                _same_bits(res[s], offline[s])
                assert np.array_equal(got[s], offline[s].tokens[0]) and gsc[s].item() == -offline[s].logp[0]
                assert np.array_equal(dec.committed()[s], sb.committed()[s])
                assert all(np.array_equal(u, v) for u, v in zip(dec.committed_detail()[s], sb.committed_detail()[s]))
            _check_best(dec, res)
    mask = torch.tensor([True, False, True])
    dec.reset(mask)
    res = dec.nbest()
    assert len(res[0].tokens[0]) == 0 and res[0].logp[0] == 0.0 and float(dec.enc_h[:, 0].abs().sum()) == 0.0
    _same_bits(res[1], offline[1])


# ------------------------------------------------------------------------------------------- 9. the old searches
# Whole-list equality with the fp64 oracle needs the oracle's own margins (tests/test_sync_beam_gpu.py: smallest selection
# margin and rank gap >= 2e-3, ten times the tolerance), a property of the inputs alone.  On test 1's inputs (blank raised
# by 1.5, 17 frames) they hold at W = 1 (1.0e-2 and 1.8e-2 for CFG and CFG32) and not at W = 4 (2.4e-4, 1.2e-3) or 10
# (7.1e-4, 5.8e-4); with the blank raised by 2 they hold at W = 4 (3.5e-3 / 1.0e-2, 7.6e-3 / 5.2e-3) and not at 10 (3.3e-4,
# 7.3e-4) or for CFGV (5.7e-4); W = 10 and CFGV are therefore compared on that file's own inputs, where its table pins
# them.  At W = 32 no input tried has them (1e-4 .. 2e-3: a beam of 32 over 40 or 64 symbols keeps candidates of almost
# equal, tiny probability); that file has no W = 32 case either.
@pytest.mark.parametrize("name,W,bias,T0", [("CFG", 1, BIAS, 17), ("CFG32", 1, BIAS, 17), ("CFG", 4, 2.0, 17),
                                            ("CFG32", 4, 2.0, 17), ("CFG", 10, 3.0, 9), ("CFG32", 10, 3.0, 9),
                                            ("CFGV", 4, 3.0, 9)])
def test_offline_sync_search_still_matches_its_oracle(hip_lib, name, W, bias, T0):
    cfg = CFGS[name][0]
    sd, xs, xlen = _inputs(name, bias, 3, T0)
    ref, infos = S.search(sd, xs, xlen, W)
    print("margin / gap / merges:", [(i["margin"], i["rank_gap"], i["merges"]) for i in infos])
    for info in infos:
        assert info["margin"] >= MIN_MARGIN and info["rank_gap"] >= MIN_MARGIN, info
    m = _engine(sd, cfg)
    res = m.sync_beam_search_nbest(xs.cuda(), xlen, W=W)
    assert len(res) == xs.shape[0] and any(len(r[0]["tokens"]) > 0 for r in ref)
    for b, (r, want) in enumerate(zip(res, ref)):
        assert len(r) == len(want), (b, len(r), len(want))
        for i, h in enumerate(want):
            assert np.array_equal(r.tokens[i], h["tokens"]), (b, i, r.tokens[i], h["tokens"])
            assert np.array_equal(r.frames[i], h["frames"]), (b, i, r.frames[i], h["frames"])
            np.testing.assert_allclose(r.token_logp[i], np.asarray(h["token_logp"], dtype=np.float64), **TOL)
        np.testing.assert_allclose(r.logp, [h["logp"] for h in want], **TOL)


@pytest.mark.parametrize("W", [4, 10])
def test_best_first_search_still_reproduces_its_golden_results(hip_lib, W):
    from edgedict_amd import decode
    sd = {k[3:]: torch.from_numpy(G[k]) for k in G.files if k.startswith("sd/")}
    m = _engine(sd, CFG)
    with torch.no_grad():
        seqs, scores = m.beam_search(torch.from_numpy(G["xs"]).cuda(), torch.from_numpy(G["xlen"]), W=W)
    for b, s in enumerate(seqs):
        assert np.array_equal(s, G["W%d_seq%d" % (W, b)]), (W, b, s)
    np.testing.assert_allclose(scores.numpy(), G["W%d_score" % W], **TOL)
    assert decode.beam_search_batch.last_expansions == int(G["W%d_expansions" % W][0])
