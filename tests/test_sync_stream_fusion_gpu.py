"""GPU: the streaming frame-synchronous beam search with LM shallow fusion and a bias list
(decode.StreamingSyncFusionBeamSearch, stream.BatchedStreamSyncFusionBeamDecoder) against the offline fused search over
the same frames.

Every comparison is a bit equality (tests/test_sync_beam_gpu._same_bits) against
``decode.sync_beam_search_nbest_rows(..., lm=, bias=)``, which tests/test_sync_fusion_gpu.py holds against the fp64
oracle: the streaming form runs the offline search's kernels on the same rows, so nothing here needs a tolerance.
Inputs are tests/test_sync_stream_gpu.py's (sharpened, the blank raised by 1.5, 17 input frames = 9 encoder frames; the
long stream: the blank raised by 3, 200 encoder frames); LM and lists are tests/test_sync_fusion_gpu.py's working points.
The rows' LM states and automaton states live in the persistent state: a state that was carried wrongly between chunks,
left in the wrong buffer by a pause, or not cleared by a reset would change the bits."""
import numpy as np
import pytest
import torch

from oracle import models_ref as M
from test_lm_fusion_gpu import STREAM_CFG, _lm, _lm_sd
from test_sync_beam_gpu import CFG32, CFGS, _engine, _inputs, _rows, _same_bits
from test_sync_fusion_gpu import MODES, _device_kwargs
from test_sync_stream_gpu import BIAS, _check_best, _check_committed, _chunk, _ragged_chunk, _random_split

pytestmark = pytest.mark.gpu


def _search(m, Sn, W, **kw):
    from edgedict_amd.decode import StreamingSyncFusionBeamSearch
    return StreamingSyncFusionBeamSearch(m, Sn, W=W, **kw)


def _offline(m, E1, n, P, W, **kw):
    """The offline fused search over the first n frames of E1 [S, T, J]."""
    from edgedict_amd import decode
    Sn = E1.shape[0]
    return decode.sync_beam_search_nbest_rows(m, E1[:, :n].contiguous().reshape(Sn * n, E1.shape[2]), Sn, n, P, None, W,
                                              **kw)


# frames per chunk and stream: stream 1 sits chunks 0 and 3 out, stream 2 chunk 1, stream 0 chunk 2 - each while the
# others run an odd number of frames, so a state left in the wrong one of the two buffers would be read
PAUSES = [[2, 0, 3], [1, 3, 0], [0, 2, 1], [3, 0, 2], [3, 3, 3], [0, 1, 0]]


# ------------------------------------------------------------------------------------------- 1. chunking invariance
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,W", [("CFG", 4), ("CFG32", 4), ("CFG32", 10)])
def test_every_chunking_equals_the_offline_fused_search_after_every_chunk(hip_lib, name, W, mode, dtype):
    cfg = CFGS[name][0]
    sd, xs, _ = _inputs(name, BIAS, 3, 17)
    m = _engine(sd, cfg, dtype)
    kw = _device_kwargs(name, mode, W, dtype)
    E1, T, P = _rows(m, xs)
    assert T == 9 and np.sum(PAUSES, axis=0).tolist() == [T] * 3
    want = {n: _offline(m, E1, n, P, W, **kw) for n in range(1, T + 1)}        # computed once, read only
    plain = _offline(m, E1, T, P, W)
    assert any(not np.array_equal(a.logp, b.logp) for a, b in zip(want[T], plain))     # the fusion does something
    assert sum(len(t) for r in want[T] for t in r.tokens) > 0      # (this LM alone empties CFG32's best hypotheses)
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


# ------------------------------------------------------------------------------------------- 2. masked reset
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("mode", MODES)
def test_masked_reset_clears_the_lm_and_automaton_state_of_one_stream(hip_lib, mode, dtype):
    Sn, W = 3, 4
    sd, xs, _ = _inputs("CFG32", BIAS, Sn, 33)
    m = _engine(sd, CFG32, dtype)
    kw = _device_kwargs("CFG32", mode, W, dtype)
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


# ------------------------------------------------------------------------------------------- 3. long stream
def test_long_fused_stream_with_a_small_tree_equals_the_offline_search(hip_lib):
    """200 frames through node_capacity 64 in chunks of 1 .. 3 frames: the tree is compacted on every advance and the
    LM and automaton states, which compaction does not touch, still belong to the rows.  On the oracle
    (sync_fusion_ref.StreamSearch on these inputs) the two streams peak at 3 and 4 live nodes and commit 1 and 5
    tokens."""
    Sn, W, NC = 2, 4, 64
    sd, xs, _ = _inputs("CFG32", 3.0, Sn, 399)
    m = _engine(sd, CFG32, "fp32")
    kw = _device_kwargs("CFG32", "both", W)
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
    _check_committed(sb, res)
    _check_best(sb, res)


# ------------------------------------------------------------------------------------------- 4. set_bias
@pytest.mark.parametrize("with_lm", [False, True])
def test_set_bias_on_fresh_streams_acts_on_the_next_advance(hip_lib, with_lm):
    from edgedict_amd.bias import ContextGraph
    Sn, W = 3, 4
    sd, xs, _ = _inputs("CFG32", BIAS, Sn, 17)
    m = _engine(sd, CFG32, "fp32")
    both = _device_kwargs("CFG32", "both", W)
    lm_kw = {k: v for k, v in both.items() if k != "bias"} if with_lm else {}
    graph = both["bias"]
    other = ContextGraph([[10, 63], [7, 8, 9]], 1.0, 64)
    E1, T, P = _rows(m, xs)
    sb = _search(m, Sn, W, **lm_kw)                 # built without a list: the plain or the LM-only form
    sb.set_bias(graph)                              # the state gains the automaton states
    sb.advance_rows(_chunk(E1, 0, 4), P)
    for s, r in enumerate(_offline(m, E1, 4, P, W, bias=graph, **lm_kw)):
        _same_bits(sb.nbest()[s], r)
    with pytest.raises(ValueError, match="stream 0 has advanced over 4 frames"):
        sb.set_bias(other)
    with pytest.raises(ValueError, match="outside the mask"):
        sb.set_bias(other, mask=[False, False, False])
    sb.advance_rows(_chunk(E1, 4, 5), P)            # the refused swaps changed nothing
    for s, r in enumerate(_offline(m, E1, T, P, W, bias=graph, **lm_kw)):
        _same_bits(sb.nbest()[s], r)
    sb.reset()
    sb.set_bias(other)                              # same state size: nothing is launched, the next advance reads it
    sb.advance_rows(_chunk(E1, 0, T), P)
    for s, r in enumerate(_offline(m, E1, T, P, W, bias=other, **lm_kw)):
        _same_bits(sb.nbest()[s], r)
    sb.reset()
    sb.set_bias(None)                               # the list is lost again
    sb.advance_rows(_chunk(E1, 0, T), P)
    for s, r in enumerate(_offline(m, E1, T, P, W, **lm_kw)):
        _same_bits(sb.nbest()[s], r)


# ------------------------------------------------------------------------------------------- 5. audio-level decoder
def test_audio_level_decoder_with_lm_and_list_equals_the_offline_fused_search(hip_lib):
    from edgedict_amd import decode
    from edgedict_amd.bias import ContextGraph
    from edgedict_amd.flags import make_flags
    from edgedict_amd.stream import BatchedStreamSyncFusionBeamDecoder, chunk_geometry
    flags = make_flags("E6D2")
    sd = M.make_state_dict(STREAM_CFG, 5)
    sd["joint.joint.2.bias"][0] += 1.0
    m = _engine(sd, STREAM_CFG, "fp32")
    kw = dict(lm=_lm(_lm_sd(64, 32, 64, 2, seed=8, scale=3.0)), lm_weight=0.5, length_bonus=0.2,
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
