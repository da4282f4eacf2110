"""GPU: the streaming CTC prefix beam search (csrc/ctc_decode.hip ``edgedict_ctc_stream_*``;
decode.StreamingCTCBeamSearch, stream.BatchedStreamCTCBeamDecoder) against the offline search over the same frames.

The oracle is the offline kernel, ``loss.ctc_prefix_beam``, which tests/test_ctc_beam_gpu.py pins to the float64
restatement tests/ctc_beam_ref.py.  Every comparison is an equality of bits - tokens, frames, counts as integers,
token_lp as float32 bits, logp as float64 bits - and nothing here has a tolerance.  The offline lists of ALL prefixes of
an utterance come from one call (a batch of T + 1 copies with lengths 0 .. T) and are shared by the tests of a case.
Rows of a chunk that a stream does not take are NaN: a read past ``n_frames[s]`` shows in the results."""
import functools

import numpy as np
import pytest
import torch

import ctc_beam_ref as BR
import ctc_stream_ref as SR
import ngram_ref as NR

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dtype", ["f32", "bf16"])
_TORCH = {"f32": torch.float32, "bf16": torch.bfloat16}
SHAPES = [(47, 32, 10, 16), (65, 40, 10, 32), (33, 520, 10, 32), (8, 40, 32, 32), (10, 80, 10, 64), (5, 8, 1, 7)]
IDS = ["%dx%dx%dx%d" % s for s in SHAPES]
LM = dict(lm_weight=0.5, length_bonus=0.1)


def _graph(phrases, boost, V):
    from edgedict_amd.bias import ContextGraph
    return ContextGraph(phrases, boost, V, blank=0, bos=-1)


def _prefix_lists(z, dtype, W, cand, **kw):
    """The offline search of every prefix z[:t], t = 0 .. T, in one call: host arrays (tokens, frames, token_lp, ntok,
    n_hyp, logp) whose row t is the list after t frames."""
    from edgedict_amd.loss import ctc_prefix_beam
    T = z.shape[0]
    tz = torch.tensor(z, device="cuda").to(_TORCH[dtype])[None].expand(T + 1, -1, -1).contiguous()
    act = torch.arange(T + 1, dtype=torch.int32, device="cuda")
    return [t.cpu().numpy() for t in ctc_prefix_beam(tz, act, W=W, blank=0, cand=cand, **kw)]


@functools.lru_cache(maxsize=None)
def _plain_case(shape, dtype, seed=None):
    z = BR.make_logits(shape[0], shape[1], BR.SEEDS[dtype][shape] if seed is None else seed, dtype == "bf16")
    return z, _prefix_lists(z, dtype, shape[2], shape[3])


def _same(res, off, t, what):
    """``res`` (an NBestResult) is row ``t`` of the offline arrays ``off``, bit for bit."""
    tokens, frames, tlp, ntok, nhyp, logp = off
    n = int(nhyp[t])
    assert len(res) == n, (what, len(res), n)
    assert res.logp.dtype == np.float64
    assert res.logp.view(np.int64).tolist() == np.ascontiguousarray(logp[t, :n]).view(np.int64).tolist(), what
    for h in range(n):
        k = int(ntok[t, h])
        assert res.tokens[h].tolist() == tokens[t, h, :k].tolist(), (what, h)
        assert res.frames[h].tolist() == frames[t, h, :k].tolist(), (what, h)
        got = res.token_logp[h].astype(np.float32)
        assert (got.astype(np.float64) == res.token_logp[h]).all(), (what, h)          # they were float32 values
        assert got.view(np.int32).tolist() == np.ascontiguousarray(tlp[t, h, :k]).view(np.int32).tolist(), (what, h)


def _same_results(a, b, what):
    assert len(a) == len(b), what
    assert a.logp.view(np.int64).tolist() == b.logp.view(np.int64).tolist(), what
    for h in range(len(a)):
        assert np.array_equal(a.tokens[h], b.tokens[h]) and np.array_equal(a.frames[h], b.frames[h]), (what, h)
        assert a.token_logp[h].view(np.int64).tolist() == b.token_logp[h].view(np.int64).tolist(), (what, h)


def _chunk(zs, pos, nf, Tc, dtype):
    """[S, Tc, V] on the device: stream s's frames pos[s] .. pos[s] + nf[s], NaN behind."""
    V = zs[0].shape[1]
    x = np.full((len(zs), Tc, V), np.nan, dtype=np.float32)
    for s, z in enumerate(zs):
        x[s, :nf[s]] = z[pos[s]:pos[s] + nf[s]]
    return torch.tensor(x, device="cuda").to(_TORCH[dtype])


def _stream(S, shape, **kw):
    from edgedict_amd.decode import StreamingCTCBeamSearch
    return StreamingCTCBeamSearch(S, shape[1], W=shape[2], cand=shape[3], blank=0, **kw)


def _check_committed(sb, results):
    """The committed log is a prefix of every hypothesis in tokens, frames and token_logp; returns its lengths."""
    detail, plain = sb.committed_detail(), sb.committed()
    for s, (r, (ct, cf, cl)) in enumerate(zip(results, detail)):
        assert ct.dtype == np.int64 and cf.dtype == np.int32 and cl.dtype == np.float64
        assert np.array_equal(plain[s], ct) and len(cf) == len(ct) == len(cl)
        k = len(ct)
        for i in range(len(r)):
            assert np.array_equal(r.tokens[i][:k], ct), (s, i)
            assert np.array_equal(r.frames[i][:k], cf), (s, i)
            assert np.array_equal(r.token_logp[i][:k], cl), (s, i)
    return [len(ct) for ct, _, _ in detail]


def _check_best_and_idle(sb, results, frames_done):
    seqs, scores = sb.best()
    idle = sb.idle_frames()
    assert scores.dtype == torch.float64 and idle.dtype == np.int64
    for s, r in enumerate(results):
        assert seqs[s].dtype == np.int64 and np.array_equal(seqs[s], r.tokens[0])
        assert scores[s].item() == -r.logp[0]
        fr = r.frames[0]
        assert idle[s] == (frames_done[s] - 1 - int(fr[-1]) if len(fr) else frames_done[s]), (s, idle[s])


def _run_chunks(sb, z, off, chunks, dtype, what, S=2):
    """Feed ``z`` to all S streams in ``chunks``; after every advance every stream is the offline list of the frames so
    far, the committed log a growing prefix of it."""
    t, seen = 0, [0] * S
    for n in chunks:
        sb.advance(_chunk([z] * S, [t] * S, [n] * S, n, dtype))
        t += n
        res = sb.nbest()
        for s in range(S):
            _same(res[s], off, t, (what, t, s))
        ks = _check_committed(sb, res)
        assert all(k >= k0 for k, k0 in zip(ks, seen)), (what, t)
        seen = ks
        _check_best_and_idle(sb, res, [t] * S)
    return seen


# ------------------------------------------------------------------------------------- 1. prefix equality, 7. idle
@pytest.mark.parametrize("kind", SR.CHUNKINGS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
@DTYPES
def test_every_chunk_leaves_the_offline_beam(hip_lib, shape, dtype, kind):
    """Two streams fed the same utterance: after each advance ``nbest()`` is ``ctc_prefix_beam`` over the frames so
    far.  W = 1 commits the whole hypothesis on every advance, so from the second chunk on the walk starts from a
    re-rooted root that carries a token."""
    z, off = _plain_case(shape, dtype)
    sb = _stream(2, shape)
    res = sb.nbest()
    for s in range(2):
        _same(res[s], off, 0, (shape, "fresh", s))
        assert len(res[s]) == 1 and len(res[s].tokens[0]) == 0 and res[s].logp[0] == 0.0
    chunks = SR.chunking(kind, shape[0])
    committed = _run_chunks(sb, z, off, chunks, dtype, (shape, dtype, kind))
    if shape[2] == 1:
        assert committed == [int(off[3][shape[0], 0])] * 2 and (sb.live_nodes() == 1).all()
        if kind == "ones":
            assert len(chunks) >= 3 and committed[0] >= 2


# ------------------------------------------------------------------------------------------------ 2. ragged streams
@DTYPES
def test_ragged_streams_and_one_that_sits_out_every_other_chunk(hip_lib, dtype):
    """ctc_beam_ref.RAGGED's utterances of 33, 0 and 1 frames as streams 0 .. 2, and stream 3 = the first utterance
    taken 4 frames at a time on even chunks only: different ``n_frames`` of the same chunk, 0 among them."""
    r = BR.RAGGED
    shape = lambda Tb: (Tb, r["V"], r["W"], r["cand"])
    cases = [_plain_case(shape(Tb), dtype, seed) if Tb else (np.zeros((0, r["V"]), np.float32), None)
             for Tb, seed in zip(r["T"], r["seeds"][dtype])]
    zs = [c[0] for c in cases] + [cases[0][0]]
    offs = [c[1] for c in cases] + [cases[0][1]]
    sb = _stream(4, shape(0))
    pos, Tc, k = [0, 0, 0, 0], 5, 0
    while pos[0] < 33 or pos[3] < 33:
        nf = [min(Tc, 33 - pos[0]), 0, 1 - pos[2], min(4, 33 - pos[3]) if k % 2 == 0 else 0]
        sb.advance(_chunk(zs, pos, nf, Tc, dtype), np.array(nf, dtype=np.int32))
        pos = [p + n for p, n in zip(pos, nf)]
        res = sb.nbest()
        for s in (0, 2, 3):
            _same(res[s], offs[s], pos[s], ("ragged", k, s))
        assert len(res[1]) == 1 and len(res[1].tokens[0]) == 0 and res[1].logp[0] == 0.0
        _check_committed(sb, res)
        _check_best_and_idle(sb, res, pos)
        assert (sb.frames_done() == np.array(pos)).all()
        k += 1
    assert pos == [33, 0, 1, 33]


# -------------------------------------------------------------------------------------------------------- 3. fusion
@functools.lru_cache(maxsize=None)
def _bias_case(shape, dtype):
    z, hyps, _, _ = BR.case(shape, dtype, BR.BIAS_SEEDS[dtype][shape])
    return z, _graph(BR.phrases_from(hyps[0].tokens), BR.BIAS_BOOST, shape[1])


@pytest.mark.parametrize("form", ["bias", "lm", "both"])
@pytest.mark.parametrize("shape", BR.BIAS_SHAPES, ids=["%dx%dx%dx%d" % s for s in BR.BIAS_SHAPES])
@DTYPES
def test_fused_forms_leave_the_offline_fused_beam(hip_lib, shape, dtype, form):
    z, g = _bias_case(shape, dtype)
    kw = {}
    if form != "lm":
        kw["bias"] = g
    if form != "bias":
        kw.update(lm=NR.model(shape[1], 3), **LM)
    off = _prefix_lists(z, dtype, shape[2], shape[3], **kw)
    plain = _prefix_lists(z, dtype, shape[2], shape[3])
    T = shape[0]
    assert off[0][T].tolist() != plain[0][T].tolist() or off[5][T].tolist() != plain[5][T].tolist()   # the terms act
    _run_chunks(_stream(2, shape, **kw), z, off, SR.chunking("357", T), dtype, (shape, dtype, form))


@DTYPES
def test_zero_weight_and_an_empty_list_are_the_plain_stream(hip_lib, dtype):
    shape = BR.BIAS_SHAPES[0]
    z, off = _plain_case(shape, dtype)
    zero = _stream(2, shape, bias=_graph([], 1.0, shape[1]), lm=NR.model(shape[1], 3), lm_weight=0.0, length_bonus=0.0)
    plain = _stream(2, shape)
    t = 0
    for n in SR.chunking("357", shape[0]):
        x = _chunk([z] * 2, [t] * 2, [n] * 2, n, dtype)
        zero.advance(x)
        plain.advance(x)
        t += n
        for a, b in zip(zero.nbest(), plain.nbest()):
            _same_results(a, b, (dtype, t))
            _same(a, off, t, (dtype, t))
        for a, b in zip(zero.committed_detail(), plain.committed_detail()):
            assert all(np.array_equal(u, v) for u, v in zip(a, b))


# ---------------------------------------------------------------------------------------------------- 4. compaction
def _live_of(off, t):
    n = int(off[4][t])
    paths = [list(zip(off[0][t, h, :off[3][t, h]].tolist(), off[1][t, h, :off[3][t, h]].tolist())) for h in range(n)]
    return SR.tree_after(paths)


@pytest.mark.parametrize("case", SR.COMPACTION, ids=["W1", "W10"])
@DTYPES
def test_small_capacity_compacts_on_every_advance(hip_lib, case, dtype):
    """A capacity the utterance's nodes exceed (tests/test_ctc_stream_host.py): the tree is compacted on every advance,
    the lists stay the offline lists, the live node count and the committed log are what the offline list's tree gives,
    and an advance beyond the capacity raises and changes nothing."""
    shape, step, NC = case
    T, V, W, cand = shape
    z, off = _plain_case(shape, dtype)
    sb = _stream(2, shape, node_capacity=NC)
    t, created = 0, 1
    while t < T:
        n = min(step, T - t)
        assert (sb.live_nodes() + n * W <= NC).all()
        sb.advance(_chunk([z] * 2, [t] * 2, [n] * 2, n, dtype))
        t += n
        res = sb.nbest()
        live, k = _live_of(off, t)
        for s in range(2):
            _same(res[s], off, t, (shape, t, s))
            ct, cf, cl = sb.committed_detail()[s]
            assert len(ct) == k and sb.live_nodes()[s] == live, (t, s, len(ct), k, sb.live_nodes()[s], live)
            assert ct.tolist() == off[0][t, 0, :k].tolist() and cf.tolist() == off[1][t, 0, :k].tolist()
            assert cl.astype(np.float32).view(np.int32).tolist() == np.ascontiguousarray(off[2][t, 0, :k]).view(np.int32).tolist()
        _check_committed(sb, res)
    before = sb.nbest()
    big = NC // W + 1
    with pytest.raises(RuntimeError, match="node_capacity"):
        sb.advance(torch.zeros(2, big, V, device="cuda", dtype=_TORCH[dtype]))
    for a, b in zip(before, sb.nbest()):
        _same_results(a, b, "after the refused advance")
    assert (sb.frames_done() == T).all()


# ----------------------------------------------------------------------------------------------- 5. reset and reuse
@DTYPES
def test_masked_reset_in_mid_utterance_and_set_bias_rules(hip_lib, dtype):
    shape = (47, 32, 10, 16)
    V = shape[1]
    z, off = _plain_case(shape, dtype)
    z2, off2 = _plain_case(shape, dtype, BR.BIAS_SEEDS[dtype][shape])
    sb = _stream(3, shape)
    sb.set_bias(None)
    zs, pos = [z, z, z], [0, 0, 0]
    for k, n in enumerate(SR.chunking("357", shape[0])):
        if k == 3:
            with pytest.raises(ValueError, match="advanced over"):
                sb.set_bias(_graph([[3, 4]], 1.0, V))
            with pytest.raises(ValueError, match="outside the mask"):
                sb.set_bias(None, mask=[False, False, False])
            before = sb.nbest()
            sb.reset(torch.tensor([False, True, False]))
            after = sb.nbest()
            _same_results(before[0], after[0], "stream 0 across the reset")
            _same_results(before[2], after[2], "stream 2 across the reset")
            assert len(after[1]) == 1 and len(after[1].tokens[0]) == 0 and after[1].logp[0] == 0.0
            assert len(sb.committed()[1]) == 0 and sb.live_nodes()[1] == 1 and sb.frames_done()[1] == 0
            zs[1], pos[1] = z2, 0
        sb.advance(_chunk(zs, pos, [n] * 3, n, dtype))
        pos = [p + n for p in pos]
        res = sb.nbest()
        _same(res[0], off, pos[0], ("kept", k, 0))
        _same(res[2], off, pos[2], ("kept", k, 2))
        _same(res[1], off2 if k >= 3 else off, pos[1], ("reset", k))
        _check_committed(sb, res)
        _check_best_and_idle(sb, res, pos)
    assert pos[1] < pos[0] == shape[0]
    sb.reset()
    sb.set_bias(_graph([[3, 4]], 1.0, V))          # every stream fresh: allowed
    assert sb.bias is not None


# ------------------------------------------------------------------------------------------------- 6. determinism
@DTYPES
def test_two_runs_are_equal_in_every_bit(hip_lib, dtype):
    shape = (65, 40, 10, 32)
    z, _ = _plain_case(shape, dtype)
    runs = []
    for _ in range(2):
        sb = _stream(2, shape)
        out, t = [], 0
        for n in SR.chunking("357", shape[0]):
            sb.advance(_chunk([z] * 2, [t] * 2, [n] * 2, n, dtype))
            t += n
            out.append((sb.nbest(), sb.committed_detail(), sb.live_nodes()))
        runs.append(out)
    for (ra, ca, la), (rb, cb, lb) in zip(*runs):
        for a, b in zip(ra, rb):
            _same_results(a, b, "run to run")
        for x, y in zip(ca, cb):
            assert all(np.array_equal(u, v) for u, v in zip(x, y))
        assert np.array_equal(la, lb)


# ------------------------------------------------------------------------------------------- 8. audio-level decoder
def test_audio_level_decoder_equals_the_search_on_its_own_head_logits(hip_lib):
    from edgedict_amd.decode import StreamingCTCBeamSearch
    from edgedict_amd.models import Transducer
    from edgedict_amd.stream import BatchedStreamCTCBeamDecoder, chunk_geometry
    from oracle import models_ref as M
    from oracle.make_golden_stream import GEOMETRIES, geometry_flags
    from test_stream_beam_gpu import STREAM_CFG
    geo, flags = GEOMETRIES["native"], geometry_flags("native")
    cfg = dict(STREAM_CFG, input_size=geo.I0)
    torch.manual_seed(11)
    m = Transducer(enc_dropout=0.0, dec_dropout=0.0, ctc_weight=0.3, **cfg)
    m.load_state_dict(M.make_state_dict(cfg, 5), strict=False)
    m = m.cuda().eval()
    m.compute_dtype = "fp32"
    Sn, W, V = 4, 4, cfg["vocab_size"]
    win, hop = chunk_geometry(flags, geo.step_n_frame)
    wave = (0.1 * torch.randn(Sn, win + 5 * hop, generator=torch.Generator().manual_seed(0))).cuda()
    dec = BatchedStreamCTCBeamDecoder(m, flags, Sn, W=W, cand=8, dither=0)
    sb = StreamingCTCBeamSearch(Sn, V, W=W, cand=8, blank=m.blank)
    L, H = len(m.encoder.lstm.lstms), m.encoder.lstm.hidden_size
    h = torch.zeros(L, Sn, H, device="cuda")
    c = torch.zeros(L, Sn, H, device="cuda")
    frames = 0
    with torch.no_grad():
        for k in range(6):
            chunk = wave[:, k * hop:k * hop + win].contiguous()
            got, gsc = dec.decode(chunk.clone())
            xs, _ = dec.transform(chunk.clone())
            enc, (h, c) = m.encoder(xs, (h, c))
            sb.advance(m._ctc_logits(enc.contiguous()).contiguous())
            frames += enc.shape[1]
            res, want = dec.nbest(), sb.nbest()
            for s in range(Sn):
                _same_results(res[s], want[s], (k, s))
                assert np.array_equal(got[s], want[s].tokens[0]) and gsc[s].item() == -want[s].logp[0]
                assert np.array_equal(dec.committed()[s], sb.committed()[s])
                assert all(np.array_equal(u, v) for u, v in zip(dec.committed_detail()[s], sb.committed_detail()[s]))
            assert np.array_equal(dec.idle_frames(), sb.idle_frames())
            assert (sb.frames_done() == frames).all()
    assert frames == 6 * geo.T_out
    plain = Transducer(enc_dropout=0.0, dec_dropout=0.0, **cfg).cuda().eval()
    with pytest.raises(RuntimeError, match="no CTC head"):
        BatchedStreamCTCBeamDecoder(plain, flags, Sn)
