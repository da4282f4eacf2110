"""GPU: N-best lists with token frames and log-probs (decode.beam_search_nbest, StreamingBeamSearch(detail=True);
csrc/decode.hip beam_pop_detail, beam_compact_detail, beam_read_paths) against the CPU restatement tests/nbest_ref.py
(pinned on oracle/beam_ref.py by tests/test_nbest_host.py), against a path re-scoring through the model's own dense
lattice that knows nothing of the restatement, against the Viterbi aligner, and streaming against offline.

Whole-list equality between an fp32 search on the device and the CPU restatement holds only where no pop is a
near-tie, so every input compared exactly has its smallest gap between the best and the second-best candidate of A over
all pops measured on the CPU (``nbest_ref``) and asserted >= 1e-3, five times the 2e-4 score tolerance.  Measured gaps:
    golden tiny model    W = 1: 3.7e-2    W = 4: 4.3e-3    W = 10: 2.5e-3    (W = 4, one row of 0 frames: 4.3e-3)
    random model, state dict seed 39 / batch seed 40, xlen [17, 9, 17, 3, 12], W = 4: 1.26e-3
        (seeds 3 / 4 of tests/test_beam_gpu.py: 1.6e-5, and of the seeds 20..139 only 39 reaches 1e-3: flat distributions)
    golden tiny model + LM (seed 11, scale 3), lm_weight 0.3, length_bonus 0.4, W = 4: 3.5e-3"""
import functools
import os

import numpy as np
import pytest
import torch

import nbest_ref as N
from oracle import models_ref as M

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(os.path.dirname(__file__), "golden", "beam_tiny.npz"))
CFG = dict(vocab_embed_size=16, vocab_size=40, input_size=24, enc_hidden_size=32, enc_layers=2,
           enc_proj_size=24, dec_hidden_size=32, dec_layers=2, dec_proj_size=24, joint_size=32)
TOL = dict(rtol=2e-4, atol=2e-4)
MIN_GAP = 1e-3


def _engine(sd, dtype="fp32"):
    from edgedict_amd.models import Transducer
    m = Transducer(enc_dropout=0.0, dec_dropout=0.0, output_loss=False, **CFG)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    m.compute_dtype = dtype
    return m


def _golden_sd():
    return {k[3:]: torch.from_numpy(G[k]) for k in G.files if k.startswith("sd/")}


def _inputs(name):
    if name == "random":
        sd = M.make_state_dict(CFG, 39)
        xs, _, _, _ = M.make_batch(CFG, 40, 5, 17, 4)
        return sd, xs, torch.tensor([17, 9, 17, 3, 12], dtype=torch.int32)
    xlen = torch.from_numpy(G["xlen"]).clone()
    if name == "zero_row":
        xlen[1] = 0
    return _golden_sd(), torch.from_numpy(G["xs"]), xlen


@functools.lru_cache(maxsize=None)
def _reference(name, W):
    """(per-utterance lists B, total expansions, smallest pop gap) of the CPU restatement: computed once, read only."""
    sd, xs, xlen = _inputs(name)
    return N.nbest(sd, xs, xlen, W=W)


def _check_shape(r, W, T, V=CFG["vocab_size"]):
    assert 1 <= len(r) <= W and r.logp.dtype == np.float64 and r.logp.shape == (len(r),)
    for t, f, l in zip(r.tokens, r.frames, r.token_logp):
        assert t.dtype == np.int64 and f.dtype == np.int32 and l.dtype == np.float64
        assert len(t) == len(f) == len(l)
        assert ((t > 0) & (t < V)).all()
        assert (np.diff(f) >= 0).all() and ((f >= 0) & (f < max(T, 1))).all()


# ------------------------------------------------------------------------------------------- 1. against the helper
@pytest.mark.parametrize("name,W", [("golden", 1), ("golden", 4), ("golden", 10), ("random", 4), ("zero_row", 4)])
def test_offline_nbest_matches_the_restatement(hip_lib, name, W):
    from edgedict_amd import decode
    sd, xs, xlen = _inputs(name)
    ref, rexp, gap = _reference(name, W)
    assert gap >= MIN_GAP, gap
    m = _engine(sd)
    with torch.no_grad():
        res = m.beam_search_nbest(xs.cuda(), xlen, W=W, max_expansions=400)
        nexp = decode.beam_search_batch.last_expansions
        seqs, scores = m.beam_search(xs.cuda(), xlen, W=W, max_expansions=400)
        assert decode.beam_search_batch.last_expansions == nexp
    assert nexp == rexp
    lens = N.encode(sd, xs, xlen)[1]
    assert len(res) == xs.shape[0]
    for b, (r, want) in enumerate(zip(res, ref)):
        _check_shape(r, W, lens[b])
        assert len(r) == len(want), (b, len(r), len(want))
        for i, h in enumerate(want):
            assert np.array_equal(r.tokens[i], h["tokens"]), (b, i, r.tokens[i], h["tokens"])
            assert np.array_equal(r.frames[i], h["frames"]), (b, i, r.frames[i], h["frames"])
            np.testing.assert_allclose(r.token_logp[i], np.asarray(h["token_logp"], dtype=np.float64), **TOL)
        np.testing.assert_allclose(r.logp, [h["logp"] for h in want], **TOL)
        # entry 0 is what beam_search returns: same tokens, same score bits
        assert np.array_equal(r.tokens[0], seqs[b])
        assert -r.logp[0] == scores[b].item()
    if name == "zero_row":
        r = res[1]
        assert len(r) == 1 and len(r.tokens[0]) == 0 and len(r.frames[0]) == 0 and r.logp[0] == 0.0


# ------------------------------------------------------------------------------------------- 2. path re-scoring
def _lattices(m, xs, xlen, tokens):
    """Dense fp32 logits [1, T, U + 1, V] of utterance rows for the label sequences ``tokens`` (one utterance each), from
    the model's own encoder, prediction network and joint."""
    with torch.no_grad():
        h_enc, _ = m.encoder(xs.cuda())
        lens = m.scale_length(h_enc, xlen)
        out = []
        for b, ys in tokens:
            y = torch.tensor([list(ys)], dtype=torch.int32).reshape(1, len(ys)).cuda()
            h_dec, _ = m.decoder(y)
            out.append(m.joint(h_enc[b:b + 1, :int(lens[b])].contiguous(), h_dec).float().contiguous())
    return out, [int(v) for v in lens]


@pytest.mark.parametrize("name,W", [("golden", 4), ("golden", 10), ("random", 4)])
def test_detail_rescores_through_the_dense_lattice_and_viterbi_bounds_it(hip_lib, name, W):
    from edgedict_amd.loss import rnnt_align
    sd, xs, xlen = _inputs(name)
    m = _engine(sd)
    with torch.no_grad():
        res = m.beam_search_nbest(xs.cuda(), xlen, W=W, max_expansions=400)
    todo = sorted({(b, tuple(int(k) for k in t)) for b, r in enumerate(res) for t in r.tokens})
    logits, lens = _lattices(m, xs, xlen, todo)
    lat = {key: z for key, z in zip(todo, logits)}
    n_checked = 0
    for b, r in enumerate(res):
        _check_shape(r, W, lens[b])
        for i in range(len(r)):
            toks = tuple(int(k) for k in r.tokens[i])
            z = lat[(b, toks)]
            lp = torch.log_softmax(z[0].double(), dim=-1).cpu().numpy()
            total, terms = N.path_logp(lp, toks, r.frames[i], blank=int(m.blank))
            np.testing.assert_allclose(total, r.logp[i], **TOL)
            np.testing.assert_allclose(r.token_logp[i], terms, **TOL)
            if toks:        # Viterbi is the maximum over the paths of this transcript
                U = len(toks)
                fr, sc = rnnt_align(z, torch.tensor([toks], dtype=torch.int32).cuda(),
                                    torch.tensor([lens[b]], dtype=torch.int32).cuda(),
                                    torch.tensor([U], dtype=torch.int32).cuda(), int(m.blank))
                assert sc[0].item() >= r.logp[i] - 2e-4, (b, i, sc[0].item(), r.logp[i])
                assert fr.shape == (1, U)
                n_checked += 1
    assert n_checked > 0


# ------------------------------------------------------------------------------------------- 3. streaming
def _same_nbest(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert len(g) == len(w)
        for i in range(len(w)):
            assert np.array_equal(g.tokens[i], w.tokens[i]), (g.tokens[i], w.tokens[i])
            assert np.array_equal(g.frames[i], w.frames[i]), (g.frames[i], w.frames[i])
            assert np.array_equal(g.token_logp[i], w.token_logp[i]), (g.token_logp[i], w.token_logp[i])
        assert np.array_equal(g.logp, w.logp), (g.logp, w.logp)


def _prefix_holds(sb):
    nb = sb.nbest()
    for (ct, cf, cl), r, c in zip(sb.committed_detail(), nb, sb.committed()):
        assert ct.dtype == np.int64 and cf.dtype == np.int32 and cl.dtype == np.float64
        assert np.array_equal(ct, c) and len(ct) == len(cf) == len(cl)
        for i in range(len(r)):
            assert np.array_equal(r.tokens[i][:len(ct)], ct)
            assert np.array_equal(r.frames[i][:len(cf)], cf)
            assert np.array_equal(r.token_logp[i][:len(cl)], cl)
    return nb


def _rows(m, enc):
    """The joint's encoder rows [S, T, J] of enc [S, T, P], computed ONCE: the streaming and the offline search read the
    same values whatever the chunking (as tests/test_stream_beam_gpu.py arranges it)."""
    from edgedict_amd import decode
    S, T, P = enc.shape
    return decode.joint_rows(m, enc.contiguous()).reshape(S, T, -1)


def _offline(m, rows, P, lens, W, EM):
    from edgedict_amd import decode
    S, T, J = rows.shape
    return decode.beam_search_nbest_rows(m, rows.reshape(S * T, J).contiguous(), S, T, P, lens, W, EM)


def _stream(m, rows, P, lens, chunk, W, EM, NC=None):
    """Feed rows [S, T, J] in chunks of ``chunk`` frames, stream s stopping after lens[s]; after every chunk the
    committed log is a prefix of every hypothesis."""
    from edgedict_amd import decode
    S, T, J = rows.shape
    sb = decode.StreamingBeamSearch(m, S, W=W, max_expansions=EM, node_capacity=NC, detail=True)
    for t in range(0, T, chunk):
        piece = rows[:, t:t + chunk].contiguous()
        n = piece.shape[1]
        nf = np.clip(np.asarray(lens) - t, 0, n).astype(np.int32)
        sb.advance_rows(piece.reshape(S * n, J), P, nf)
        _prefix_holds(sb)
    return sb


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_streaming_nbest_equals_offline(hip_lib, dtype):
    from edgedict_amd import decode
    m = _engine(_golden_sd(), dtype)
    with torch.no_grad():
        enc, _ = m.encoder(torch.from_numpy(G["xs"]).cuda())
    S, T, P = enc.shape
    rows = _rows(m, enc)
    lens = [T, 7, T - 1]
    W, EM = 4, 64
    want = _offline(m, rows, P, lens, W, EM)
    wexp = decode.beam_search_batch.last_expansions
    assert any(len(t) > 1 for r in want for t in r.tokens)
    # EM + 64 nodes: one frame's pops on top of at most 64 live nodes (4 survivors x at most T tokens below their common
    # ancestor) - every chunk starts from a compacted tree, LDS mode; 5000 > 4096 nodes: the global-memory mode
    for chunk, NC in ((1, None), (2, None), (5, None), (1, EM + 64), (2, 5000), (5, 5000)):
        sb = _stream(m, rows, P, lens, chunk, W, EM, NC)
        _same_nbest(_prefix_holds(sb), want)
        assert int(sb.expansions().sum()) == wexp
        best, bsc = sb.best()
        for s, r in enumerate(want):
            assert np.array_equal(best[s], r.tokens[0]) and -r.logp[0] == bsc[s].item()


def test_streaming_frames_survive_a_masked_reset(hip_lib):
    from edgedict_amd import decode
    m = _engine(_golden_sd())
    with torch.no_grad():
        enc, _ = m.encoder(torch.from_numpy(G["xs"]).cuda())
    S, T, P = enc.shape
    rows = _rows(m, enc)
    J = rows.shape[2]
    W, EM, cut = 4, 64, 4
    sb = decode.StreamingBeamSearch(m, S, W=W, max_expansions=EM, detail=True)
    for t in range(0, T, 2):
        if t == cut:
            sb.reset(torch.tensor([0, 1, 0]))
            assert len(sb.committed_detail()[1][0]) == 0
        piece = rows[:, t:t + 2].contiguous()
        sb.advance_rows(piece.reshape(S * piece.shape[1], J), P)
    got = _prefix_holds(sb)
    whole = _offline(m, rows, P, None, W, EM)
    tail = _offline(m, rows[1:2, cut:].contiguous(), P, None, W, EM)
    _same_nbest([got[0], got[2]], [whole[0], whole[2]])       # absolute frames, counted from these streams' start
    _same_nbest([got[1]], tail)                               # counted from the reset
    assert max(int(f.max()) for f in got[0].frames if len(f)) >= cut


@pytest.mark.parametrize("NC", [3 * 32 + 400, 4500])
def test_long_stream_in_chunks_of_three_loses_nothing(hip_lib, NC):
    """64 frames in chunks of 3 (22 advances, a compaction after each) with a tree bounded below the 64 x 32 + 1 nodes
    of the offline search: 3 frames' pops on top of at most 400 live nodes (4 survivors x at most 64 tokens), LDS mode,
    and the global-memory mode.  A second stream sits out the first 54 frames and then reads 10: its frames count from
    its own first frame, whatever the other stream has done.  (The trained tiny model emits its tokens in the first
    frames of a stream and blanks after them - the CPU restatement gives 5 tokens on such a stream - so all this asks of
    the input is that something gets committed; equality with the offline lists is the check.)"""
    m = _engine(_golden_sd())
    with torch.no_grad():
        enc, _ = m.encoder(torch.from_numpy(G["xs"]).cuda())
    P = enc.shape[2]
    long = torch.cat([enc[:1]] * 6 + [enc[1:2]], dim=1)[:, :64]
    late = torch.cat([torch.zeros_like(long[:, :54]), enc[1:2, :10]], dim=1)
    rows = _rows(m, torch.cat([long, late], dim=0).contiguous())
    S, T, J = rows.shape
    assert (S, T) == (2, 64)
    W, EM = 4, 32
    assert NC < T * EM + 1 or NC > 4096         # bounded below the offline tree, or the global-memory mode
    want = _offline(m, rows[:1].contiguous(), P, None, W, EM) + _offline(m, rows[1:, 54:].contiguous(), P, None, W, EM)
    from edgedict_amd import decode
    sb = decode.StreamingBeamSearch(m, S, W=W, max_expansions=EM, node_capacity=NC, detail=True)
    for t in range(0, T, 3):
        piece = rows[:, t:t + 3].contiguous()
        n = piece.shape[1]
        sb.advance_rows(piece.reshape(S * n, J), P, np.array([n, n if t >= 54 else 0], dtype=np.int32))
        _prefix_holds(sb)
    _same_nbest(_prefix_holds(sb), want)
    assert len(sb.committed_detail()[0][0]) > 0
    assert all(int(f.max()) < 10 for f in want[1].frames if len(f))


# ------------------------------------------------------------------------------------------- 4. LM fusion
def test_lm_zero_weight_is_bit_equal_and_fused_matches_the_restatement(hip_lib):
    from test_lm_fusion_gpu import RefLM, _lm, _lm_sd
    sd, xs, xlen = _inputs("golden")
    m = _engine(sd)
    W = 4
    lm_sd = _lm_sd(40, 16, 32, 2, seed=11, scale=3.0)
    lm = _lm(lm_sd)
    with torch.no_grad():
        plain = m.beam_search_nbest(xs.cuda(), xlen, W=W, max_expansions=400)
        zero = m.beam_search_nbest(xs.cuda(), xlen, W=W, max_expansions=400, lm=lm, lm_weight=0.0, length_bonus=0.0)
    _same_nbest(zero, plain)
    lw, bonus = 0.3, 0.4
    ref_lm = RefLM(lm_sd)
    ref, rexp, gap = N.nbest(sd, xs, xlen, W=W, lm=ref_lm, lm_weight=lw, length_bonus=bonus)
    assert gap >= MIN_GAP, gap
    from edgedict_amd import decode
    with torch.no_grad():
        res = m.beam_search_nbest(xs.cuda(), xlen, W=W, max_expansions=400, lm=lm, lm_weight=lw, length_bonus=bonus)
        assert decode.beam_search_batch.last_expansions == rexp
        seqs, scores = m.beam_search(xs.cuda(), xlen, W=W, max_expansions=400, lm=lm, lm_weight=lw, length_bonus=bonus)
    todo = sorted({(b, tuple(int(k) for k in t)) for b, r in enumerate(res) for t in r.tokens})
    logits, lens = _lattices(m, xs, xlen, todo)
    lat = {key: z for key, z in zip(todo, logits)}
    for b, (r, want) in enumerate(zip(res, ref)):
        assert len(r) == len(want)
        assert np.array_equal(r.tokens[0], seqs[b]) and -r.logp[0] == scores[b].item()
        for i, h in enumerate(want):
            assert np.array_equal(r.tokens[i], h["tokens"]) and np.array_equal(r.frames[i], h["frames"])
            np.testing.assert_allclose(r.token_logp[i], np.asarray(h["token_logp"], dtype=np.float64), **TOL)
            # sum of the increments + the blank terms of the lattice = the fused log p; and an increment is the lattice's
            # token term plus the LM term lm_weight * lp_lm + length_bonus
            toks = h["tokens"]
            lp = torch.log_softmax(lat[(b, tuple(toks))][0].double(), dim=-1).cpu().numpy()
            total, terms = N.path_logp(lp, toks, r.frames[i], blank=int(m.blank))
            blanks = total - terms.sum()
            np.testing.assert_allclose(r.token_logp[i].sum() + blanks, r.logp[i], **TOL)
            hidden, prev, lm_terms = ref_lm.zero(), 1, []
            for k in toks:
                lpl, hidden = ref_lm.forward(torch.tensor([[prev]]), hidden)
                lm_terms.append(lw * float(lpl[0, k]) + bonus)
                prev = k
            np.testing.assert_allclose(r.token_logp[i], terms + np.asarray(lm_terms), **TOL)
        np.testing.assert_allclose(r.logp, [h["logp"] for h in want], **TOL)


# ------------------------------------------------------------------------------------------- 5. bf16
def test_bf16_nbest_is_valid_and_entry_zero_is_the_plain_search(hip_lib):
    sd, xs, xlen = _inputs("golden")
    m = _engine(sd, "bf16")
    with torch.no_grad():
        res = m.beam_search_nbest(xs.cuda(), xlen, W=4)
        seqs, scores = m.beam_search(xs.cuda(), xlen, W=4)
    lens = N.encode(sd, xs, xlen)[1]
    for b, r in enumerate(res):
        _check_shape(r, 4, lens[b])
        assert np.isfinite(r.logp).all() and (r.logp <= 0).all()
        assert np.array_equal(r.tokens[0], seqs[b]) and -r.logp[0] == scores[b].item()
        for l in r.token_logp:
            assert np.isfinite(l).all()


# ------------------------------------------------------------------------------------------- 6. errors
def test_prefix_with_detail_is_refused(hip_lib):
    import ctypes
    from edgedict_amd import decode
    sd, xs, xlen = _inputs("golden")
    m = _engine(sd)
    with torch.no_grad():
        enc, _ = m.encoder(xs.cuda())
    with pytest.raises(ValueError, match="prefix"):
        decode.beam_search_nbest_enc(m, enc.contiguous(), None, 4, prefix=True)
    with pytest.raises(ValueError, match="prefix"):
        decode.StreamingBeamSearch(m, 2, W=4, prefix=True, detail=True)
    # ... and by the native call itself, with a status code, before it looks at anything else
    rc = hip_lib.edgedict_beam_search_nbest(*([None, None, ctypes.c_longlong(0), ctypes.c_longlong(0), 1, 1, None, 0, 0]
                                              + [1] + [None] * 13))
    assert rc == -1 and b"prefix" in hip_lib.edgedict_last_error()


def test_nbest_without_detail_raises(hip_lib):
    from edgedict_amd import decode
    m = _engine(_golden_sd())
    sb = decode.StreamingBeamSearch(m, 2, W=4)
    with pytest.raises(RuntimeError, match="detail=True"):
        sb.nbest()
    with pytest.raises(RuntimeError, match="detail=True"):
        sb.committed_detail()
    seqs, sc = sb.best()
    assert all(len(s) == 0 for s in seqs)


def test_too_small_max_tokens_or_node_capacity_is_an_error_not_a_truncation(hip_lib):
    from edgedict_amd import decode
    sd, xs, xlen = _inputs("golden")
    m = _engine(sd)
    with torch.no_grad():
        enc, _ = m.encoder(xs.cuda())
    enc = enc.contiguous()
    S, T, P = enc.shape
    E1 = decode.joint_rows(m, enc)
    full = decode.beam_search_nbest_rows(m, E1, S, T, P, None, 4)
    longest = max(len(t) for r in full for t in r.tokens)
    assert longest >= 2
    _same_nbest(decode.beam_search_nbest_rows(m, E1, S, T, P, None, 4, max_tokens=longest), full)
    with pytest.raises(RuntimeError, match="max_tokens"):
        decode.beam_search_nbest_rows(m, E1, S, T, P, None, 4, max_tokens=longest - 1)
    sb = decode.StreamingBeamSearch(m, S, W=4, max_expansions=32, node_capacity=40, detail=True)
    with pytest.raises(RuntimeError, match="node_capacity"):
        sb.advance(enc[:, :2].contiguous())
    nb = sb.nbest()             # the check runs before anything: the state is as it was
    assert all(len(r) == 1 and len(r.tokens[0]) == 0 and r.logp[0] == 0.0 for r in nb)
