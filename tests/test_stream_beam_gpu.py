"""GPU: streaming beam search (decode.StreamingBeamSearch, stream.BatchedStreamBeamDecoder) against the offline search
over the same frames: after every chunk the best hypothesis, its fp64 score and the expansion count equal what one
offline call over the frames so far returns; ragged chunks and masked resets equal independent single streams; a long
stream keeps a bounded token tree and loses nothing to compaction; too small a tree is an error, not a truncation."""
import os

import numpy as np
import pytest
import torch

from oracle import beam_ref, models_ref as M

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(os.path.dirname(__file__), "golden", "beam_tiny.npz"))
CFG = dict(vocab_embed_size=16, vocab_size=40, input_size=24, enc_hidden_size=32, enc_layers=2,
           enc_proj_size=24, dec_hidden_size=32, dec_layers=2, dec_proj_size=24, joint_size=32)


def _engine(sd, dtype="fp32", cfg=CFG):
    from edgedict_amd.models import Transducer
    m = Transducer(enc_dropout=0.0, dec_dropout=0.0, output_loss=False, **cfg)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    m.compute_dtype = dtype
    return m


def _golden_sd():
    return {k[3:]: torch.from_numpy(G[k]) for k in G.files if k.startswith("sd/")}


def _splits(T, kind, seed=0):
    if kind == "ragged":
        rng = np.random.default_rng(seed)
        out, t = [], 0
        while t < T:
            n = int(rng.integers(1, 6))
            out.append(min(n, T - t))
            t += out[-1]
        return out
    return [min(kind, T - t) for t in range(0, T, kind)]


def _offline(m, rows, P, W, EM, lens=None):
    """The offline search over the concatenation of per-chunk rows ([S, t, J] pieces)."""
    from edgedict_amd import decode
    S = rows[0].shape[0]
    E1 = torch.cat(rows, dim=1).reshape(-1, rows[0].shape[2]).contiguous()
    seqs, sc = decode.beam_search_rows(m, E1, S, E1.shape[0] // S, P, lens, W=W, max_expansions=EM)
    return seqs, sc, decode.beam_search_batch.last_expansions


def _same(a_seqs, a_sc, b_seqs, b_sc):
    assert len(a_seqs) == len(b_seqs)
    for x, y in zip(a_seqs, b_seqs):
        assert x.dtype == np.int64 and np.array_equal(x, y), (x, y)
    assert a_sc.dtype == torch.float64
    assert np.array_equal(a_sc.numpy(), b_sc.numpy()), (a_sc, b_sc)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("W", [1, 4, 10])
def test_chunking_invariance_against_the_offline_search(hip_lib, W, dtype):
    from edgedict_amd import decode
    sd = _golden_sd()
    m = _engine(sd, dtype)
    xs = torch.from_numpy(G["xs"]).cuda()
    with torch.no_grad():
        enc, _ = m.encoder(xs)
    enc = enc.contiguous()
    S, T, P = enc.shape
    EM = max(16, 8 * W)
    final = None
    for kind in (1, 3, 7, "ragged"):
        sb = decode.StreamingBeamSearch(m, S, W=W)
        rows, t = [], 0
        for n in _splits(T, kind, seed=W):
            chunk = enc[:, t:t + n].contiguous()
            rows.append(sb.joint_rows(chunk).reshape(S, n, -1))
            sb.advance(chunk)
            t += n
            got, gsc = sb.best()
            want, wsc, wexp = _offline(m, rows, P, W, EM)
            _same(got, gsc, want, wsc)
            assert int(sb.expansions().sum()) == wexp
            for c, g in zip(sb.committed(), got):
                assert np.array_equal(c, g[:len(c)])
        if final is not None:
            _same(got, gsc, final[0], final[1])
        final = (got, gsc)
    if dtype == "fp32":
        rs, rsc, _ = beam_ref.beam_search(sd, torch.from_numpy(G["xs"]), None, W=W)
        for a, b in zip(final[0], rs):
            assert np.array_equal(a, b)
        np.testing.assert_allclose(final[1].numpy(), rsc, rtol=2e-4, atol=2e-4)


def test_joint_rows_do_not_depend_on_the_number_of_rows(hip_lib):
    """The E1 product's row r is the same whether it is computed with the others or alone (these shapes)."""
    from edgedict_amd import decode
    m = _engine(_golden_sd())
    with torch.no_grad():
        enc, _ = m.encoder(torch.from_numpy(G["xs"]).cuda())
    enc = enc.contiguous()
    full = decode.joint_rows(m, enc).reshape(enc.shape[0], enc.shape[1], -1)
    for t in range(enc.shape[1]):
        part = decode.joint_rows(m, enc[:, t:t + 1].contiguous()).reshape(enc.shape[0], 1, -1)
        assert torch.equal(part, full[:, t:t + 1])


def _blanky_model(seed, bias=2.0, dtype="fp32"):   # random weights, blank favoured
    sd = M.make_state_dict(CFG, seed)
    sd["joint.joint.2.bias"][0] += bias
    return sd, _engine(sd, dtype)


def test_ragged_frames_and_masked_reset_equal_independent_streams(hip_lib):
    from edgedict_amd import decode
    m = _engine(_golden_sd())           # the trained tiny model: the streams emit tokens
    with torch.no_grad():
        full, _ = m.encoder(torch.from_numpy(G["xs"]).cuda())
    Tf = full.shape[1]
    S, W, EM = 5, 4, 400
    P = CFG["enc_proj_size"]
    frames = [[2, 0, 3, 1, 3], [1, 3, 0, 3, 2], [3, 3, 3, 0, 1], [0, 2, 1, 3, 3], [2, 1, 3, 2, 0], [3, 0, 2, 1, 3]]
    sb = decode.StreamingBeamSearch(m, S, W=W, max_expansions=EM)
    singles = [decode.StreamingBeamSearch(m, 1, W=W, max_expansions=EM) for _ in range(S)]
    for k, nf in enumerate(frames):
        # stream s reads utterance s % 3 from frame 2 s on, wrapping around
        idx = torch.tensor([[(2 * s + 3 * k + j) % Tf for j in range(3)] for s in range(S)])
        enc = torch.stack([full[s % 3, idx[s].cuda()] for s in range(S)]).contiguous()
        E1 = sb.joint_rows(enc)
        sb.advance_rows(E1, P, nf)
        rows = E1.reshape(S, 3, -1)
        for s in range(S):
            if nf[s]:
                singles[s].advance_rows(rows[s, :nf[s]].contiguous(), P)
        if k == 2:
            sb.reset(torch.tensor([0, 1, 0, 0, 1]))
            singles[1].reset()
            singles[4].reset()
        got, gsc = sb.best()
        for s in range(S):
            one, osc = singles[s].best()
            assert np.array_equal(got[s], one[0]), (k, s)
            np.testing.assert_allclose(gsc[s].item(), osc[0].item(), rtol=1e-6)
            assert np.array_equal(sb.committed()[s], singles[s].committed()[0])
    assert int(sb.expansions()[1]) == int(singles[1].expansions()[0])
    assert any(len(x) for x in got)


def test_long_stream_bounded_tree_loses_nothing(hip_lib):
    from edgedict_amd import decode
    sd = _golden_sd()
    m = _engine(sd)
    xs = torch.from_numpy(G["xs"])
    xlen = G["xlen"]
    utt = torch.cat([xs[b, :int(xlen[b])] for b in range(xs.shape[0])], 0)
    reps = 4000 // utt.shape[0] + 2
    long_xs = utt.repeat(reps, 1)[None].cuda()
    with torch.no_grad():
        enc, _ = m.encoder(long_xs)
    enc = enc.contiguous()
    T, P = enc.shape[1], enc.shape[2]
    assert T >= 2000
    W, EM, NC = 4, 32, 1024
    assert NC * 4 < T * EM
    sb = decode.StreamingBeamSearch(m, 1, W=W, max_expansions=EM, node_capacity=NC)
    rows = []
    step = 10
    for t in range(0, T, step):
        chunk = enc[:, t:t + step].contiguous()
        rows.append(sb.joint_rows(chunk).reshape(1, chunk.shape[1], -1))
        sb.advance(chunk)
        if (t // step) % 20 == 0 or t + step >= T:
            got, _ = sb.best()
            c = sb.committed()[0]
            assert np.array_equal(c, got[0][:len(c)])
    got, gsc = sb.best()
    want, wsc, wexp = _offline(m, rows, P, W, EM)
    _same(got, gsc, want, wsc)
    assert int(sb.expansions()[0]) == wexp
    assert len(sb.committed()[0]) > 0


def test_node_capacity_too_small_is_an_error_not_a_truncation(hip_lib):
    from edgedict_amd import decode
    sd, m = _blanky_model(5)
    P = CFG["enc_proj_size"]
    sb = decode.StreamingBeamSearch(m, 2, W=4, max_expansions=32, node_capacity=40)
    enc = torch.randn(2, 2, P, generator=torch.Generator().manual_seed(1)).cuda()
    with pytest.raises(RuntimeError, match="node_capacity"):
        sb.advance(enc)
    # the check runs before anything: the state is as it was
    seqs, sc = sb.best()
    assert all(len(s) == 0 for s in seqs) and np.array_equal(sc.numpy(), np.zeros(2))


STREAM_CFG = dict(vocab_embed_size=16, vocab_size=64, input_size=240, enc_hidden_size=64, enc_layers=3,
                  enc_proj_size=48, dec_hidden_size=32, dec_layers=2, dec_proj_size=32, joint_size=64)


@pytest.mark.parametrize("geometry", ["native", "hop640", "one_frame"])
def test_audio_level_decoder_equals_offline_search_over_the_module_path(hip_lib, geometry):
    """native: 2 stacked frames of 240 features per chunk; hop640: 3 of 160, the odd count zero-padded by the time
    reduction in every chunk; one_frame: a lone frame of 240 (oracle.make_golden_stream.GEOMETRIES)."""
    from edgedict_amd import decode
    from edgedict_amd.stream import BatchedStreamBeamDecoder, chunk_geometry
    from oracle.make_golden_stream import GEOMETRIES, geometry_flags
    geo, flags = GEOMETRIES[geometry], geometry_flags(geometry)
    cfg = dict(STREAM_CFG, input_size=geo.I0)
    sd = M.make_state_dict(cfg, 5)
    sd["joint.joint.2.bias"][0] += 1.0
    m = _engine(sd, "fp32", cfg)
    S, W = 3, 4
    win, hop = chunk_geometry(flags, geo.step_n_frame)
    assert (win, hop) == (geo.win, geo.hop)
    g = torch.Generator().manual_seed(0)
    wave = (0.1 * torch.randn(S, win + 5 * hop, generator=g)).cuda()
    dec = BatchedStreamBeamDecoder(m, flags, S, W=W, dither=0)
    L, H = len(m.encoder.lstm.lstms), m.encoder.lstm.hidden_size
    h = torch.zeros(L, S, H, device="cuda")
    c = torch.zeros(L, S, H, device="cuda")
    rows = []
    with torch.no_grad():
        for k in range(6):
            chunk = wave[:, k * hop:k * hop + win].contiguous()
            got, gsc = dec.decode(chunk.clone())
            xs, _ = dec.transform(chunk.clone())
            assert tuple(xs.shape) == (S, geo.T0, geo.I0)
            enc, (h, c) = m.encoder(xs, (h, c))
            enc = enc.contiguous()
            assert enc.shape[1] == geo.T_out
            rows.append(decode.joint_rows(m, enc).reshape(S, enc.shape[1], -1))
            want, wsc, _ = _offline(m, rows, enc.shape[2], W, max(16, 8 * W))
            _same(got, gsc, want, wsc)
    with pytest.raises(ValueError):
        BatchedStreamBeamDecoder(m, flags, S, W=W, prefix=True, dither=0)
    with pytest.raises(ValueError):
        decode.StreamingBeamSearch(m, S, W=W, prefix=True)


def test_e6d2_bf16_many_streams(hip_lib):
    from edgedict_amd import decode
    from edgedict_amd.flags import make_flags, model_kwargs
    from edgedict_amd.models import Transducer
    flags = make_flags("E6D2")
    torch.manual_seed(0)
    m = Transducer(**model_kwargs(flags, vocab_size=2048)).cuda().eval()
    m.compute_dtype = "bf16"
    with torch.no_grad():
        m.joint.joint[2].bias[0] += 12.0
    S, W = 64, 10
    P = m.joint.joint[0].weight.shape[1] - m.decoder.proj.weight.shape[0]
    g = torch.Generator().manual_seed(2)
    sb = decode.StreamingBeamSearch(m, S, W=W)
    picks = [0, 37, 63]
    singles = {s: decode.StreamingBeamSearch(m, 1, W=W) for s in picks}
    with torch.no_grad():
        for k in range(4):
            enc = torch.randn(S, 2, P, generator=g).cuda().to(torch.bfloat16)
            E1 = sb.joint_rows(enc)
            sb.advance_rows(E1, P)
            rows = E1.reshape(S, 2, -1)
            for s in picks:
                singles[s].advance_rows(rows[s].contiguous(), P)
    got, gsc = sb.best()
    assert torch.isfinite(gsc).all() and (gsc >= 0).all()
    for s in picks:
        one, osc = singles[s].best()
        assert np.array_equal(got[s], one[0]), s
        np.testing.assert_allclose(gsc[s].item(), osc[0].item(), rtol=1e-6)
