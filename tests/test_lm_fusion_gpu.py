"""GPU: LM shallow fusion in the batched and streaming beam searches (csrc/decode.hip beam_expand_lm, the LM step of
decode_fused.hip / the composed kernels) and edgedict_amd.lm.LMModel.

The oracle is an fp64 restatement of the fused search, written below as a copy of oracle/beam_ref.beam_search_one's
loop with an LM state per hypothesis: the LM is the reference's LMModel (/root/reference/models.py:224-261) restated
with torch.nn.Embedding / nn.LSTM / nn.Linear on the CPU from the same state dict, and a non-blank child k scores
``logp(y*) + lp_rnnt[k] + (lm_weight * lp_lm[k] + length_bonus)`` (Python floats: fp64 sums of fp32 log-probs)."""
import os

import numpy as np
import pytest
import torch

from oracle import models_ref as M

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(os.path.dirname(__file__), "golden", "beam_tiny.npz"))
CFG = dict(vocab_embed_size=16, vocab_size=40, input_size=24, enc_hidden_size=32, enc_layers=2,
           enc_proj_size=24, dec_hidden_size=32, dec_layers=2, dec_proj_size=24, joint_size=32)
# every prediction-network, joint and LM width a multiple of 32: the fused step kernels run
CFG32 = dict(vocab_embed_size=32, vocab_size=64, input_size=24, enc_hidden_size=32, enc_layers=2,
             enc_proj_size=32, dec_hidden_size=64, dec_layers=2, dec_proj_size=32, joint_size=64)


def _engine(sd, dtype="fp32", cfg=CFG):
    from edgedict_amd.models import Transducer
    m = Transducer(enc_dropout=0.0, dec_dropout=0.0, output_loss=False, **cfg)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    m.compute_dtype = dtype
    return m


def _golden_sd():
    return {k[3:]: torch.from_numpy(G[k]) for k in G.files if k.startswith("sd/")}


def _lm_sd(ntoken, ninp, nhid, nlayers, seed, scale=1.0):
    """A reference-keyed LMModel state dict (the keys torch.save(model.state_dict()) writes in cli/train_lm.py:109)."""
    torch.manual_seed(seed)
    emb = torch.nn.Embedding(ntoken, ninp)
    rnn = torch.nn.LSTM(ninp, nhid, nlayers, batch_first=True)
    dec = torch.nn.Linear(nhid, ntoken)
    sd = {"encoder.weight": emb.weight.detach().clone() * 0.5}
    sd.update({"rnn." + k: v.detach().clone() for k, v in rnn.state_dict().items()})
    sd["decoder.weight"] = dec.weight.detach().clone() * scale
    sd["decoder.bias"] = dec.bias.detach().clone() * scale
    return sd


def _lm(sd, dtype="fp32"):
    from edgedict_amd.lm import LMModel
    ntoken, ninp = sd["encoder.weight"].shape
    nhid = sd["rnn.weight_hh_l0"].shape[1]
    nl = sum(1 for k in sd if k.startswith("rnn.weight_hh_l"))
    lm = LMModel(ntoken, ninp, nhid, nl, dropout=0.0)
    lm.load_state_dict(sd, strict=True)
    lm = lm.cuda().eval()
    lm.compute_dtype = dtype
    for p in lm.parameters():
        p.requires_grad_(False)
    return lm


class RefLM:
    """LMModel (models.py:224-261) restated with torch.nn modules on the CPU (fp32), one step at a time."""

    def __init__(self, sd):
        ntoken, ninp = sd["encoder.weight"].shape
        nhid = sd["rnn.weight_hh_l0"].shape[1]
        self.L = sum(1 for k in sd if k.startswith("rnn.weight_hh_l"))
        self.H = nhid
        self.emb = torch.nn.Embedding(ntoken, ninp)
        self.rnn = torch.nn.LSTM(ninp, nhid, self.L, batch_first=True)
        self.dec = torch.nn.Linear(nhid, ntoken)
        self.emb.load_state_dict({"weight": sd["encoder.weight"]})
        self.rnn.load_state_dict({k[4:]: v for k, v in sd.items() if k.startswith("rnn.")})
        self.dec.load_state_dict({"weight": sd["decoder.weight"], "bias": sd["decoder.bias"]})

    def zero(self, B=1):
        return (torch.zeros(self.L, B, self.H), torch.zeros(self.L, B, self.H))

    @torch.no_grad()
    def forward(self, tokens, hidden):
        out, hidden = self.rnn(self.emb(tokens), hidden)
        return torch.log_softmax(self.dec(out).reshape(-1, self.dec.out_features), dim=-1), hidden


class _Hyp:
    __slots__ = ("k", "tok", "h", "logp", "lm_tok", "lm_h")

    def __init__(self, k, tok, h, logp, lm_tok, lm_h):
        self.k, self.tok, self.h, self.logp, self.lm_tok, self.lm_h = k, tok, h, logp, lm_tok, lm_h


def fused_beam_one(sd, ref_lm, h_enc, W, lm_weight, length_bonus, lm_bos=1, blank=M.NUL):
    """oracle/beam_ref.beam_search_one (prefix=False) with an LM state per hypothesis and the fused score."""
    L = M.n_dec_layers(sd)
    H = sd["decoder.lstm.weight_hh_l0"].shape[1]
    zero = (torch.zeros(L, 1, H), torch.zeros(L, 1, H))
    V = sd["joint.joint.2.weight"].shape[0]
    B = [_Hyp([], M.BOS, zero, 0.0, lm_bos, ref_lm.zero())]
    n_expansions = 0
    for x in h_enc:
        A = B
        B = []
        while True:
            y_hat = max(A, key=lambda a: a.logp)
            A.remove(y_hat)
            pred, hidden = M.decoder_forward(sd, torch.tensor([[y_hat.tok]]), y_hat.h)
            logp = torch.log_softmax(M.joint_forward(sd, x[None, :], pred[:, 0])[0], dim=0)
            lp_lm, lm_hidden = ref_lm.forward(torch.tensor([[y_hat.lm_tok]]), y_hat.lm_h)
            lp_lm = lp_lm[0]
            n_expansions += 1
            for k in range(V):
                if k == blank:
                    B.append(_Hyp(y_hat.k, y_hat.tok, y_hat.h, y_hat.logp + float(logp[k]), y_hat.lm_tok, y_hat.lm_h))
                else:
                    lp = y_hat.logp + float(logp[k]) + (lm_weight * float(lp_lm[k]) + length_bonus)
                    A.append(_Hyp(y_hat.k + [k], k, hidden, lp, k, lm_hidden))
            y_a = max(A, key=lambda a: a.logp)
            y_b = max(B, key=lambda a: a.logp)
            if len(B) >= W and y_b.logp >= y_a.logp:
                break
        B = B[:W]
    return list(B[0].k), -B[0].logp, n_expansions


def fused_beam(sd, lm_sd, xs, xlen, W, lm_weight, length_bonus, lm_bos=1):
    h_enc, _ = M.encoder_forward(sd, xs, None)
    Bn, T = h_enc.shape[0], h_enc.shape[1]
    lens = [T] * Bn if xlen is None else [int(v) for v in M.scale_length(T, xlen)]
    ref_lm = RefLM(lm_sd)
    seqs, scores, total = [], [], 0
    for b in range(Bn):
        k, s, n = fused_beam_one(sd, ref_lm, h_enc[b, :lens[b]], W, lm_weight, length_bonus, lm_bos)
        seqs.append(np.array(k, dtype=np.int64))
        scores.append(s)
        total += n
    return seqs, np.array(scores, dtype=np.float64), total


def _same(a_seqs, a_sc, b_seqs, b_sc):
    assert len(a_seqs) == len(b_seqs)
    for x, y in zip(a_seqs, b_seqs):
        assert x.dtype == np.int64 and np.array_equal(x, y), (x, y)
    assert a_sc.dtype == torch.float64
    assert np.array_equal(a_sc.numpy(), b_sc.numpy()), (a_sc, b_sc)


# ---------------------------------------------------------------------------------------------------- 1. LMModel
@pytest.mark.parametrize("dtype,tol", [("fp32", 1e-5), ("bf16", 2e-2)])
def test_lm_forward_matches_the_torch_restatement(hip_lib, dtype, tol):
    sd = _lm_sd(48, 32, 64, 2, seed=3)
    lm = _lm(sd, dtype)
    ref = RefLM(sd)
    g = torch.Generator().manual_seed(0)
    toks = torch.randint(0, 48, (3, 7), generator=g)
    h0 = (0.3 * torch.randn(2, 3, 64, generator=g), 0.3 * torch.randn(2, 3, 64, generator=g))
    with torch.no_grad():
        out, (h, c) = lm(toks.cuda(), (h0[0].cuda(), h0[1].cuda()))
        zout, _ = lm(toks.cuda(), lm.init_hidden(3))
    want, (wh, wc) = ref.forward(toks, h0)
    zwant, _ = ref.forward(toks, ref.zero(3))
    assert out.dtype == torch.float32 and out.shape == (21, 48)
    np.testing.assert_allclose(out.cpu().numpy(), want.numpy(), atol=tol, rtol=0)
    np.testing.assert_allclose(zout.cpu().numpy(), zwant.numpy(), atol=tol, rtol=0)
    np.testing.assert_allclose(h.cpu().numpy(), wh.numpy(), atol=tol, rtol=0)
    np.testing.assert_allclose(c.cpu().numpy(), wc.numpy(), atol=tol, rtol=0)


def test_lm_tied_weights_forward(hip_lib):
    from edgedict_amd.lm import LMModel
    lm = LMModel(40, 32, 32, 1, dropout=0.0, tie_weights=True).cuda().eval()
    assert lm.decoder.weight is lm.encoder.weight
    sd = {k: v.detach().cpu() for k, v in lm.state_dict().items()}
    toks = torch.randint(0, 40, (2, 5))
    with torch.no_grad():
        out, _ = lm(toks.cuda(), lm.init_hidden(2))
    want, _ = RefLM(sd).forward(toks, RefLM(sd).zero(2))
    np.testing.assert_allclose(out.cpu().numpy(), want.numpy(), atol=1e-5, rtol=0)


def test_log_softmax_rows_kernel(hip_lib):
    from edgedict_amd.lm import log_softmax_rows
    x = 4 * torch.randn(5, 1000, generator=torch.Generator().manual_seed(1))
    y = log_softmax_rows(x.cuda())
    np.testing.assert_allclose(y.cpu().numpy(), torch.log_softmax(x, -1).numpy(), atol=1e-5, rtol=0)
    yb = log_softmax_rows(x.cuda().to(torch.bfloat16))
    np.testing.assert_allclose(yb.cpu().numpy(), torch.log_softmax(x.to(torch.bfloat16).float(), -1).numpy(),
                               atol=1e-5, rtol=0)


# ---------------------------------------------------------------------------------------------------- 2. weight 0
def _ragged_random():
    sd = M.make_state_dict(CFG, 3)
    xs, _, _, _ = M.make_batch(CFG, 4, 5, 17, 4)
    xlen = torch.tensor([17, 9, 17, 3, 12], dtype=torch.int32)
    return sd, xs, xlen


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("W", [1, 4, 10])
@pytest.mark.parametrize("model", ["trained", "random"])
def test_zero_weight_is_bit_equal_to_the_plain_search(hip_lib, dtype, W, model):
    from edgedict_amd import decode
    if model == "trained":
        sd, xs, xlen = _golden_sd(), torch.from_numpy(G["xs"]), torch.from_numpy(G["xlen"])
    else:
        sd, xs, xlen = _ragged_random()
    m = _engine(sd, dtype)
    lm = _lm(_lm_sd(40, 16, 32, 2, seed=W), dtype)
    with torch.no_grad():
        s0, c0 = m.beam_search(xs.cuda(), xlen, W=W, max_expansions=400)
        e0 = decode.beam_search_batch.last_expansions
        s1, c1 = m.beam_search(xs.cuda(), xlen, W=W, max_expansions=400, lm=lm, lm_weight=0.0, length_bonus=0.0)
        e1 = decode.beam_search_batch.last_expansions
    _same(s1, c1, s0, c0)
    assert e1 == e0


# ---------------------------------------------------------------------------------------------------- 3. oracle
@pytest.mark.parametrize("path", ["composed", "fused"])
@pytest.mark.parametrize("lm_weight,length_bonus", [(0.5, 0.0), (0.3, 0.4), (0.8, -0.2)])
def test_fused_search_matches_the_restatement(hip_lib, path, lm_weight, length_bonus):
    from edgedict_amd import decode
    if path == "composed":
        cfg, lm_dims = CFG, (40, 16, 32, 2)
    else:
        cfg, lm_dims = CFG32, (64, 32, 64, 2)
    sd = M.make_state_dict(cfg, 7)
    sd["joint.joint.2.bias"][0] -= 2.0         # blank disfavoured: hundreds of pops per utterance
    xs, _, _, _ = M.make_batch(cfg, 4, 4, 13, 4)
    xlen = torch.tensor([13, 8, 13, 5], dtype=torch.int32)
    lm_sd = _lm_sd(*lm_dims, seed=11, scale=3.0)
    m = _engine(sd, "fp32", cfg)
    lm = _lm(lm_sd)
    W = 4
    with torch.no_grad():
        seqs, scores = m.beam_search(xs.cuda(), xlen, W=W, max_expansions=400, lm=lm, lm_weight=lm_weight,
                                     length_bonus=length_bonus)
    nexp = decode.beam_search_batch.last_expansions
    rs, rsc, rexp = fused_beam(sd, lm_sd, xs, xlen, W, lm_weight, length_bonus)
    for a, b in zip(seqs, rs):
        assert np.array_equal(a, b), (a, b)
    np.testing.assert_allclose(scores.numpy(), rsc, rtol=2e-4, atol=2e-4)
    assert nexp == rexp


# ---------------------------------------------------------------------------------------------------- 4. LM matters
def test_a_strong_lm_changes_the_output(hip_lib):
    """An LM whose output bias strongly favours one token the plain search never emits: at a large weight the fused
    search emits it (every other token costs about lm_weight x 8), and the restatement agrees."""
    sd = _golden_sd()
    xs, xlen = torch.from_numpy(G["xs"]), torch.from_numpy(G["xlen"])
    m = _engine(sd)
    W = 4
    with torch.no_grad():
        plain, _ = m.beam_search(xs.cuda(), xlen, W=W)
    emitted = set(np.concatenate(plain).tolist())
    assert emitted
    found = None
    for fav in [k for k in range(4, 40) if k not in emitted][:8]:
        lm_sd = _lm_sd(40, 16, 32, 2, seed=5)
        lm_sd["decoder.bias"][fav] += 8.0
        with torch.no_grad():
            fused, fsc = m.beam_search(xs.cuda(), xlen, W=W, max_expansions=400, lm=_lm(lm_sd), lm_weight=1.5)
        if any(fav in s for s in fused):
            found = (fav, lm_sd, fused, fsc)
            break
    assert found is not None, "no favoured token reached the output"
    fav, lm_sd, fused, fsc = found
    rs, rsc, _ = fused_beam(sd, lm_sd, xs, xlen, W, 1.5, 0.0)
    for a, b in zip(fused, rs):
        assert np.array_equal(a, b)
    np.testing.assert_allclose(fsc.numpy(), rsc, rtol=2e-4, atol=2e-4)


def test_lm_bos_is_the_lm_root_token(hip_lib):
    """lm_bos is what the LM reads first: another start token changes the scores as the restatement says."""
    sd = _golden_sd()
    xs, xlen = torch.from_numpy(G["xs"])[:2], torch.from_numpy(G["xlen"])[:2]
    lm_sd = _lm_sd(40, 16, 32, 2, seed=9, scale=3.0)
    m = _engine(sd)
    lm = _lm(lm_sd)
    with torch.no_grad():
        a, asc = m.beam_search(xs.cuda(), xlen, W=2, max_expansions=400, lm=lm, lm_weight=0.5)
        b, bsc = m.beam_search(xs.cuda(), xlen, W=2, max_expansions=400, lm=lm, lm_weight=0.5, lm_bos=7)
    assert not np.array_equal(asc.numpy(), bsc.numpy())
    rs, rsc, _ = fused_beam(sd, lm_sd, xs, xlen, 2, 0.5, 0.0, lm_bos=7)
    for x, y in zip(b, rs):
        assert np.array_equal(x, y)
    np.testing.assert_allclose(bsc.numpy(), rsc, rtol=2e-4, atol=2e-4)


# ---------------------------------------------------------------------------------------------------- 5. streaming
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


def _offline(m, rows, P, W, EM, **kw):
    from edgedict_amd import decode
    S = rows[0].shape[0]
    E1 = torch.cat(rows, dim=1).reshape(-1, rows[0].shape[2]).contiguous()
    seqs, sc = decode.beam_search_rows(m, E1, S, E1.shape[0] // S, P, None, W=W, max_expansions=EM, **kw)
    return seqs, sc, decode.beam_search_batch.last_expansions


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("path", ["composed", "fused"])
def test_streaming_with_lm_equals_the_offline_fused_search(hip_lib, dtype, path):
    from edgedict_amd import decode
    sd = _golden_sd()
    m = _engine(sd, dtype)
    lm_dims = (40, 16, 32, 2) if path == "composed" else (40, 32, 64, 2)
    lm = _lm(_lm_sd(*lm_dims, seed=2, scale=3.0), dtype)
    fuse = dict(lm=lm, lm_weight=0.4, length_bonus=0.3)
    with torch.no_grad():
        enc, _ = m.encoder(torch.from_numpy(G["xs"]).cuda())
    enc = enc.contiguous()
    S, T, P = enc.shape
    W, EM = 4, 400
    for kind in (1, 3, 7, "ragged"):
        sb = decode.StreamingBeamSearch(m, S, W=W, max_expansions=EM, **fuse)
        rows, t = [], 0
        for n in _splits(T, kind, seed=W):
            chunk = enc[:, t:t + n].contiguous()
            rows.append(sb.joint_rows(chunk).reshape(S, n, -1))
            sb.advance(chunk)
            t += n
            got, gsc = sb.best()
            want, wsc, wexp = _offline(m, rows, P, W, EM, **fuse)
            _same(got, gsc, want, wsc)
            assert int(sb.expansions().sum()) == wexp
            for c, g in zip(sb.committed(), got):
                assert np.array_equal(c, g[:len(c)])


def test_streaming_with_lm_masked_reset_equals_independent_streams(hip_lib):
    from edgedict_amd import decode
    m = _engine(_golden_sd())
    lm = _lm(_lm_sd(40, 16, 32, 2, seed=4, scale=3.0))
    fuse = dict(lm=lm, lm_weight=0.5, length_bonus=0.2)
    with torch.no_grad():
        full, _ = m.encoder(torch.from_numpy(G["xs"]).cuda())
    Tf = full.shape[1]
    S, W, EM = 5, 4, 400
    P = CFG["enc_proj_size"]
    frames = [[2, 0, 3, 1, 3], [1, 3, 0, 3, 2], [3, 3, 3, 0, 1], [0, 2, 1, 3, 3], [2, 1, 3, 2, 0], [3, 0, 2, 1, 3]]
    sb = decode.StreamingBeamSearch(m, S, W=W, max_expansions=EM, **fuse)
    singles = [decode.StreamingBeamSearch(m, 1, W=W, max_expansions=EM, **fuse) for _ in range(S)]
    for k, nf in enumerate(frames):
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
            assert gsc[s].item() == osc[0].item(), (k, s)
            assert np.array_equal(sb.committed()[s], singles[s].committed()[0])
    assert int(sb.expansions()[1]) == int(singles[1].expansions()[0])
    assert any(len(x) for x in got)


def test_long_stream_with_lm_bounded_tree_equals_the_offline_search(hip_lib):
    """2000+ frames through a small node_capacity: the tree is compacted many times, so most pops of the root feed the
    last COMMITTED token to the LM (not lm_bos); the end result still equals the offline fused search."""
    from edgedict_amd import decode
    sd = _golden_sd()
    m = _engine(sd)
    lm = _lm(_lm_sd(40, 16, 32, 2, seed=6, scale=3.0))
    fuse = dict(lm=lm, lm_weight=0.3, length_bonus=0.1)
    xs = torch.from_numpy(G["xs"])
    xlen = G["xlen"]
    utt = torch.cat([xs[b, :int(xlen[b])] for b in range(xs.shape[0])], 0)
    reps = 4000 // utt.shape[0] + 2
    with torch.no_grad():
        enc, _ = m.encoder(utt.repeat(reps, 1)[None].cuda())
    enc = enc.contiguous()
    T, P = enc.shape[1], enc.shape[2]
    assert T >= 2000
    W, EM, NC = 4, 32, 1024
    assert NC * 4 < T * EM
    sb = decode.StreamingBeamSearch(m, 1, W=W, max_expansions=EM, node_capacity=NC, **fuse)
    rows = []
    step = 10
    for t in range(0, T, step):
        chunk = enc[:, t:t + step].contiguous()
        rows.append(sb.joint_rows(chunk).reshape(1, chunk.shape[1], -1))
        sb.advance(chunk)
    got, gsc = sb.best()
    want, wsc, wexp = _offline(m, rows, P, W, EM, **fuse)
    _same(got, gsc, want, wsc)
    assert int(sb.expansions()[0]) == wexp
    assert len(sb.committed()[0]) > 0


# ---------------------------------------------------------------------------------------------------- 6. audio level
STREAM_CFG = dict(vocab_embed_size=16, vocab_size=64, input_size=240, enc_hidden_size=64, enc_layers=3,
                  enc_proj_size=48, dec_hidden_size=32, dec_layers=2, dec_proj_size=32, joint_size=64)


def test_audio_level_decoder_with_lm_equals_the_offline_fused_search(hip_lib):
    from edgedict_amd import decode
    from edgedict_amd.flags import make_flags
    from edgedict_amd.stream import BatchedStreamBeamDecoder, chunk_geometry
    flags = make_flags("E6D2")
    sd = M.make_state_dict(STREAM_CFG, 5)
    sd["joint.joint.2.bias"][0] += 1.0
    m = _engine(sd, "fp32", STREAM_CFG)
    lm = _lm(_lm_sd(64, 32, 64, 2, seed=8, scale=3.0))
    fuse = dict(lm=lm, lm_weight=0.5, length_bonus=0.2)
    S, W = 3, 4
    win, hop = chunk_geometry(flags, 2)
    g = torch.Generator().manual_seed(0)
    wave = (0.1 * torch.randn(S, win + 5 * hop, generator=g)).cuda()
    dec = BatchedStreamBeamDecoder(m, flags, S, W=W, dither=0, max_expansions=400, **fuse)
    L, H = len(m.encoder.lstm.lstms), m.encoder.lstm.hidden_size
    h = torch.zeros(L, S, H, device="cuda")
    c = torch.zeros(L, S, H, device="cuda")
    rows = []
    with torch.no_grad():
        for k in range(6):
            chunk = wave[:, k * hop:k * hop + win].contiguous()
            got, gsc = dec.decode(chunk.clone())
            xs, _ = dec.transform(chunk.clone())
            enc, (h, c) = m.encoder(xs, (h, c))
            enc = enc.contiguous()
            rows.append(decode.joint_rows(m, enc).reshape(S, enc.shape[1], -1))
            want, wsc, _ = _offline(m, rows, enc.shape[2], W, 400, **fuse)
            _same(got, gsc, want, wsc)


@pytest.mark.parametrize("streaming", [False, True])
def test_expansion_cap_with_lm_is_an_error(hip_lib, streaming):
    """A large length bonus keeps popping: hitting max_expansions raises, it never truncates."""
    from edgedict_amd import decode
    sd = _golden_sd()
    m = _engine(sd)
    lm = _lm(_lm_sd(40, 16, 32, 2, seed=1))
    xs, xlen = torch.from_numpy(G["xs"]).cuda(), torch.from_numpy(G["xlen"])
    fuse = dict(lm=lm, lm_weight=0.1, length_bonus=50.0)
    with torch.no_grad():
        m.beam_search(xs, xlen, W=2, max_expansions=16)           # the plain search fits
        if streaming:
            enc, _ = m.encoder(xs)
            sb = decode.StreamingBeamSearch(m, enc.shape[0], W=2, max_expansions=16, **fuse)
            with pytest.raises(RuntimeError, match="max_expansions"):
                sb.advance(enc.contiguous())
        else:
            with pytest.raises(RuntimeError, match="max_expansions"):
                m.beam_search(xs, xlen, W=2, max_expansions=16, **fuse)
