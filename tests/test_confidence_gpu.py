"""GPU: the confidence pass (csrc/confidence.hip conf_row_stats / conf_hidden_rows; loss.row_confidence,
decode.hypothesis_confidence / ctc_hypothesis_confidence, Transducer.confidence) against the fp64 oracle
tests/confidence_ref.py (pinned by tests/test_confidence_host.py), against the searches' own ``token_logp``, and
against itself (a second run, a chunked run: the same bits).

Bounds, none taken from the device: the row kernel's log-prob columns rtol = atol = 1e-5 (the project's figure for the
form (z - m) - log s, tests/test_ilme_gpu.py), its H and log sum p^alpha 4 x the fp32 numpy restatement's error on the
same inputs with a floor of 1e-5 (the host test finds the floor everywhere); the hidden kernel in fp32
2^-24 (2 S + 2), S = |e| + |d| + |b1| (two additions rounded at a sum of at most S, passed on by tanh's slope <= 1, and
tanhf within 2 ulp of a value below 1), in bf16 one bf16 ulp of the rounded fp64 value; end to end 3 x ERR of
confidence_ref (fp32: ``logp`` at the suite's TOL instead), the arg max exact where the oracle's top-two gap allows.
The end-to-end reference is the fp64 replay FROM THE ENCODER OUTPUT THE PASS WAS GIVEN (read from the device) with the
weights as the kernels get them, on the oracle's lists (sync_beam_ref.search, W = 4, blank_bias 1.0: 44 / 55 / 57 token
rows, no near-tie), wrapped as NBestResult: no search decision is involved."""
import numpy as np
import pytest
import torch

import confidence_ref as C
import sync_beam_ref as S
from oracle import models_ref as M
from test_sync_beam_gpu import CFG, CFGS, TOL, _engine, _inputs

pytestmark = pytest.mark.gpu
DT = {"fp32": torch.float32, "bf16": torch.bfloat16}


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def _check_rows(got, top, exact, etop, gap, bound, what):
    got, top = got.double().cpu().numpy(), top.cpu().numpy()
    with np.errstate(invalid="ignore"):
        d = np.abs(got - exact)
    print(what, "largest differences per column:", np.nanmax(np.where(np.isnan(d), 0, d), axis=0), "bounds", bound)
    assert np.array_equal(np.isnan(got), np.isnan(exact)), what
    assert np.array_equal(np.isneginf(got), np.isneginf(exact)), what
    fin = np.isfinite(exact)
    for c in range(3):
        np.testing.assert_allclose(got[fin[:, c], c], exact[fin[:, c], c], rtol=bound[c], atol=bound[c], err_msg=what)
    for c in (3, 4):
        assert (d[fin[:, c], c] <= bound[c]).all(), (what, c, d[:, c].max(), bound[c])
    keep = gap >= C.MIN_MARGIN
    assert keep.sum() >= 0.9 * len(gap), what                     # the oracle alone excludes at most 10 % of the rows
    assert np.array_equal(top[keep], etop[keep]), (what, top, etop)


# ------------------------------------------------------------------------------------------- 1. the row kernel
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("V", C.KERNEL_V)
def test_row_kernel_matches_fp64_on_the_same_logits(hip_lib, V, dtype):
    from edgedict_amd.loss import row_confidence
    td = DT[dtype]
    for Rn in C.KERNEL_R:
        z, tok = C.kernel_rows(V, Rn, dtype == "bf16")
        exact, etop, gap, bound = C.kernel_bounds(z, tok)
        zd, td_tok = _dev(z, td), _dev(tok)
        stats, top = row_confidence(zd, td_tok)
        assert stats.dtype == torch.float32 and tuple(stats.shape) == (Rn, 5) and top.dtype == torch.int32
        _check_rows(stats, top, exact, etop, gap, bound, "V=%d R=%d %s" % (V, Rn, dtype))
        again = row_confidence(zd, td_tok)
        assert torch.equal(stats.view(torch.int32), again[0].view(torch.int32)) and torch.equal(top, again[1])
        # a gather index with repeats, in reversed order, into a wider NaN-filled buffer: an odd pitch (element loads)
        # and a 16-byte pitch (vector loads; for V % 8 != 0 the last access straddles V and must not read the NaN).
        # Another layout is another summation order: each is held to the oracle, and to itself bit by bit
        idx = np.concatenate([np.arange(Rn)[::-1], [0, Rn - 1]]).astype(np.int32)
        pick = torch.from_numpy(idx).long().cuda()
        for ld in (V + 5, (V + 7) // 8 * 8 + 8):
            buf = torch.full((Rn + 2, ld), float("nan"), dtype=td, device="cuda")
            buf[1:Rn + 1, :V] = zd
            s3, t3 = row_confidence(buf[1:, :V], td_tok, ld=ld)               # no index: row r, the pitch given
            _check_rows(s3, t3, exact, etop, gap, bound, "V=%d R=%d %s ld=%d" % (V, Rn, dtype, ld))
            s2, t2 = row_confidence(buf[:, :V], td_tok[pick], rows=_dev(idx + 1))
            assert torch.equal(s2.view(torch.int32), s3[pick].view(torch.int32)), (V, Rn, ld)
            assert torch.equal(t2, t3[pick])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("V", [65, 2112])
def test_row_kernel_dead_rows_stray_tokens_and_stray_indices(hip_lib, V, dtype):
    """An all -inf row and a row holding a NaN between normal rows, tokens -1 and V, and gather indices -1 and N: NaN
    where the contract says so, the neighbours' bits untouched, nothing read for a stray index."""
    from edgedict_amd.loss import row_confidence
    td = DT[dtype]
    z, tok = C.kernel_rows(V, 5, dtype == "bf16")
    z, tok = z.copy(), tok.copy()
    base, btop = row_confidence(_dev(z, td), _dev(tok))
    z[1] = -np.inf
    z[3, V - 1] = np.nan
    tok[0], tok[2] = -1, V
    exact, etop, gap, bound = C.kernel_bounds(z, tok)
    stats, top = row_confidence(_dev(z, td), _dev(tok))
    _check_rows(stats, top, exact, etop, np.where(np.isnan(gap), 1.0, gap), bound, "special V=%d %s" % (V, dtype))
    s, b = stats.cpu().numpy(), base.cpu().numpy()
    assert np.isnan(s[1]).all() and np.isnan(s[3]).all() and top.cpu().tolist()[1] == -1 and top.cpu().tolist()[3] == -1
    assert np.isnan(s[0, 0]) and np.isnan(s[2, 0])
    assert np.array_equal(s[[0, 2], 1:].view(np.int32), b[[0, 2], 1:].view(np.int32))         # the rest of those rows
    assert np.array_equal(s[4].view(np.int32), b[4].view(np.int32)) and top[4].item() == btop[4].item()
    idx = np.array([4, -1, 0, 5, 2], dtype=np.int32)
    s2, t2 = row_confidence(_dev(z, td), _dev(tok[[4, 4, 4, 4, 4]]), rows=_dev(idx))
    s2 = s2.cpu().numpy()
    assert np.isnan(s2[1]).all() and np.isnan(s2[3]).all() and t2.cpu().tolist()[1] == -1 and t2.cpu().tolist()[3] == -1
    assert np.array_equal(s2[0].view(np.int32), s[4].view(np.int32)) and np.isfinite(s2[[2, 4]]).all()
    with pytest.raises(ValueError, match="alpha"):
        row_confidence(_dev(z, td), _dev(tok), alpha=1.0)
    with pytest.raises(ValueError, match="tokens for"):
        row_confidence(_dev(z, td), _dev(np.zeros(6, dtype=np.int32)))


# ------------------------------------------------------------------------------------------- 2. the hidden kernel
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("J", [20, 24, 32, 64])
def test_hidden_kernel_gathers_adds_and_rounds_once(hip_lib, J, dtype):
    """J = 20: element loads in bf16 (20 % 8 != 0) and, with the operands 4 bytes off a 16-byte boundary, in fp32; 24:
    16-byte accesses in fp32 (6 per row) and bf16 (3 per row); repeated indices; one index out of range on either side
    gives a NaN row, the others' bits as without it."""
    from edgedict_amd.decode import confidence_hidden_rows
    td = DT[dtype]
    g = torch.Generator().manual_seed(J)
    E1 = (torch.randn(7, J, generator=g) * 1.5).to(td)
    D1 = torch.randn(4, J, generator=g).to(td)
    b1 = torch.randn(J, generator=g) * 0.5

    def up(t):
        """on the device; for J = 20 one element behind a 16-byte boundary"""
        if J != 20:
            return t.cuda()
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
        buf[1:] = t.reshape(-1).cuda()
        return buf[1:].view(t.shape)

    dE1, dD1 = up(E1), up(D1)
    assert dE1.is_contiguous() and (dE1.data_ptr() % 16 == 0) == (J != 20)
    for Rn in (1, 5):
        er = np.array([6, 2, 2, 0, 5][:Rn], dtype=np.int32)
        dr = np.array([3, 1, 1, 0, 3][:Rn], dtype=np.int32)
        for bias in (None, b1):
            hid = confidence_hidden_rows(dE1, dD1, _dev(er), _dev(dr), None if bias is None else bias.cuda())
            assert hid.dtype == td and tuple(hid.shape) == (Rn, J)
            e, d = E1.double()[er.astype(np.int64)], D1.double()[dr.astype(np.int64)]
            x = e + d + (0 if bias is None else bias.double())
            want = torch.tanh(x)
            if dtype == "fp32":
                bound = 2.0 ** -24 * (2 * (e.abs() + d.abs() + (0 if bias is None else bias.double().abs())) + 2)
                diff = (hid.double().cpu() - want).abs()
                print("J=%d R=%d largest difference / bound: %.3g" % (J, Rn, float((diff / bound).max())))
                assert (diff <= bound).all()
            else:
                got, ref = hid.cpu().view(torch.int16).int(), want.to(td).view(torch.int16).int()
                print("J=%d R=%d bf16 ulps apart: %d" % (J, Rn, int((got - ref).abs().max())))
                assert ((got - ref).abs() <= 1).all()
            for bad_e, bad_d in ((7, 0), (-1, 0), (0, 4), (0, -1)):
                er2, dr2 = er.copy(), dr.copy()
                er2[Rn // 2], dr2[Rn // 2] = bad_e, bad_d
                h2 = confidence_hidden_rows(dE1, dD1, _dev(er2), _dev(dr2),
                                            None if bias is None else bias.cuda())
                assert torch.isnan(h2[Rn // 2].float()).all()
                live = [r for r in range(Rn) if r != Rn // 2]
                assert torch.equal(h2[live].view(torch.int16), hid[live].view(torch.int16))


# ------------------------------------------------------------------------------------------- 3. end to end
def _encoded(m, xs, xlen):
    with torch.no_grad():
        enc, _ = m.encoder(xs.cuda())
    enc = enc.contiguous()
    return enc, m.scale_length(enc, xlen).numpy().astype(np.int32)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["CFG", "CFG32", "CFGV"])
def test_pass_matches_the_fp64_replay_on_the_oracles_lists(hip_lib, name, dtype):
    """Largest |device - fp64 replay| / (3 x ERR) measured on the MI355X, columns logp, logp_max, logp_blank, H,
    log sum p^alpha (fp32: ``logp`` against TOL = 2e-4 instead): see the figures in DESIGN.md section 4.57."""
    from edgedict_amd import decode
    cfg = CFGS[name][0]
    V = cfg["vocab_size"]
    fused = hip_lib.edgedict_decode_fused_ok(0 if dtype == "fp32" else 1, 0, cfg["joint_size"], V,
                                             cfg["vocab_embed_size"], cfg["dec_hidden_size"], cfg["dec_proj_size"])
    assert fused == (0 if name == "CFG" else 1)               # the searches' composed route and their fused one
    sd, xs, xlen, _, lens, _ = C.oracle_lists(name)
    w = C.wrapped(name)
    m = _engine(sd, cfg, dtype)
    enc, dlens = _encoded(m, xs, xlen)
    assert enc.dtype == DT[dtype] and dlens.tolist() == list(lens)
    table = decode.WordTable(np.arange(V) % 3 == 0)
    got = decode.hypothesis_confidence(m, enc, dlens, w.results, words=table)
    exact = C.replay_stats(C.rounded_sd(sd, DT[dtype]), enc.cpu(), w.lists)
    err = C.err(name, dtype)
    bound = 3.0 * err
    worst, rows = np.zeros(5), 0
    assert len(got) == len(w.results)
    for b, (c, r, ex) in enumerate(zip(got, w.results, exact)):
        assert len(c) == len(r) and c.utterance.shape == (len(r),)
        for i, (stats, etop, gap) in enumerate(ex):
            n = len(r.tokens[i])
            assert c.raw[i].shape == (n, 5) and c.raw[i].dtype == np.float64 and c.top[i].dtype == np.int32
            assert c.token[i].shape == (n,) and c.top[i].shape == (n,)
            if n == 0:
                assert np.isnan(c.utterance[i]) and c.word[i] == []
                continue
            d = np.abs(c.raw[i] - stats)
            worst, rows = np.maximum(worst, d.max(axis=0)), rows + n
            if dtype == "fp32":
                np.testing.assert_allclose(c.raw[i][:, 0], stats[:, 0], **TOL)
                assert (d[:, 1:] <= bound[1:]).all(), (name, dtype, b, i, d.max(axis=0), bound)
            else:
                assert (d <= bound).all(), (name, dtype, b, i, d.max(axis=0), bound)
            keep = gap >= (C.MIN_MARGIN if dtype == "fp32" else max(C.MIN_MARGIN, 6.0 * err[1]))
            assert np.array_equal(c.top[i][keep], etop[keep])
            # the host side of the pass: measures, aggregates, words
            assert np.array_equal(c.token[i], decode.confidence_measure(c.raw[i], V, "tsallis", 1.0 / 3.0))
            assert ((c.token[i] >= 0) & (c.token[i] <= 1)).all() and c.utterance[i] == c.token[i].min()
            assert c.word[i] == decode.word_confidence(r.tokens[i], r.frames[i], c.token[i], table, "min")
    print(name, dtype, rows, "rows; largest differences", worst, "; 3 x ERR", bound, "; ratio", worst / bound)
    assert rows == {"CFG": 44, "CFG32": 55, "CFGV": 57}[name]
    # the model-level entry point runs the encoder itself and gives the same bits; other measures reuse the statistics
    again = m.confidence(xs.cuda(), xlen, w.results, method="entropy", aggregate="mean")
    for c, a in zip(got, again):
        for i in range(len(c)):
            assert np.array_equal(c.raw[i], a.raw[i], equal_nan=True) and np.array_equal(c.top[i], a.top[i])
            assert np.array_equal(a.token[i], decode.confidence_measure(a.raw[i], V, "entropy"))
            assert a.word[i] is None


# ------------------------------------------------------------------------------------------- 4. chunks
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["CFG", "CFGV"])
def test_chunked_pass_gives_the_bits_of_the_unchunked_one(hip_lib, name, dtype):
    from edgedict_amd import decode
    sd, xs, xlen, _, _, _ = C.oracle_lists(name)
    w = C.wrapped(name)
    m = _engine(sd, CFGS[name][0], dtype)
    enc, lens = _encoded(m, xs, xlen)
    whole = decode.hypothesis_confidence(m, enc, lens, w.results)
    for chunk in (7, 1000):
        parts = decode.hypothesis_confidence(m, enc, lens, w.results, chunk_rows=chunk)
        for a, b in zip(whole, parts):
            for i in range(len(a)):
                assert np.array_equal(a.raw[i], b.raw[i]) and np.array_equal(a.top[i], b.top[i])
    assert sum(len(t) for r in w.results for t in r.tokens) > 7


# ------------------------------------------------------------------------------------------- 5. the engine's own lists
def _assert_reproduces_token_logp(conf, res):
    n = 0
    for c, r in zip(conf, res):
        for i in range(len(r)):
            np.testing.assert_allclose(c.raw[i][:, 0], r.token_logp[i], rtol=2 * TOL["rtol"], atol=2 * TOL["atol"])
            n += len(r.tokens[i])
    assert n > 0
    return n


@pytest.mark.parametrize("search", ["sync", "best_first"])
@pytest.mark.parametrize("name", ["CFG", "CFG32"])
def test_pass_reproduces_the_token_logp_of_the_engines_own_lists(hip_lib, name, search):
    """Plain searches, fp32: each side is within TOL of the same oracle value, hence 2 x TOL."""
    sd, xs, xlen = _inputs(name)
    m = _engine(sd, CFGS[name][0])
    if search == "sync":
        res = m.sync_beam_search_nbest(xs.cuda(), xlen, W=4)
    else:
        res = m.beam_search_nbest(xs.cuda(), xlen, W=4, max_expansions=400)
    print(name, search, _assert_reproduces_token_logp(m.confidence(xs.cuda(), xlen, res), res), "token rows")


def _with_head(name, seed=7):
    """The model of ``_inputs(name)`` with a CTC head whose blank bias puts the median frame's blank posterior (found on
    the oracle's encoder output, on the host) on 0.5: skip_blank=0.5 then drops about half of the frames."""
    from edgedict_amd.models import Transducer
    cfg = CFGS[name][0]
    sd, xs, xlen = _inputs(name)
    torch.manual_seed(seed)
    m = Transducer(enc_dropout=0.0, dec_dropout=0.0, output_loss=False, ctc_weight=0.3, **cfg)
    m.load_state_dict(sd, strict=False)
    h_enc, lens = S.encode(sd, xs, xlen)
    with torch.no_grad():
        m.ctc_head.weight *= 4.0
        m.ctc_head.bias.zero_()
        z = (h_enc.double() @ m.ctc_head.weight.double().t()).numpy()
        live = np.arange(z.shape[1])[None, :] < np.asarray(lens)[:, None]
        zm = z[:, :, 1:].max(axis=2)
        odds = z[:, :, 0] - (zm + np.log(np.exp(z[:, :, 1:] - zm[:, :, None]).sum(axis=2)))
        m.ctc_head.bias[0] = float(-np.median(odds[live]))
    return m.cuda().eval(), xs, xlen


def test_pass_reproduces_token_logp_of_a_skip_blank_search(hip_lib):
    from edgedict_amd import decode
    m, xs, xlen = _with_head("CFG")
    m.compute_dtype = "fp32"
    enc, lens = _encoded(m, xs, xlen)
    sk = decode.skip_blank_frames(m, enc, lens, 0.5)
    assert 0 < int(np.sum(sk.lens)) < int(np.sum(lens))                # frames were dropped, and frames were kept
    res = m.sync_beam_search_nbest(xs.cuda(), xlen, W=4, skip_blank=0.5)
    _assert_reproduces_token_logp(m.confidence(xs.cuda(), xlen, res), res)


# ------------------------------------------------------------------------------------------- 6. the CTC head
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_ctc_head_confidence_on_ctc_beam_search_lists(hip_lib, dtype):
    from edgedict_amd import decode
    m, xs, xlen = _with_head("CFG")
    m.compute_dtype = dtype
    V = CFG["vocab_size"]
    res = m.ctc_beam_search(xs.cuda(), xlen, W=4)
    got = m.confidence(xs.cuda(), xlen, res, head="ctc")
    enc, lens = _encoded(m, xs, xlen)
    with torch.no_grad():
        z = m._ctc_logits(enc).double().cpu().numpy()            # the head's logits as the kernel read them
    n = 0
    for b, (c, r) in enumerate(zip(got, res)):
        for i in range(len(r)):
            if not len(r.tokens[i]):
                continue
            rows = z[b, r.frames[i].astype(np.int64)]
            exact, etop, gap, bound = C.kernel_bounds(rows, r.tokens[i])
            np.testing.assert_allclose(c.raw[i][:, 0], r.token_logp[i], rtol=1e-5, atol=1e-5)
            np.testing.assert_allclose(c.raw[i][:, :3], exact[:, :3], rtol=1e-5, atol=1e-5)
            assert (np.abs(c.raw[i][:, 3:] - exact[:, 3:]) <= bound[3:]).all()
            keep = gap >= C.MIN_MARGIN
            assert np.array_equal(c.top[i][keep], etop[keep])
            n += len(r.tokens[i])
    print("ctc head,", dtype, n, "token rows")
    assert n > 0
    same = decode.ctc_hypothesis_confidence(m, enc, lens, res)
    assert all(np.array_equal(a.raw[i], b.raw[i]) for a, b in zip(got, same) for i in range(len(a)))
    plain = _engine(_inputs("CFG")[0], CFG)
    with pytest.raises(RuntimeError, match="no CTC head"):
        plain.confidence(xs.cuda(), xlen, res, head="ctc")


# ------------------------------------------------------------------------------------------- 7. errors, the empty case
def test_errors_come_before_any_launch_and_empty_lists_launch_nothing(hip_lib, monkeypatch):
    from edgedict_amd import _lib, decode, ops
    from edgedict_amd.decode import NBestResult
    sd, xs, xlen = _inputs("CFG")
    m = _engine(sd, CFG)
    enc, lens = _encoded(m, xs, xlen)
    B, T, _ = enc.shape
    lens = lens.copy()
    lens[1] = T - 1

    def one(tokens, frames):
        return NBestResult([np.asarray(tokens, dtype=np.int64)], [np.asarray(frames, dtype=np.int32)],
                           [np.zeros(len(tokens))], [0.0])

    ok = [one([5, 6], [0, 1]), one([], []), one([7], [T - 1])]
    good = decode.hypothesis_confidence(m, enc, lens, ok)
    assert [len(c.token[0]) for c in good] == [2, 0, 1] and np.isnan(good[1].utterance[0])

    def boom(*a, **k):
        raise AssertionError("a launch")

    monkeypatch.setattr(_lib, "call", boom)
    monkeypatch.setattr(ops, "call", boom)
    monkeypatch.setattr(ops, "gemm", boom)
    for bad, msg in (([one([5], [T]), ok[1], ok[2]], "a frame outside"),
                     ([ok[0], one([5], [T - 1]), ok[2]], "a frame outside"),           # behind lens[1] = T - 1
                     ([one([5], [-1]), ok[1], ok[2]], "a frame outside"),
                     ([one([5, M.NUL], [0, 1]), ok[1], ok[2]], "blank or outside"),
                     ([one([CFG["vocab_size"]], [0]), ok[1], ok[2]], "blank or outside"),
                     ([one([-1], [0]), ok[1], ok[2]], "blank or outside"),
                     (ok[:2], "2 lists for a batch of 3")):
        with pytest.raises(ValueError, match=msg):
            decode.hypothesis_confidence(m, enc, lens, bad)
    for kw in (dict(method="renyi"), dict(alpha=0.0), dict(alpha=1.5), dict(aggregate="max")):
        with pytest.raises(ValueError):
            decode.hypothesis_confidence(m, enc, lens, ok, **kw)
    with pytest.raises(ValueError, match="lens must be"):
        decode.hypothesis_confidence(m, enc, [T + 1, 1, 1], ok)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        decode.hypothesis_confidence(m, enc.cpu(), lens, ok)
    # every hypothesis empty: nothing is launched (every launch path raises here), empty arrays come back
    empty = decode.hypothesis_confidence(m, enc, lens, [one([], [])] * 3, words=decode.WordTable(np.zeros(40, dtype=bool)))
    for c in empty:
        assert len(c) == 1 and c.token[0].shape == (0,) and c.raw[0].shape == (0, 5) and c.top[0].shape == (0,)
        assert c.top[0].dtype == np.int32 and np.isnan(c.utterance[0]) and c.word[0] == []
