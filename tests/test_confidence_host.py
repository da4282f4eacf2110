"""Host tests (no GPU) of the confidence pass: the oracle tests/confidence_ref.py - the row statistics' closed forms,
its two routes to the measures, the teacher-forced replay against the lists' own token_logp, the measured ERR table and
the fp32 restatement's error that scale the bounds of tests/test_confidence_gpu.py -, decode.confidence_measure and the
word aggregation (pure host code of the engine), and the argument checks that come before any launch.

Measured here (this CPU): the fp32 numpy restatement of H and of log sum p^alpha differs from fp64 by at most 2.4e-6
over every case of ``confidence_ref.kernel_rows`` (V in 2 .. 2112, fp32 and bf16 values), so 4 x that error is below
the 1e-5 floor everywhere and the GPU bound on both columns is 1e-5; the three log-prob columns differ by at most
1.6e-5 on values as large as 160 (relative 1e-7), well inside rtol = atol = 1e-5."""
import ctypes

import numpy as np
import pytest
import torch

import confidence_ref as C
from oracle import models_ref as M
from test_sync_beam_gpu import CFGS

NAMES = ["CFG", "CFG32", "CFGV"]


# ------------------------------------------------------------------------------------------- closed forms
@pytest.mark.parametrize("V", [2, 40, 2112])
def test_uniform_and_one_hot_rows_have_their_closed_forms(V):
    from edgedict_amd import decode
    tok = np.array([1, 0], dtype=np.int32)
    z = np.zeros((2, V))
    z[0] += 3.25                                    # uniform at another level
    z[1, V - 1] += 80.0                             # one logit raised by 80
    stats, top, _ = C.row_stats(z, tok)
    assert top.tolist() == [0, V - 1]               # a tie takes the lowest index
    for method in decode.CONF_METHODS:
        got = decode.confidence_measure(stats, V, method, C.ALPHA)
        assert np.array_equal(got, C.measure(stats, V, method))
        np.testing.assert_allclose(got, C.measures_direct(z, tok)[method], rtol=0, atol=1e-12)
    for method in ("entropy", "tsallis"):
        got = decode.confidence_measure(stats, V, method, C.ALPHA)
        assert abs(got[0]) <= 1e-12, (method, got)
    # one logit raised by 80: the entropy measure is 1 within 1e-12.  The Tsallis measure of order 1/3 is not, and
    # cannot be: the V - 1 other symbols have p = e^-80 each and p^(1/3) = e^(-80/3) = 2.6e-12, so the exact value is
    # 1 - (V - 1) e^(-80/3) / (V^(2/3) - 1) (1 - 4.4e-12 at V = 2, 1 - 9.5e-12 at 40, 1 - 3.4e-11 at 2112); it is held
    # to that closed form within 1e-12, and to 1 within 1e-12 for a logit raised by 300
    assert abs(decode.confidence_measure(stats, V, "entropy")[1] - 1.0) <= 1e-12
    closed = 1.0 - (V - 1) * np.exp(-80.0 * C.ALPHA) / (V ** (1.0 - C.ALPHA) - 1.0)
    assert abs(decode.confidence_measure(stats, V, "tsallis", C.ALPHA)[1] - closed) <= 1e-12
    z[1, V - 1] += 220.0
    far, _, _ = C.row_stats(z, tok)
    for method in ("entropy", "tsallis", "max_prob"):
        assert abs(decode.confidence_measure(far, V, method, C.ALPHA)[1] - 1.0) <= 1e-12, method
    mp = decode.confidence_measure(stats, V, "max_prob")
    assert abs(mp[0] - 1.0 / V) <= 1e-12 and abs(mp[1] - 1.0) <= 1e-12
    assert abs(decode.confidence_measure(stats, V, "prob")[0] - 1.0 / V) <= 1e-12
    np.testing.assert_allclose(stats[0], [-np.log(V)] * 3 + [np.log(V), (1 - C.ALPHA) * np.log(V)], rtol=1e-12)


def test_a_sharper_row_is_never_less_confident_and_the_routes_agree():
    from edgedict_amd import decode
    g = np.random.default_rng(0)
    z = g.normal(size=(50, 40)) * g.uniform(0.1, 4.0, size=(50, 1))
    tok = g.integers(0, 40, 50).astype(np.int32)
    one, _, _ = C.row_stats(z, tok)
    two, _, _ = C.row_stats(2.0 * z, tok)
    direct = C.measures_direct(z, tok)
    for method in decode.CONF_METHODS:
        np.testing.assert_allclose(decode.confidence_measure(one, 40, method, C.ALPHA), direct[method], rtol=0, atol=1e-12)
    for method in ("entropy", "tsallis", "max_prob"):
        a, b = (decode.confidence_measure(s, 40, method, C.ALPHA) for s in (one, two))
        assert (b >= a).all(), method
    for alpha in (0.1, 0.5, 0.9):
        s, _, _ = C.row_stats(z, tok, alpha)
        np.testing.assert_allclose(decode.confidence_measure(s, 40, "tsallis", alpha),
                                   C.measures_direct(z, tok, alpha)["tsallis"], rtol=0, atol=1e-12)


def test_dead_rows_minus_inf_logits_and_stray_tokens_in_the_oracle():
    z = np.array([[1.0, -np.inf, 0.5, -np.inf], [-np.inf] * 4, [0.0, np.nan, 1.0, 2.0], [0.0, 1.0, 2.0, 3.0]])
    stats, top, _ = C.row_stats(z, np.array([1, 0, 0, 4]))
    assert top.tolist() == [0, -1, -1, 3]
    assert stats[0, 0] == -np.inf and np.isfinite(stats[0, 1:]).all()          # a -inf token: log 0, nothing else moves
    two, _, _ = C.row_stats(z[:1, [0, 2]], np.array([0]))
    np.testing.assert_allclose(stats[0, 1:], two[0, 1:], rtol=1e-15)           # the -inf logits added exactly nothing
    assert np.isnan(stats[1]).all() and np.isnan(stats[2]).all()
    assert np.isnan(stats[3, 0]) and np.isfinite(stats[3, 1:]).all()           # a token outside [0, V): logp alone


def test_confidence_measure_argument_rules():
    from edgedict_amd import decode
    s = np.zeros((3, 5))
    for bad in (0.0, 1.0, -0.5, 2.0, float("nan")):
        with pytest.raises(ValueError, match="alpha"):
            decode.confidence_measure(s, 40, "tsallis", bad)
    with pytest.raises(ValueError, match="method"):
        decode.confidence_measure(s, 40, "renyi")
    with pytest.raises(ValueError, match=r"\[\.\.\., 5\]"):
        decode.confidence_measure(np.zeros((3, 4)), 40)
    with pytest.raises(ValueError, match="two symbols"):
        decode.confidence_measure(s, 1)
    nan = decode.confidence_measure(np.full((2, 5), np.nan), 40)
    assert np.isnan(nan).all()
    assert decode.confidence_measure(np.zeros((0, 5)), 40).shape == (0,)


# ------------------------------------------------------------------------------------------- the restatement's error
def test_fp32_restatement_error_scales_the_kernel_bounds():
    worst = np.zeros(5)
    for bf16 in (False, True):
        for V in C.KERNEL_V:
            for Rn in C.KERNEL_R:
                z, tok = C.kernel_rows(V, Rn, bf16)
                assert z.shape == (Rn, V) and ((tok >= 0) & (tok < V)).all()
                if bf16:
                    assert np.array_equal(torch.from_numpy(z).to(torch.bfloat16).float().numpy(), z)
                exact, top, gap, bound = C.kernel_bounds(z, tok)
                assert (gap >= 0.9).all(), (V, Rn, gap)                      # no row is excluded from the arg-max check
                f32, top32, _ = C.row_stats(z, tok, dtype=np.float32)
                assert np.array_equal(top, top32)
                with np.errstate(invalid="ignore"):
                    d = np.abs(f32 - exact)
                d[np.isnan(d)] = 0.0                                           # (-inf) - (-inf): a -inf token on both sides
                worst = np.maximum(worst, d.max(axis=0))
                assert (d[:, :3] <= 1e-5 + 1e-5 * np.abs(np.where(np.isfinite(exact[:, :3]), exact[:, :3], 0))).all()
                assert bound[3] == 1e-5 and bound[4] == 1e-5, (V, Rn, bound)
    print("fp32 restatement against fp64, per column:", worst)
    assert worst[3] <= 2.5e-6 and worst[4] <= 2.5e-6
    # every kind of row occurs: -inf entries, a span of 160, the token on the arg max
    z, tok = C.kernel_rows(65, 9)
    assert np.isinf(z[1]).any() and z[2].max() - z[2].min() >= 150.0 and tok[3] == z[3].argmax()


# ------------------------------------------------------------------------------------------- the oracle's lists
@pytest.mark.parametrize("name,rows", [("CFG", 44), ("CFG32", 55), ("CFGV", 57)])
def test_teacher_forced_replay_reproduces_the_lists_own_token_logp(name, rows):
    _, _, _, _, lens, res = C.oracle_lists(name)
    exact = C.exact_stats(name)
    n, worst, small = 0, 0.0, 0
    for b, (r, st) in enumerate(zip(res, exact)):
        assert len(r) >= 1
        for h, (stats, top, gap) in zip(r, st):
            assert all(0 <= f < lens[b] for f in h["frames"]) and M.NUL not in h["tokens"]
            if not h["tokens"]:
                continue
            worst = max(worst, float(np.abs(stats[:, 0] - np.asarray(h["token_logp"])).max()))
            n += len(h["tokens"])
            small += int((gap < C.MIN_MARGIN).sum())
            assert (stats[:, 0] <= stats[:, 1]).all() and (stats[:, 3] >= 0).all()
    print(name, "rows", n, "replay against token_logp", worst, "gaps below MIN_MARGIN", small)
    assert n == rows and worst <= 2e-6 and small == 0


def test_a_list_with_a_near_tie_exists_and_is_not_used():
    """blank_bias 3.0, W = 10 on CFG: 1 row of 32 has a top-two gap below MIN_MARGIN - why the lists above are taken."""
    exact = C.exact_stats("CFG", 3.0, 10)
    gaps = np.concatenate([g for u in exact for _, _, g in u if len(g)])
    assert gaps.size == 32 and int((gaps < C.MIN_MARGIN).sum()) == 1


@pytest.mark.parametrize("name", NAMES)
def test_err_table_is_the_measured_one(name):
    """bf16: float64 arithmetic with deterministic roundings, reproduced within 2x; fp32: a float32 replay, whose last
    bits follow the host's matmul (another CPU gave up to 2.2x the table's figure) - within 5x.  The GPU test
    multiplies the live measurement, not the table."""
    for dtype, factor in (("fp32", 5.0), ("bf16", 2.0)):
        got, table = C.err(name, dtype), np.asarray(C.ERR_TABLE[(name, dtype)])
        print(name, dtype, "ERR", got)
        assert (got <= factor * table).all() and (got >= table / factor).all(), (name, dtype, got, table)
        for v in table:
            assert "%.1e" % v in C.__doc__


def test_rounded_replay_keeps_every_arg_max_of_the_exact_one():
    for name in NAMES:
        sd, _, _, h_enc, _, res = C.oracle_lists(name)
        exact = C.exact_stats(name)
        for cd in (torch.float32, torch.bfloat16):
            rounded = C.replay_stats(sd, h_enc.to(cd), C.pairs(res), cd)
            for u, v in zip(exact, rounded):
                for (_, top, gap), (_, rtop, _) in zip(u, v):
                    keep = gap >= (C.MIN_MARGIN if cd == torch.float32 else 0.25)
                    assert np.array_equal(top[keep], rtop[keep])


# ------------------------------------------------------------------------------------------- words
def _table():
    from edgedict_amd import decode
    end = np.zeros(12, dtype=bool)
    end[[5, 6, 7]] = True                       # BPE-style pieces ending in </w>
    return decode.WordTable(end, separators=[4])


def test_word_spans_end_markers_separators_and_a_trailing_partial_word():
    t = _table()
    assert t.spans([8, 5, 6, 9, 10, 7]) == [(0, 1), (2, 2), (3, 5)]
    assert t.spans([8, 9]) == [(0, 1)]                                  # no end marker: still a word
    assert t.spans([8, 5, 9]) == [(0, 1), (2, 2)]                       # a trailing partial word
    assert t.spans([]) == []
    assert t.spans([8, 9, 4, 10, 4, 4, 11]) == [(0, 1), (3, 3), (6, 6)]  # separators end a word and belong to none
    assert t.spans([4, 8, 4]) == [(1, 1)]
    assert t.spans([8, 5, 4, 9]) == [(0, 1), (3, 3)]                    # an end marker then a separator: one boundary
    assert t.spans([8, 50]) == [(0, 1)]                                 # an id outside the table ends nothing
    with pytest.raises(ValueError, match="separator"):
        from edgedict_amd import decode
        decode.WordTable(np.zeros(4, dtype=bool), [4])


def test_word_confidence_aggregates_and_frames():
    from edgedict_amd import decode
    t = _table()
    tokens, frames = [8, 5, 6, 9, 10, 7], [0, 2, 3, 7, 8, 11]
    c = np.array([0.9, 0.5, 0.8, 0.4, 1.0, 0.5])
    want = {"min": [0.5, 0.8, 0.4], "mean": [0.7, 0.8, (0.4 + 1.0 + 0.5) / 3], "prod": [0.45, 0.8, 0.2]}
    for how, vals in want.items():
        words = decode.word_confidence(tokens, frames, c, t, how)
        assert [w[:4] for w in words] == [(0, 1, 0, 2), (2, 2, 3, 3), (3, 5, 7, 11)]
        np.testing.assert_allclose([w[4] for w in words], vals, rtol=1e-15)
        assert decode.aggregate_confidence(c, how) == pytest.approx({"min": 0.4, "mean": 4.1 / 6, "prod": 0.072}[how])
    assert decode.word_confidence([], [], np.zeros(0), t) == []
    assert np.isnan(decode.aggregate_confidence([], "min"))
    with pytest.raises(ValueError, match="aggregate"):
        decode.aggregate_confidence(c, "max")


def test_word_table_from_a_tokenizers_piece_texts():
    from edgedict_amd import decode

    class Tok:                                  # tests/test_stream_gpu.py's stub vocabulary, with a space piece
        def id_to_token(self, i):
            return {0: "<nul>", 1: "<pad>", 2: "<bos>", 3: "<unk>", 4: " ", 5: "un", 6: "re"}.get(i, "t%d</w>" % i)

    class Wrapper:
        tokenizer = Tok()

    for tok in (Tok(), Wrapper()):
        t = decode.word_table(tok, 10)
        assert t.word_end.tolist() == [False] * 7 + [True] * 3 and t.separators == [4]
        assert t.spans([5, 7, 6, 6, 8, 4, 9]) == [(0, 1), (2, 4), (6, 6)]


# ------------------------------------------------------------------------------------------- before any launch
def test_python_entry_points_refuse_cpu_tensors_and_bad_arguments(hip_lib):
    from edgedict_amd import decode, loss
    from edgedict_amd.models import Transducer
    cfg = CFGS["CFG"][0]
    m = Transducer(enc_dropout=0.0, dec_dropout=0.0, output_loss=False, **cfg).eval()
    enc = torch.zeros(2, 5, cfg["enc_proj_size"])
    empty = [decode.NBestResult([np.zeros(0, np.int64)], [np.zeros(0, np.int32)], [np.zeros(0)], [0.0])] * 2
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        decode.hypothesis_confidence(m, enc, None, empty)
    for kw in (dict(method="renyi"), dict(alpha=1.0), dict(alpha=0.0), dict(alpha="x"), dict(aggregate="max"),
               dict(chunk_rows=0)):
        with pytest.raises(ValueError):
            decode.hypothesis_confidence(m, enc, None, empty, **kw)
    with pytest.raises(TypeError, match="WordTable"):
        decode.hypothesis_confidence(m, enc, None, empty, words=[True] * 40)
    with pytest.raises(RuntimeError, match="no CTC head"):
        decode.ctc_hypothesis_confidence(m, enc, None, empty)
    with pytest.raises(RuntimeError, match="no CTC head"):
        m.confidence(torch.zeros(2, 9, cfg["input_size"]), None, empty, head="ctc")
    with pytest.raises(ValueError, match="head"):
        m.confidence(torch.zeros(2, 9, cfg["input_size"]), None, empty, head="joint")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.confidence(torch.zeros(2, 9, cfg["input_size"]), None, empty)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        loss.row_confidence(torch.zeros(3, 8), torch.zeros(3, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        decode.confidence_hidden_rows(torch.zeros(3, 8), torch.zeros(3, 8), torch.zeros(2, dtype=torch.int32),
                                      torch.zeros(2, dtype=torch.int32))


def test_native_argument_errors_come_before_any_launch(hip_lib):
    from edgedict_amd import _lib
    names = {"edgedict_conf_hidden_rows", "edgedict_conf_row_stats"}
    assert names <= set(_lib.declared_symbols())
    buf = ctypes.create_string_buffer(64)
    fake = ctypes.c_void_p(ctypes.addressof(buf))
    ll, fl = ctypes.c_longlong, ctypes.c_float

    def stats(logits=fake, dtype=0, ld=40, n=8, rows=fake, tokens=fake, R=4, V=40, blank=0, alpha=1.0 / 3.0, out=fake,
              top=fake):
        return hip_lib.edgedict_conf_row_stats(logits, dtype, ll(ld), n, rows, tokens, R, V, blank, fl(alpha), out, top, None)

    for kw, msg in ((dict(dtype=5), b"bad dtype"), (dict(V=1, ld=1), b"V = 1"), (dict(ld=39), b"bad shape"),
                    (dict(R=0), b"bad shape"), (dict(rows=None, R=9), b"bad shape"), (dict(blank=40), b"blank 40 outside"),
                    (dict(blank=-1), b"blank -1 outside"), (dict(alpha=0.0), b"alpha"), (dict(alpha=1.0), b"alpha"),
                    (dict(alpha=float("nan")), b"alpha"), (dict(tokens=None), b"null pointer"),
                    (dict(out=None), b"null pointer"), (dict(top=None), b"null pointer"),
                    (dict(logits=None), b"null pointer")):
        assert stats(**kw) == -1, kw
        assert msg in hip_lib.edgedict_last_error() and hip_lib.edgedict_last_error().startswith(b"conf_row_stats"), kw

    def hidden(dtype=0, E1=fake, ne=4, D1=fake, nd=4, b1=None, er=fake, dr=fake, R=3, J=32, hid=fake):
        return hip_lib.edgedict_conf_hidden_rows(dtype, E1, ne, D1, nd, b1, er, dr, R, J, hid, None)

    for kw, msg in ((dict(dtype=2), b"bad dtype"), (dict(R=0), b"bad shape"), (dict(J=0), b"bad shape"),
                    (dict(ne=-1), b"bad shape"), (dict(E1=None), b"null pointer"), (dict(D1=None), b"null pointer"),
                    (dict(er=None), b"null pointer"), (dict(dr=None), b"null pointer"), (dict(hid=None), b"null pointer")):
        assert hidden(**kw) == -1, kw
        assert msg in hip_lib.edgedict_last_error() and hip_lib.edgedict_last_error().startswith(b"conf_hidden_rows"), kw
