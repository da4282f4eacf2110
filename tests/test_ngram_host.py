"""CPU: the back-off n-gram's host side (edgedict_amd/ngram.py) - the hand-written ARPA file's known answers, the
round trip through ``to_arpa``, the normalisation and the table invariants of the trained models the GPU tests use, the
margin condition of every case tests/test_ctc_beam_ngram_gpu.py runs, the struct mirror, and every argument refusal of
the three native entry points (fake pointers: every call fails a check before the device is touched)."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import ctc_beam_ref as BR
import ngram_ref as NR

LN10 = math.log(10.0)
TINY = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ngram", "tiny.arpa")
A, B_ = 4, 5                                  # the ids of the file's words
MODELS = [(8, 1), (8, 2), (29, 3), (32, 3), (40, 3), (40, 4), (80, 5), (520, 3)]


def _tiny(**kw):
    from edgedict_amd.ngram import NGramLM
    return NGramLM.from_arpa(TINY, {"a": A, "b": B_}, 8, **kw)


def test_from_arpa_takes_a_path_object_a_path_string_and_the_text():
    import pathlib
    from edgedict_amd.ngram import NGramLM
    lm = _tiny()
    _same_tables(lm, NGramLM.from_arpa(pathlib.Path(TINY), {"a": A, "b": B_}, 8))
    _same_tables(lm, NGramLM.from_arpa(open(TINY).read(), {"a": A, "b": B_}, 8))


def test_known_answers_of_the_hand_written_file():
    """The file's log10 sums times ln 10, at 1e-12; an id without a unigram takes <unk> plus the context's back-offs."""
    lm = _tiny()
    assert (lm.order, lm.n_states, lm.n_arcs, lm.start) == (2, 4, 3, lm._index[(2,)])
    assert abs(lm.score([A, B_], bos=True, eos=True) - (-0.92082 * LN10)) <= 1e-12
    want = (-0.30103 - 0.52288) + (-0.17609 - 0.52288) + (-0.30103 - 0.69897)
    assert abs(want - -2.52288) <= 1e-12
    assert abs(lm.score([B_, A], bos=True, eos=True) - want * LN10) <= 1e-12
    # without <s> and </s>: the unigram of a, then the bigram a b
    assert abs(lm.score([A, B_], bos=False) - (-0.52288 - 0.39794) * LN10) <= 1e-12
    # id 6 has no unigram: after a it costs a's back-off plus <unk>, and leaves the empty context
    l, s = lm.step(lm._index[(A,)], 6)
    assert abs(l - (-0.30103 - 1.0) * LN10) <= 1e-12 and s == 0
    assert abs(lm.step(lm.start, 6)[0] - (-0.30103 - 1.0) * LN10) <= 1e-12
    assert lm.step(0, 6) == (-1.0 * LN10, 0)
    # the order of additions: ((0 + backoff) + unigram), not a re-associated sum
    s_b = lm._index[(B_,)]
    assert lm.step(s_b, A)[0] == (0.0 + lm.backoff[s_b]) + lm.uni_lp[A]
    # bad tokens
    assert lm.score([A, 0]) == -np.inf and lm.score([8]) == -np.inf and lm.score([-1]) == -np.inf
    assert lm.score([]) == 0.0 and lm.uni_lp[0] == 0.0


def test_unknown_ids_need_unk_or_unk_logp():
    from edgedict_amd.ngram import NGramLM
    text = open(TINY).read().replace("-1.0\t<unk>\n", "")
    with pytest.raises(ValueError, match="neither <unk> nor unk_logp"):
        NGramLM.from_arpa(text, {"a": A, "b": B_}, 8)
    lm = NGramLM.from_arpa(text, {"a": A, "b": B_}, 8, unk_logp=-3.0)
    assert abs(lm.uni_lp[6] + 3.0) <= 1e-15 and np.isfinite(lm.uni_lp).all()
    with pytest.raises(ValueError, match="not in `symbols`"):
        NGramLM.from_arpa(text, {"a": A}, 8, unk_logp=-3.0)
    with pytest.raises(ValueError, match="blank or BOS"):
        NGramLM.from_arpa(text, {"a": A, "b": 2}, 8, unk_logp=-3.0)
    with pytest.raises(ValueError, match="order 7"):
        NGramLM.train([[3, 4]], 7, 8)


def _same_tables(x, y):
    from edgedict_amd.ngram import _TABLES
    assert (x.V, x.order, x.n_states, x.n_arcs, x.start) == (y.V, y.order, y.n_states, y.n_arcs, y.start)
    for name in _TABLES:
        a, b = getattr(x, name), getattr(y, name)
        assert a.dtype == b.dtype and a.shape == b.shape and (a == b).all(), name


def test_arpa_round_trip_gives_identical_tables():
    from edgedict_amd.ngram import NGramLM
    lm = _tiny()
    _same_tables(lm, NGramLM.from_arpa(lm.to_arpa(), {"a": A, "b": B_}, 8))
    for V, order in ((8, 2), (29, 3), (40, 4)):
        lm = NR.model(V, order)
        back = NGramLM.from_arpa(lm.to_arpa(), None, V)
        _same_tables(lm, back)
        _same_tables(back, NGramLM.from_arpa(back.to_arpa(), None, V))
    lm = NR.closure_model()
    _same_tables(lm, NGramLM.from_arpa(lm.to_arpa(), None, 12))


@pytest.mark.parametrize("V,order", MODELS, ids=["V%d-o%d" % m for m in MODELS])
def test_trained_models_are_normalised_and_their_tables_consistent(V, order):
    """For every state, sum_k exp(step(s, k)) over all non-blank symbols and eos is 1 within 1e-9; fail drops the oldest
    token, arc_next / uni_next name the longest suffix that is a state, rows are sorted, state 0's row is empty."""
    lm = NR.model(V, order)
    assert lm.order == order and lm.n_states == len(lm.contexts) and lm.contexts[0] == ()
    assert (order == 1) == (lm.n_states == 1)
    index = {h: s for s, h in enumerate(lm.contexts)}
    worst = 0.0
    for s in range(lm.n_states):
        total = sum(math.exp(lm.step(s, k)[0]) for k in range(V + 1) if k != lm.blank)
        worst = max(worst, abs(total - 1.0))
    print("normalisation V %d order %d: %d states, %d arcs, max |sum - 1| %.3g" % (V, order, lm.n_states, lm.n_arcs, worst))
    assert worst <= 1e-9

    def longest(h):
        h = h[-(order - 1):] if order > 1 else ()
        while h not in index:
            h = h[1:]
        return index[h]

    assert lm.row_ptr[0] == 0 and lm.row_ptr[1] == 0 and lm.row_ptr[-1] == lm.n_arcs
    assert lm.start == index.get((lm.bos,), 0) and (order == 1 or lm.start != 0)
    for s, h in enumerate(lm.contexts):
        assert len(h) <= order - 1 and lm.blank not in h and lm.eos not in h
        lo, hi = int(lm.row_ptr[s]), int(lm.row_ptr[s + 1])
        assert (np.diff(lm.arc_tok[lo:hi]) > 0).all()
        if s:
            assert lm.contexts[lm.fail[s]] == h[1:]
        for a in range(lo, hi):
            k = int(lm.arc_tok[a])
            assert 0 <= k <= V and k != lm.blank
            assert lm.arc_next[a] == (0 if k == lm.eos else longest(h + (k,)))
    for k in range(V):
        assert lm.uni_next[k] == (0 if k == lm.blank else longest((k,)))
    assert np.isfinite(lm.uni_lp).all() and (lm.backoff <= 0).all()


def test_the_wide_and_the_closure_model_have_the_rows_the_gpu_tests_need():
    lm = NR.wide_model()
    s = lm._index[(3,)]
    assert lm.row_ptr[s + 1] - lm.row_ptr[s] >= 130 and lm.V == 520 and lm.order == 2
    total = sum(math.exp(lm.step(s, k)[0]) for k in range(lm.V + 1) if k != lm.blank)
    assert abs(total - 1.0) <= 1e-9
    lm = NR.closure_model()
    empty = [h for s, h in enumerate(lm.contexts) if s and lm.row_ptr[s + 1] == lm.row_ptr[s]]
    assert set(empty) == {(5,), (7,), (6, 7)} and (5, 6, 7) in lm._index
    assert lm.step(lm._index[(5, 6, 7)], 8) == (-0.125 * LN10, 0)
    assert lm.step(lm._index[(5,)], 9) == ((0.0 + -0.25 * LN10) + -1.5 * LN10, 0)
    # walking 5 6 7 8 never reaches (5, 6, 7) - (5, 6) is no state -: 5, then 5's back-off and <unk>, then <unk> twice,
    # the last one from the arc-less state (7,)
    unk = -1.5 * LN10
    assert lm.start == 0 and lm.step(0, 7) == (unk, lm._index[(7,)])
    assert lm.score([5, 6, 7, 8]) == (((0.0 + -0.4 * LN10) + ((0.0 + -0.25 * LN10) + unk)) + unk) + (0.0 + unk)


def test_oracle_with_a_zero_weight_is_the_plain_oracle():
    """weight = bonus = 0: the fused restatement decides and scores as ctc_beam_ref.search_one does, bit for bit; with
    a weight every logp minus the LM total is the plain score of that prefix (unpruned)."""
    z = BR.make_logits(5, 8, 3)
    lm = NR.model(8, 2)
    plain, mp, n0 = BR.search_one(z, 4, 7)
    fused, mf, n1 = NR.search_one(z, 4, 7, lm, 0.0, 0.0)
    assert [(h.tokens, h.frames, h.logp) for h in plain] == [(h.tokens, h.frames, h.logp) for h in fused]
    assert mp == mf and n0 == n1
    z = np.random.default_rng(1).standard_normal((3, 8))  # 1 + 7 + 49 + 343 prefixes at most: nothing is cut
    base = {tuple(h.tokens): h.logp for h in BR.search_one(z, 1000, 7)[0]}
    fused = NR.search_one(z, 1000, 7, lm, 0.5, 0.3)[0]
    assert {tuple(h.tokens) for h in fused} == set(base)
    for h in fused:
        ln = 0.0
        s = lm.start
        for k in h.tokens:
            l, s = lm.step(s, k)
            ln = ln + (0.5 * l + 0.3)
        assert abs((h.logp - ln) - base[tuple(h.tokens)]) <= 1e-12, h.tokens


# ------------------------------------------------------------------------------------------------ the margin condition
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_every_stored_seed_meets_its_margin(dtype):
    """Every case of tests/test_ctc_beam_ngram_gpu.py: margin >= 1e-3 (bf16 cases listed as tied: over the non-zero
    gaps) with the LM terms in the scores, and the fused top-1 differs from the plain one."""
    worst = np.inf
    for shape in NR.SHAPES:
        z, hyps, m, nodes, plain, _ = NR.case(shape, dtype)
        tied = shape in NR.BF16_TIED
        assert NR.stored_margin(m, dtype, tied) >= NR.MARGIN, (shape, m)
        assert NR.lm_acts((z, hyps, m, nodes, plain, None)), shape
        assert len(hyps) == min(shape[2], nodes)
        worst = min(worst, NR.stored_margin(m, dtype, tied))
    r = NR.RAGGED
    for i, (Tb, seed) in enumerate(zip(r["T"], r["seeds"][dtype])):
        m = NR.case((Tb, r["V"], r["W"], r["cand"], r["order"]), dtype, seed)[2]
        assert NR.stored_margin(m, dtype, (dtype, i) in r["tied"]) >= NR.MARGIN, (Tb, m)
    c = NR.case(NR.BOTH_SHAPE, dtype, NR.BOTH_SEEDS[dtype], True)
    assert NR.stored_margin(c[2], dtype, dtype in NR.BOTH_TIED) >= NR.MARGIN and NR.both_act(c)
    print("margin", dtype, "smallest %.3g" % worst)


# ------------------------------------------------------------------------------------------------ the native surface
def test_struct_mirror_abi_version_and_symbols(hip_lib):
    from edgedict_amd import _lib
    from edgedict_amd.ngram import CtcBeamOpts, NGramStruct
    want = {"edgedict_ngram_lm_struct_bytes", "edgedict_ngram_logprobs", "edgedict_ngram_score",
            "edgedict_ctc_beam_search_fused"}
    assert want <= set(_lib.declared_symbols())
    for name in want:
        assert hasattr(hip_lib, name), name
    assert hip_lib.edgedict_ngram_lm_struct_bytes.restype is ctypes.c_size_t
    assert ctypes.sizeof(NGramStruct) == hip_lib.edgedict_ngram_lm_struct_bytes() == 104
    assert ctypes.sizeof(CtcBeamOpts) == 16
    assert hip_lib.edgedict_abi_version() == 2
    import edgedict_amd
    from edgedict_amd.ngram import NGramLM
    assert edgedict_amd.NGramLM is NGramLM


def _fake():
    buf = ctypes.create_string_buffer(b"\x01" * 256, 256)
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def _struct(fake, **kw):
    from edgedict_amd.ngram import _TABLES, NGramStruct
    s = NGramStruct()
    s.V, s.order, s.S, s.n_arcs, s.start, s.blank = 16, 3, 5, 7, 1, 0
    for name in _TABLES:
        setattr(s, name, fake.value)
    s.weight, s.length_bonus = 0.5, 0.0
    for k, v in kw.items():
        setattr(s, k, v)
    return s


BAD_TABLES = [(dict(V=1), b"V = 1"), (dict(order=0), b"order = 0"), (dict(order=7), b"order = 7"),
              (dict(S=0), b"bad n-gram tables"), (dict(n_arcs=-1), b"bad n-gram tables"),
              (dict(start=5), b"start state 5"), (dict(start=-1), b"start state -1"), (dict(blank=16), b"blank 16")]


def test_scorer_and_rows_refuse_bad_arguments_before_any_launch(hip_lib):
    from edgedict_amd.ngram import _TABLES
    buf, f = _fake()
    err = hip_lib.edgedict_last_error
    rows = lambda lm, states=f, R=3, lp=f: hip_lib.edgedict_ngram_logprobs(lm, states, R, lp, None, None)
    score = lambda lm, hyps=f, lens=f, B=2, N=3, U=4, total=f: hip_lib.edgedict_ngram_score(lm, hyps, lens, None, B, N, U,
                                                                                           1, 0, total, None, None)
    for call, what in ((rows, b"ngram_logprobs"), (score, b"ngram_score")):
        assert call(None) == -1 and err().startswith(what) and b"not a pointer" in err()
        assert call(ctypes.c_void_p(16)) == -1 and b"not a pointer" in err()
        for kw, word in BAD_TABLES:
            assert call(ctypes.byref(_struct(f, **kw))) == -1, kw
            assert err().startswith(what) and word in err(), (kw, err())
        for name in _TABLES:
            assert call(ctypes.byref(_struct(f, **{name: None}))) == -1 and b"null n-gram table" in err(), name
    ok = _struct(f)
    assert rows(ctypes.byref(ok), R=0) == -1 and b"R = 0" in err()
    assert rows(ctypes.byref(ok), states=None) == -1 and b"null pointer" in err()
    assert rows(ctypes.byref(ok), lp=None) == -1 and b"null pointer" in err()
    assert rows(ctypes.byref(_struct(f, V=1 << 20)), R=1 << 12) == -1 and b"exceeds 2^31" in err()
    assert score(ctypes.byref(ok), B=0) == -1 and b"B, N must be positive" in err()
    assert score(ctypes.byref(ok), N=0) == -1 and b"B, N must be positive" in err()
    assert score(ctypes.byref(ok), U=-1) == -1 and b"U = -1" in err()
    assert score(ctypes.byref(ok), hyps=None) == -1 and b"null pointer" in err()
    assert score(ctypes.byref(ok), lens=None) == -1 and b"null pointer" in err()
    assert score(ctypes.byref(ok), total=None) == -1 and b"null pointer" in err()


def test_fused_search_refuses_bad_arguments_before_any_launch(hip_lib):
    from edgedict_amd.bias import BeamBias
    from edgedict_amd.ngram import _TABLES, CtcBeamOpts
    buf, f = _fake()
    err = hip_lib.edgedict_last_error

    def run(lm=None, bias=None, opts=True, V=16, blank=0, W=4, cand=8, logits=f, ws=f):
        o = CtcBeamOpts(bias=None if bias is None else ctypes.addressof(bias),
                        ngram=None if lm is None else ctypes.addressof(lm))
        o = ctypes.byref(o) if opts is True else opts
        return hip_lib.edgedict_ctc_beam_search_fused(logits, 0, f, 2, 5, V, blank, W, cand, o, f, f, f, f, f, f, ws, None)

    # the plain search's own checks come first
    for kw, word in ((dict(W=0), b"W = 0"), (dict(cand=65), b"cand = 65"), (dict(V=1), b"V = 1"), (dict(blank=16), b"blank"),
                     (dict(logits=None), b"null pointer"), (dict(ws=ctypes.c_void_p(f.value + 4)), b"aligned")):
        assert run(_struct(f), **kw) == -1 and word in err(), (kw, err())
    assert run(opts=ctypes.c_void_p(2)) == -1 and b"opts is not a pointer" in err()
    for kw, word in BAD_TABLES:
        if "blank" in kw:
            continue
        assert run(_struct(f, **kw)) == -1 and err().startswith(b"ctc_beam_search") and word in err(), (kw, err())
    for name in _TABLES:
        assert run(_struct(f, **{name: None})) == -1 and b"null n-gram table" in err(), name
    assert run(_struct(f, V=12)) == -1 and b"n-gram's vocabulary = 12 differs from the head's V = 16" in err()
    assert run(_struct(f, blank=3)) == -1 and b"n-gram's blank = 3" in err()
    for kw in (dict(weight=float("nan")), dict(weight=float("inf")), dict(weight=-0.5), dict(length_bonus=float("inf")),
               dict(length_bonus=float("nan"))):
        assert run(_struct(f, **kw)) == -1 and b"must be finite" in err(), kw
    # the bias list is still checked, with or without an n-gram
    bad = BeamBias()
    bad.S, bad.V, bad.n_exc = 1, 12, 0
    assert run(_struct(f), bias=bad) == -1 and b"bias list's vocabulary" in err()
    assert run(None, bias=bad) == -1 and b"bias list's vocabulary" in err()


def test_python_surface_refuses_bad_lm_arguments():
    from edgedict_amd.decode import NBestResult, lm_rescore
    from edgedict_amd.lm import LMModel
    from edgedict_amd.loss import ctc_prefix_beam
    z = torch.zeros(2, 5, 8)
    al = torch.tensor([5, 4], dtype=torch.int32)
    lm = NR.model(8, 2)
    rnn = LMModel.__new__(LMModel)
    with pytest.raises(TypeError, match="NGramLM"):
        ctc_prefix_beam(z, al, lm=rnn, lm_weight=0.5)
    with pytest.raises(ValueError, match="lm_weight is required"):
        ctc_prefix_beam(z, al, lm=lm)
    with pytest.raises(ValueError, match="lm_weight without lm"):
        ctc_prefix_beam(z, al, lm_weight=0.5)
    for w in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="lm_weight must be a finite number >= 0"):
            ctc_prefix_beam(z, al, lm=lm, lm_weight=w)
    with pytest.raises(ValueError, match="length_bonus must be finite"):
        ctc_prefix_beam(z, al, lm=lm, lm_weight=0.5, length_bonus=float("inf"))
    with pytest.raises(ValueError, match="vocabulary"):
        ctc_prefix_beam(z, al, lm=NR.model(29, 3), lm_weight=0.5)
    with pytest.raises(ValueError, match="blank"):
        ctc_prefix_beam(z, al, blank=3, lm=lm, lm_weight=0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ctc_prefix_beam(z, al, lm=lm, lm_weight=0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lm.logprobs(torch.zeros(3, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lm.score_nbest(torch.zeros(1, 2, 3, dtype=torch.int32), torch.zeros(1, 2, dtype=torch.int32))
    with pytest.raises(ValueError, match="hyp_lens"):
        lm.score_nbest(torch.zeros(1, 2, 3, dtype=torch.int32), torch.zeros(2, 2, dtype=torch.int32))
    r = NBestResult([np.array([3, 4])], [np.array([0, 1], dtype=np.int32)], [np.zeros(2)], np.array([-1.0]))
    with pytest.raises(TypeError, match="NGramLM"):
        lm_rescore([r], rnn, 0.5)
    with pytest.raises(ValueError, match="weight must be finite"):
        lm_rescore([r], lm, -1.0)
    # lm_logp is carried by ranked() as ctc_logp is
    two = NBestResult([np.array([3]), np.array([4])], [np.zeros(1, np.int32)] * 2, [np.zeros(1)] * 2, np.array([-2.0, -1.0]),
                      np.array([-5.0, -6.0]), np.array([-7.0, -8.0]))
    rk = two.ranked()
    assert rk.logp.tolist() == [-1.0, -2.0] and rk.ctc_logp.tolist() == [-6.0, -5.0] and rk.lm_logp.tolist() == [-8.0, -7.0]
    with pytest.raises(ValueError, match="lm_logp"):
        NBestResult([np.array([3])], [np.zeros(1, np.int32)], [np.zeros(1)], np.array([-2.0]), None, np.zeros(2))
