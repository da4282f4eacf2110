"""CPU: the host side of CTC N-best rescoring.  The float64 oracle tests/ctc_score_ref.py that the GPU tests compare
against is pinned here on the enumeration of all V^T frame labellings; the combine-and-sort rule, ``NBestResult.ctc_logp``
and every argument error (raised before anything is launched) are checked without a device."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import ctc_ref as CR
import ctc_score_ref as SR

_KW = dict(vocab_embed_size=8, vocab_size=12, input_size=16, enc_hidden_size=16, enc_layers=2, enc_dropout=0.0,
           enc_proj_size=12, dec_hidden_size=8, dec_layers=1, dec_dropout=0.0, dec_proj_size=8, joint_size=16)
NEG = -np.inf


def _collapse(path, blank=0):
    out, prev = [], None
    for k in path:
        if k != blank and k != prev:
            out.append(k)
        prev = k
    return out


def _brute(logits, y, blank=0):
    """log of the summed probability of all V^T frame labellings that collapse to y (-inf: none does)."""
    lp = CR.log_softmax(logits)
    T, V = lp.shape
    terms = [sum(lp[t, k] for t, k in enumerate(path)) for path in itertools.product(range(V), repeat=T)
             if _collapse(path, blank) == list(y)]
    if not terms:
        return NEG
    m = max(terms)
    return m + np.log(sum(np.exp(v - m) for v in terms))


def test_oracle_equals_the_sum_over_all_frame_labellings():
    rng = np.random.default_rng(0)
    feasible = infeasible = 0
    for y in ([], [1], [1, 1], [1, 2], [2, 1, 2]):
        for T in range(1, 5):
            z = 2.0 * rng.normal(size=(T, 3))
            got, want = SR.score_one(z, y), _brute(z, y)
            assert SR.has_path(y, T) == np.isfinite(want), (y, T)
            if not np.isfinite(want):
                infeasible += 1
                assert got == NEG, (y, T)
                continue
            feasible += 1
            assert abs(got - want) <= 1e-12 * max(1.0, abs(want)), (y, T, got, want)
    assert feasible >= 12 and infeasible >= 5
    # no frame, a token outside [0, V), slots beyond n_hyp
    assert SR.score_one(np.zeros((0, 3)), []) == NEG and SR.score_one(np.zeros((2, 3)), [3]) == NEG
    z = rng.normal(size=(2, 4, 3))
    hyps = np.array([[[1, 2], [2, 0]], [[1, 1], [2, 2]]])
    got = SR.score_nbest(z, [4, 3], hyps, [[2, 1], [2, 2]], [2, 1])
    assert got[0, 0] == SR.score_one(z[0], [1, 2]) and got[0, 1] == SR.score_one(z[0], [2])
    assert got[1, 0] == SR.score_one(z[1, :3], [1, 1]) and got[1, 1] == NEG
    assert np.isfinite(got[0]).all() and np.isfinite(got[1, 0])


def test_combine_rule_weight_zero_minus_infinity_and_ties():
    from edgedict_amd.decode import combine_ctc
    logp = np.array([-3.0, -1.0, -1.0, -2.0, NEG])
    ctc = np.array([-1.0, NEG, -4.0, -4.0, NEG])
    # weight 0: logp itself (no 0 * inf -> nan), the stable sort of logp - the tie 1, 2 keeps its order
    for fn in (SR.combine, combine_ctc):
        comb, order = fn(logp, ctc, 0.0)
        assert np.array_equal(comb, logp) and not np.isnan(comb).any()
        assert list(order) == [1, 2, 3, 0, 4]
        # a -inf member goes last for weight > 0, exactly logp + w * ctc elsewhere
        comb, order = fn(logp, ctc, 0.5)
        assert comb[1] == NEG and comb[4] == NEG and not np.isnan(comb).any()
        assert comb[0] == -3.0 + 0.5 * -1.0 and comb[2] == -1.0 + 0.5 * -4.0 and comb[3] == -2.0 + 0.5 * -4.0
        assert list(order) == [2, 0, 3, 1, 4]
        # ties of the combined score keep their order
        comb, order = fn([-2.0, -1.0, -2.0, -1.0], [-2.0, -4.0, -2.0, -4.0], 0.5)
        assert list(comb) == [-3.0, -3.0, -3.0, -3.0] and list(order) == [0, 1, 2, 3]
        comb, order = fn([], [], 0.3)
        assert comb.shape == (0,) and order.shape == (0,)
    rng = np.random.default_rng(3)
    for _ in range(20):
        a, c = np.round(rng.normal(size=7), 1), np.round(rng.normal(size=7), 1)
        c[rng.integers(0, 7)] = NEG
        for w in (0.0, 0.3, 2.0):
            want, got = SR.combine(a, c, w), combine_ctc(a, c, w)
            assert np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1])


def _nbest(ctc=True):
    from edgedict_amd.decode import NBestResult
    tokens = [np.array([1, 2]), np.array([3]), np.array([1, 2]), np.array([], dtype=np.int64)]
    frames = [np.array([0, 4], dtype=np.int32), np.array([2], dtype=np.int32), np.array([1, 3], dtype=np.int32),
              np.zeros(0, dtype=np.int32)]
    tlp = [np.array([-0.5, -0.25]), np.array([-1.0]), np.array([-0.75, -0.5]), np.zeros(0)]
    logp = [-2.0, -1.0, -1.5, -4.0]
    if ctc:
        return NBestResult(tokens, frames, tlp, logp, ctc_logp=[-3.0, -5.0, -3.0, NEG])
    return NBestResult(tokens, frames, tlp, logp)


def test_nbest_result_carries_ctc_logp_through_ranked():
    from edgedict_amd.decode import NBestResult
    r = _nbest()
    assert r.ctc_logp.dtype == np.float64 and r.ctc_logp.tolist() == [-3.0, -5.0, -3.0, NEG]
    plain = r.ranked(merge=False)
    assert plain.logp.tolist() == [-1.0, -1.5, -2.0, -4.0]
    assert plain.ctc_logp.tolist() == [-5.0, -3.0, -3.0, NEG]
    assert [t.tolist() for t in plain.tokens] == [[3], [1, 2], [1, 2], []]
    merged = r.ranked(merge=True)
    assert [t.tolist() for t in merged.tokens] == [[3], [1, 2], []]
    assert merged.ctc_logp.tolist() == [-5.0, -3.0, NEG]              # the kept member's value
    assert merged.frames[1].tolist() == [1, 3]                        # the kept member is entry 2 (logp -1.5)
    np.testing.assert_allclose(merged.logp[1], np.log(np.exp(-2.0) + np.exp(-1.5)), rtol=1e-14)
    # the positional form of the constructor too, and an empty list
    again = NBestResult(r.tokens, r.frames, r.token_logp, r.logp, r.ctc_logp)
    assert np.array_equal(again.ctc_logp, r.ctc_logp)
    empty = NBestResult([], [], [], [], ctc_logp=[])
    for merge in (False, True):
        e = empty.ranked(merge=merge)
        assert len(e) == 0 and e.ctc_logp is not None and e.ctc_logp.shape == (0,)
    with pytest.raises(ValueError, match="ctc_logp"):
        NBestResult(r.tokens, r.frames, r.token_logp, r.logp, ctc_logp=[-1.0])


def test_nbest_result_built_the_old_way_has_no_ctc_logp():
    r = _nbest(ctc=False)
    assert r.ctc_logp is None
    assert r.ranked(merge=False).ctc_logp is None and r.ranked(merge=True).ctc_logp is None
    assert r.ranked().logp.tolist()[::2] == [-1.0, -4.0]


def test_ctc_rescore_checks_the_weight_before_it_touches_the_device():
    from edgedict_amd import decode
    from edgedict_amd.models import Transducer
    torch.manual_seed(0)
    m = Transducer(ctc_weight=0.3, **_KW)
    enc = torch.zeros(1, 4, 12)
    xs = torch.zeros(1, 4, 16)
    res = [_nbest(ctc=False)]
    for bad in (-0.1, float("inf"), float("-inf"), float("nan"), "x", None):
        with pytest.raises(ValueError, match="weight"):
            decode.ctc_rescore(m, enc, None, res, bad)
        with pytest.raises(ValueError, match="weight"):
            m.rescore_nbest(xs, None, res, bad)
    for bad in (-0.1, float("inf"), float("nan")):
        for fn in (decode.beam_search_nbest, decode.sync_beam_search_nbest, decode.beam_search_nbest_enc,
                   decode.sync_beam_search_nbest_enc, m.beam_search_nbest, m.sync_beam_search_nbest):
            with pytest.raises(ValueError, match="weight"):
                fn(*(() if getattr(fn, "__self__", None) is m else (m,)), xs, None, 2, ctc_rescore=bad)
    # a good weight gets as far as the device: CPU tensors are refused, nothing is computed on the host instead
    for w in (0.0, 0.3):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            decode.ctc_rescore(m, enc, None, res, w)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.ctc_score(xs, None, [[[1, 2]]])


def test_model_without_the_head_refuses():
    from edgedict_amd import decode
    from edgedict_amd.models import Transducer
    plain = Transducer(**_KW)
    xs = torch.zeros(1, 4, 16)
    res = [_nbest(ctc=False)]
    with pytest.raises(RuntimeError, match="no CTC head"):
        decode.ctc_rescore(plain, torch.zeros(1, 4, 12), None, res, 0.3)
    with pytest.raises(RuntimeError, match="no CTC head"):
        plain.rescore_nbest(xs, None, res, 0.3)
    with pytest.raises(RuntimeError, match="no CTC head"):
        plain.ctc_score(xs, None, [[[1]]])
    with pytest.raises(RuntimeError, match="no CTC head"):
        plain.beam_search_nbest(xs, None, 2, ctc_rescore=0.3)
    with pytest.raises(RuntimeError, match="no CTC head"):
        plain.sync_beam_search_nbest(xs, None, 2, ctc_rescore=0.3)


def test_new_symbols_are_declared_and_exported(hip_lib):
    from edgedict_amd import _lib
    for name in ("edgedict_ctc_score_workspace_bytes", "edgedict_ctc_score_nbest"):
        assert name in _lib.declared_symbols()
        assert hasattr(hip_lib, name)
    assert hip_lib.edgedict_abi_version() == 2


def test_workspace_holds_the_two_row_arrays_only(hip_lib):
    ws = hip_lib.edgedict_ctc_score_workspace_bytes
    for B, T in ((1, 1), (3, 17), (64, 200)):
        n = ws(B, T, 10, 100)
        assert 8 * B * T <= n < 4096 + 16 * B * T
        assert n == ws(B, T, 10, 0) == ws(B, T, 1, 1023) == ws(B, T, 32, 7)
        assert n % 16 == 0
    for bad in ((0, 5, 1, 1), (2, 0, 1, 1), (2, 5, 0, 1), (2, 5, 33, 1), (2, 5, 1, -1), (2, 5, 1, 1024)):
        assert ws(*bad) == 0, bad


def test_argument_errors_are_raised_before_any_launch(hip_lib):
    """Null pointers, N outside [1, 32], U = 1024, blank out of range, a bad dtype code, a misaligned workspace: -1
    with a message, no device needed; U = 0 may leave hyps null, n_hyp may always be null."""
    buf = ctypes.create_string_buffer(128)
    fake = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    odd = ctypes.c_void_p(fake.value + 4)

    def score(logits=fake, dtype=0, al=fake, hyps=fake, hl=fake, nh=fake, N=2, U=3, V=16, blank=0, scores=fake, ws=fake):
        return hip_lib.edgedict_ctc_score_nbest(logits, dtype, al, hyps, hl, nh, 2, 5, N, U, V, blank, scores, ws, None)

    for name in ("logits", "al", "hyps", "hl", "scores", "ws"):
        assert score(**{name: None}) == -1, name
        assert b"null pointer" in hip_lib.edgedict_last_error(), name
    for kw, word in ((dict(N=0), b"N = 0"), (dict(N=33), b"N = 33"), (dict(U=1024), b"1023"), (dict(U=-1), b"U >= 0"),
                     (dict(V=1), b"V = 1"), (dict(blank=16), b"blank"), (dict(blank=-1), b"blank"),
                     (dict(dtype=7), b"dtype"), (dict(ws=odd), b"16-byte aligned")):
        assert score(**kw) == -1, kw
        assert word in hip_lib.edgedict_last_error(), kw
        assert b"ctc_score_nbest" in hip_lib.edgedict_last_error(), kw
    # U = 0 with null hyps, and a null n_hyp, pass the pointer test - the next complaint is the workspace's
    assert score(U=0, hyps=None, nh=None, ws=odd) == -1
    assert b"16-byte aligned" in hip_lib.edgedict_last_error()
    assert score(nh=None, ws=odd) == -1
    assert b"16-byte aligned" in hip_lib.edgedict_last_error()


def test_ctc_score_nbest_refuses_cpu_tensors_and_bad_inputs():
    from edgedict_amd.loss import ctc_score_nbest
    z = torch.zeros(2, 5, 8)
    al = torch.tensor([5, 4], dtype=torch.int32)
    hyps = torch.ones(2, 3, 4, dtype=torch.int32)
    hl = torch.full((2, 3), 2, dtype=torch.int32)
    nh = torch.tensor([3, 1], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ctc_score_nbest(z, al, hyps, hl, nh)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ctc_score_nbest(z, al, hyps, hl)
    with pytest.raises(TypeError, match="float32 or bfloat16"):
        ctc_score_nbest(z.double(), al, hyps, hl, nh)
    for name, args in (("act_lens", (z, al.long(), hyps, hl, nh)), ("hyps", (z, al, hyps.long(), hl, nh)),
                       ("hyp_lens", (z, al, hyps, hl.long(), nh)), ("n_hyp", (z, al, hyps, hl, nh.long()))):
        with pytest.raises(TypeError, match="%s must be int32" % name):
            ctc_score_nbest(*args)
    with pytest.raises(ValueError, match="3 dimensions \\[B,T,V\\]"):
        ctc_score_nbest(z[0], al, hyps, hl, nh)
    with pytest.raises(ValueError, match="3 dimensions \\[B,N,U\\]"):
        ctc_score_nbest(z, al, hyps[:, 0].contiguous(), hl, nh)
    with pytest.raises(ValueError, match="2 dimensions"):
        ctc_score_nbest(z, al, hyps, hl[:, 0].contiguous(), nh)
    with pytest.raises(ValueError, match="contiguous"):
        ctc_score_nbest(z.transpose(1, 2), al, hyps, hl, nh)
    with pytest.raises(ValueError, match="contiguous"):
        ctc_score_nbest(z, al, hyps.transpose(1, 2), hl, nh)
    with pytest.raises(ValueError, match="length per example"):
        ctc_score_nbest(z, al[:1], hyps, hl, nh)
    with pytest.raises(ValueError, match="hypothesis length per slot"):
        ctc_score_nbest(z, al, hyps, hl[:, :2].contiguous(), nh)
    with pytest.raises(ValueError, match="hypothesis count per example"):
        ctc_score_nbest(z, al, hyps, hl, nh[:1])
    with pytest.raises(ValueError, match="outside \\[1, 32\\]"):
        ctc_score_nbest(z, al, torch.ones(2, 33, 4, dtype=torch.int32), torch.ones(2, 33, dtype=torch.int32))
    with pytest.raises(ValueError, match="outside \\[1, 32\\]"):
        ctc_score_nbest(z, al, torch.ones(2, 0, 4, dtype=torch.int32), torch.ones(2, 0, dtype=torch.int32))
    with pytest.raises(ValueError, match="1023"):
        ctc_score_nbest(z, al, torch.ones(2, 1, 1024, dtype=torch.int32), torch.ones(2, 1, dtype=torch.int32))
    with pytest.raises(ValueError, match="blank"):
        ctc_score_nbest(z, al, hyps, hl, nh, blank=8)
