"""CPU: the host side of MWER training.  The float64 oracle tests/mwer_ref.py that the GPU tests compare the risk kernel
against is pinned here on torch's float64 autograd and on central differences; the list packer, every argument error
(raised before the device is touched) and the native entry point's argument checks are exercised without a device."""
import ctypes

import numpy as np
import pytest
import torch

import mwer_ref as MR

_KW = dict(vocab_embed_size=8, vocab_size=12, input_size=16, enc_hidden_size=16, enc_layers=2, enc_dropout=0.0,
           enc_proj_size=12, dec_hidden_size=8, dec_layers=1, dec_dropout=0.0, dec_proj_size=8, joint_size=16)


def _case(seed, B, N, spread=3.0, max_err=9):
    rng = np.random.default_rng(seed)
    costs = rng.uniform(1.0, 1.0 + spread, size=(B, N))
    errs = rng.integers(0, max_err + 1, size=(B, N))
    return costs, errs


def _torch_risk(costs, errs, live):
    """(risk [B], d risk_b / d costs [B, N]) by torch float64 autograd of (softmax(-c) * e).sum() over the live slots."""
    B, N = costs.shape
    risk, grad = np.zeros(B), np.zeros((B, N))
    for b in range(B):
        idx = np.nonzero(live[b])[0]
        if idx.size == 0:
            continue
        c = torch.tensor(costs[b, idx], dtype=torch.float64, requires_grad=True)
        e = torch.tensor(errs[b, idx], dtype=torch.float64)
        r = (torch.softmax(-c, 0) * e).sum()
        r.backward()
        risk[b], grad[b, idx] = r.item(), c.grad.numpy()
    return risk, grad


def test_oracle_equals_torch_float64_autograd():
    for seed, (B, N) in enumerate([(1, 1), (3, 5), (4, 32)]):
        costs, errs = _case(seed, B, N)
        n_hyp = np.random.default_rng(seed + 10).integers(0, N + 1, size=B)
        costs[0, N // 2] = np.inf
        live = MR.live_mask(costs, n_hyp)
        risk, post, coef = MR.risk(costs, errs, n_hyp)
        want_risk, want_grad = _torch_risk(costs, errs, live)
        np.testing.assert_allclose(risk, want_risk, rtol=1e-14, atol=1e-15)
        np.testing.assert_allclose(coef, want_grad, rtol=1e-12, atol=1e-15)
        assert (post[~live] == 0).all() and (coef[~live] == 0).all()
        rows = live.any(1)
        np.testing.assert_allclose(post.sum(1)[rows], 1.0, rtol=1e-15)
        assert (risk[~rows] == 0).all()
        # the scale multiplies the coefficients and nothing else
        r2, p2, c2 = MR.risk(costs, errs, n_hyp, scale=0.25)
        assert np.array_equal(r2, risk) and np.array_equal(p2, post)
        np.testing.assert_allclose(c2, 0.25 * coef, rtol=1e-15)


def test_oracle_equals_central_differences():
    costs, errs = _case(3, 3, 6)
    costs[1, 2] = np.inf
    _, _, coef = MR.risk(costs, errs)
    h = 1e-6
    for b in range(3):
        for n in range(6):
            if np.isinf(costs[b, n]):
                continue
            up, dn = costs.copy(), costs.copy()
            up[b, n] += h
            dn[b, n] -= h
            fd = (MR.risk(up, errs)[0][b] - MR.risk(dn, errs)[0][b]) / (2 * h)
            assert abs(fd - coef[b, n]) <= 1e-8 * max(1.0, abs(coef[b, n])), (b, n)


def test_oracle_properties():
    costs, errs = _case(4, 5, 7)
    risk, post, coef = MR.risk(costs, errs)
    # adding a constant to an utterance's costs changes nothing
    shifted = costs + np.array([0.0, 5.0, -3.0, 100.0, 1e3])[:, None]
    r2, p2, c2 = MR.risk(shifted, errs)
    np.testing.assert_allclose(r2, risk, rtol=1e-12)
    np.testing.assert_allclose(p2, post, rtol=1e-11)
    np.testing.assert_allclose(c2, coef, rtol=1e-10, atol=1e-13)
    # the coefficients of an utterance sum to zero: the posterior is normalised
    assert np.abs(coef.sum(1)).max() <= 1e-15 * errs.max()
    # one hypothesis: nothing to move
    r1, p1, c1 = MR.risk(costs[:, :1], errs[:, :1])
    assert (c1 == 0).all() and (p1 == 1).all() and np.array_equal(r1, errs[:, 0].astype(np.float64))
    # equal errors: the risk is that count whatever the costs are
    same = np.full_like(errs, 4)
    rs, _, cs = MR.risk(costs, same)
    np.testing.assert_allclose(rs, 4.0, rtol=1e-15)
    assert np.abs(cs).max() <= 4 * 2e-16
    # a +inf entry weighs nothing: the result is that of the list without it
    holed = costs.copy()
    holed[:, 3] = np.inf
    rh, ph, ch = MR.risk(holed, errs)
    keep = [0, 1, 2, 4, 5, 6]
    rk, pk, ck = MR.risk(costs[:, keep], errs[:, keep])
    assert np.array_equal(rh, rk) and np.array_equal(ph[:, keep], pk) and np.array_equal(ch[:, keep], ck)
    assert (ph[:, 3] == 0).all() and (ch[:, 3] == 0).all()
    # costs 1e4 apart: no overflow, the cheap hypothesis takes everything
    far = np.array([[1e4, 0.0, 2e4]])
    rf, pf, cf = MR.risk(far, np.array([[3, 1, 7]]))
    assert rf[0] == 1.0 and pf.tolist() == [[0.0, 1.0, 0.0]] and (cf == 0).all()
    assert MR.reduced([1.0, 2.0], 0.5) == 1.5
    assert MR.reduced([1.0, 2.0], 0.5, 0.25, [4.0, 8.0]) == 3.0


def test_rows_layout_deduplication_empty_list_and_reference_rows():
    from edgedict_amd import loss
    ys = np.array([[5, 6, 7], [8, 0, 0], [9, 9, 0]])
    ylen = np.array([3, 1, 2])
    lists = [[[5, 6], [5, 6, 7, 7], [5, 6]], [], [np.array([9, 9]), np.array([9, 9])]]
    for with_ref in (False, True):
        rows = loss.mwer_rows(lists, ys, ylen, with_ref)
        assert (rows.B, rows.N, rows.Rh, rows.Uh, rows.Ur) == (3, 2, 4, 4, 3)
        assert rows.R == (7 if with_ref else 4) and rows.Umax == 4
        assert rows.host.dtype == np.int32 and rows.host.ndim == 1 and rows.host.size == rows.size()
        v = rows.views()
        # one buffer, the arrays back to back in the documented order
        sizes = [v[k].size for k in ("labels", "label_lens", "row_utt", "row_slot", "row_dense", "hyps", "hyp_lens",
                                     "n_hyp", "refs", "ref_lens")]
        assert sum(sizes) == rows.host.size and list(v) == ["labels", "label_lens", "row_utt", "row_slot", "row_dense",
                                                           "hyps", "hyp_lens", "n_hyp", "refs", "ref_lens"]
        assert all(np.shares_memory(a, rows.host) for a in v.values())
        assert [[t.tolist() for t in own] for own in rows.lists] == [[[5, 6], [5, 6, 7, 7]], [[]], [[9, 9]]]
        assert v["n_hyp"].tolist() == [2, 1, 1]
        assert v["hyps"].shape == (3, 2, 4) and v["hyps"][0].tolist() == [[5, 6, 0, 0], [5, 6, 7, 7]]
        assert v["hyp_lens"].tolist() == [[2, 4], [0, 0], [2, 0]]
        assert v["refs"].tolist() == [[5, 6, 7], [8, 0, 0], [9, 9, 0]] and v["ref_lens"].tolist() == [3, 1, 2]
        assert v["labels"][:4].tolist() == [[5, 6, 0, 0], [5, 6, 7, 7], [0, 0, 0, 0], [9, 9, 0, 0]]
        assert v["label_lens"][:4].tolist() == [2, 4, 0, 2]
        assert v["row_utt"][:4].tolist() == [0, 0, 1, 2] and v["row_slot"][:4].tolist() == [0, 1, 0, 0]
        assert v["row_dense"][:4].tolist() == [0, 1, 2, 4]
        if with_ref:
            assert v["labels"][4:].tolist() == [[5, 6, 7, 0], [8, 0, 0, 0], [9, 9, 0, 0]]
            assert v["label_lens"][4:].tolist() == [3, 1, 2] and v["row_utt"][4:].tolist() == [0, 1, 2]
            assert v["row_slot"][4:].tolist() == [-1, -1, -1] and v["row_dense"][4:].tolist() == [-1, -1, -1]
        # the same views of a tensor copy of the buffer (what the device side works on)
        tv = rows.views(torch.from_numpy(rows.host.copy()))
        assert all(tuple(tv[k].shape) == v[k].shape and np.array_equal(tv[k].numpy(), v[k]) for k in v)
    # torch inputs, a reference longer than every hypothesis counts only with reference rows
    rows = loss.mwer_rows([[[1]]], torch.tensor([[1, 2, 3]], dtype=torch.int32), torch.tensor([3], dtype=torch.int32), False)
    assert (rows.Umax, rows.Ur, rows.R) == (1, 3, 1)
    assert loss.mwer_rows([[[1]]], torch.tensor([[1, 2, 3]]), torch.tensor([3]), True).Umax == 3
    # all hypotheses empty: the label matrix keeps one column
    rows = loss.mwer_rows([[], [[]]], np.zeros((2, 0), dtype=np.int64), np.array([0, 0]), False)
    assert (rows.Umax, rows.Uh, rows.Ur, rows.N, rows.R) == (1, 0, 0, 1, 2)


def test_rows_refuse_33_sequences_and_bad_input():
    from edgedict_amd import loss
    ys, ylen = np.array([[1, 2]]), np.array([2])
    many = [[k] for k in range(33)]
    with pytest.raises(ValueError, match="33 distinct hypotheses"):
        loss.mwer_rows([many], ys, ylen, False)
    assert loss.mwer_rows([many[:32] + many[:5]], ys, ylen, False).N == 32         # duplicates do not count
    with pytest.raises(ValueError, match="2 lists for 1 references"):
        loss.mwer_rows([[], []], ys, ylen, False)
    with pytest.raises(ValueError, match="one length per row"):
        loss.mwer_rows([[]], ys, np.array([2, 2]), False)
    with pytest.raises(TypeError, match="integers"):
        loss.mwer_rows([[[0.5]]], ys, ylen, False)
    with pytest.raises(ValueError, match="1023"):
        loss.mwer_rows([[np.zeros(1024, dtype=np.int64)]], ys, ylen, False)


def test_mwer_risk_and_loss_refuse_cpu_tensors_and_bad_inputs():
    from edgedict_amd.loss import MWERLoss, mwer_risk
    costs = torch.ones(2, 3)
    errs = torch.ones(2, 3, dtype=torch.int32)
    errs4 = torch.ones(2, 3, 4, dtype=torch.int32)
    nh = torch.tensor([3, 1], dtype=torch.int32)
    ref = torch.ones(2)
    for e in (errs, errs4):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            mwer_risk(costs, e, nh)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            MWERLoss(0.5)(costs, e, None, ref)
    with pytest.raises(TypeError, match="costs must be float32"):
        mwer_risk(costs.double(), errs)
    with pytest.raises(TypeError, match="errs must be int32"):
        mwer_risk(costs, errs.long())
    with pytest.raises(TypeError, match="n_hyp must be int32"):
        mwer_risk(costs, errs, nh.long())
    with pytest.raises(TypeError, match="ref_costs must be float32"):
        MWERLoss(0.5)(costs, errs, nh, ref.double())
    with pytest.raises(TypeError, match="must be a tensor"):
        mwer_risk(costs.numpy(), errs)
    with pytest.raises(ValueError, match="contiguous"):
        mwer_risk(torch.ones(3, 2).t(), errs)
    with pytest.raises(ValueError, match="contiguous"):
        mwer_risk(costs, torch.ones(3, 2, dtype=torch.int32).t())
    with pytest.raises(ValueError, match="contiguous"):
        mwer_risk(costs, errs4[:, :, 0])                     # a strided view of the counts: pass the [B,N,4] itself
    with pytest.raises(ValueError, match="2 dimensions \\[B,N\\]"):
        mwer_risk(costs[0], errs)
    with pytest.raises(ValueError, match="\\[B,N,4\\]"):
        mwer_risk(costs, errs[0])
    with pytest.raises(ValueError, match="1 dimension"):
        mwer_risk(costs, errs, nh.unsqueeze(1))
    with pytest.raises(ValueError, match="1 dimension"):
        MWERLoss(0.5)(costs, errs, nh, ref.unsqueeze(1))
    with pytest.raises(ValueError, match="error count per slot"):
        mwer_risk(costs, errs[:, :2].contiguous())
    with pytest.raises(ValueError, match="error count per slot"):
        mwer_risk(costs, torch.ones(2, 3, 3, dtype=torch.int32))
    with pytest.raises(ValueError, match="hypothesis count per example"):
        mwer_risk(costs, errs, nh[:1])
    with pytest.raises(ValueError, match="reference cost per example"):
        MWERLoss(0.5)(costs, errs, nh, ref[:1])
    with pytest.raises(ValueError, match="at least one utterance"):
        mwer_risk(torch.ones(0, 3), torch.ones(0, 3, dtype=torch.int32))
    with pytest.raises(ValueError, match="outside \\[1, 32\\]"):
        mwer_risk(torch.ones(2, 33), torch.ones(2, 33, dtype=torch.int32))
    with pytest.raises(ValueError, match="outside \\[1, 32\\]"):
        mwer_risk(torch.ones(2, 0), torch.ones(2, 0, dtype=torch.int32))
    with pytest.raises(ValueError, match="needs ref_costs"):
        MWERLoss(0.5)(costs, errs, nh)
    with pytest.raises(ValueError, match="nll_weight"):
        MWERLoss(-1.0)
    with pytest.raises(ValueError, match="nll_weight"):
        MWERLoss(float("nan"))
    with pytest.raises(ValueError, match="reduction"):
        MWERLoss(0.0, "average")


def test_mwer_loss_refuses_bad_arguments_before_the_device():
    from edgedict_amd.models import Transducer
    m = Transducer(**_KW)
    xs, ys = torch.zeros(1, 4, 16), torch.ones(1, 2, dtype=torch.int32)
    xlen, ylen = torch.tensor([4], dtype=torch.int32), torch.tensor([2], dtype=torch.int32)
    with pytest.raises(ValueError, match="search must be one of sync_beam, beam"):
        m.mwer_loss(xs, ys, xlen, ylen, search="nonsense")
    with pytest.raises(ValueError, match="nll_weight"):
        m.mwer_loss(xs, ys, xlen, ylen, nll_weight=-0.5)
    with pytest.raises(ValueError, match="device batch"):
        m.mwer_loss(xs, ys, xlen, ylen)
    assert m.last_mwer is None


def test_packed_joint_row_costs_refuse_windows_and_fastemit():
    from edgedict_amd.models import _JointLossFn
    enc, dec = torch.zeros(1, 2, 4), torch.zeros(1, 2, 4)
    w1, b1, w2, b2 = torch.zeros(3, 8), torch.zeros(3), torch.zeros(5, 3), torch.zeros(5)
    labels = torch.ones(1, 1, dtype=torch.int32)
    al, ll = torch.tensor([2], dtype=torch.int32), torch.tensor([1], dtype=torch.int32)
    with pytest.raises(ValueError, match="no windows, no band plan and no FastEmit"):
        _JointLossFn.apply(enc, dec, w1, b1, w2, b2, labels, al, ll, 0, torch.float32, 0.5, None, None, None, True)
    with pytest.raises(ValueError, match="no windows, no band plan and no FastEmit"):
        _JointLossFn.apply(enc, dec, w1, b1, w2, b2, labels, al, ll, 0, torch.float32, 0.0, labels, labels, None, True)
    with pytest.raises(ValueError, match="Input length mismatch"):
        _JointLossFn.apply(enc, dec, w1, b1, w2, b2, labels, al + 1, ll, 0, torch.float32, 0.0, None, None, None, True)


def test_new_symbol_is_declared_and_exported(hip_lib):
    from edgedict_amd import _lib, loss
    from edgedict_amd.models import Transducer
    from edgedict_amd.trainer import TrainEngine
    assert "edgedict_mwer_risk" in _lib.declared_symbols()
    assert hasattr(hip_lib, "edgedict_mwer_risk")
    assert hip_lib.edgedict_abi_version() == 2
    for name in ("mwer_risk", "MWERLoss", "mwer_rows", "MWERRows", "MWER_MAX_N"):
        assert hasattr(loss, name), name
    assert loss.MWER_MAX_N == 32
    assert callable(Transducer.mwer_loss) and callable(TrainEngine.mwer_step)


def test_native_argument_errors_are_raised_before_any_launch(hip_lib):
    """B < 1, N outside [1, 32], an err stride other than 1 or 4, B * N above the grid limit, a needed pointer that is
    null: -1 with a message, no device needed.  (That n_hyp, ref_costs and reduced may be null takes a launch to show:
    test_mwer_gpu.py.)"""
    buf = ctypes.create_string_buffer(128)
    fake = ctypes.addressof(buf)

    def risk(costs=fake, errs=fake, stride=1, nh=fake, ref=fake, B=2, N=2, risk=fake, post=fake, coef=fake, red=fake):
        return hip_lib.edgedict_mwer_risk(costs, errs, stride, nh, ref, B, N, 0.5, 1.0, risk, post, coef, red, None)

    for kw, word in ((dict(B=0), b"B must be positive"), (dict(B=-1), b"B must be positive"), (dict(N=0), b"N = 0"),
                     (dict(N=33), b"N = 33"), (dict(stride=0), b"err_stride = 0"), (dict(stride=2), b"err_stride = 2"),
                     (dict(stride=8), b"err_stride = 8"), (dict(B=1 << 30, N=32), b"exceeds the grid")):
        assert risk(**kw) == -1, kw
        assert word in hip_lib.edgedict_last_error(), kw
        assert b"mwer_risk" in hip_lib.edgedict_last_error(), kw
    for name in ("costs", "errs", "risk", "post", "coef"):
        assert risk(**{name: None}) == -1, name
        assert b"null pointer" in hip_lib.edgedict_last_error(), name
