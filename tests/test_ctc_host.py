"""CPU: the CTC head's host side.  The float64 restatement tests/ctc_ref.py that the GPU tests compare against is pinned
here - against the enumeration of all V^T paths and against torch.nn.functional.ctc_loss in float64 - and every argument
error is raised before anything is launched."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import ctc_ref as CR

_KW = dict(vocab_embed_size=8, vocab_size=12, input_size=16, enc_hidden_size=16, enc_layers=2, enc_dropout=0.0,
           enc_proj_size=12, dec_hidden_size=8, dec_layers=1, dec_dropout=0.0, dec_proj_size=8, joint_size=16)


def _collapse(path, blank):
    out, prev = [], None
    for k in path:
        if k != blank and k != prev:
            out.append(k)
        prev = k
    return out


def _brute(logits, y, blank=0):
    """-log of the summed probability of every length-T path that collapses to y, and its gradient, path by path."""
    lp = CR.log_softmax(logits)
    T, V = lp.shape
    total = 0.0
    counts = np.zeros((T, V))                       # sum over matching paths of p(path) [path_t == v]
    for path in itertools.product(range(V), repeat=T):
        if _collapse(path, blank) != list(y):
            continue
        p = np.exp(sum(lp[t, k] for t, k in enumerate(path)))
        total += p
        for t, k in enumerate(path):
            counts[t, k] += p
    if total == 0.0:
        return np.inf, np.zeros((T, V))
    return -np.log(total), np.exp(lp) - counts / total


_TRANSCRIPTS = [[], [1], [1, 1], [2, 2, 1], [1, 1, 1], [1, 2], [3, 1, 3], [2, 1, 1, 2]]


def test_restatement_equals_the_enumeration_of_all_paths():
    """Lattices up to T = 6, V = 4: cost and gradient to 1e-12, T = U + repeats exactly included; the occupancies of a
    frame sum to 1 and sit on live states only."""
    rng = np.random.default_rng(0)
    exact = 0
    for y in _TRANSCRIPTS:
        need = len(y) + CR.repeats(y)
        for T in range(max(1, need), 7):
            for V in ((4,) if T == 6 else (3, 4)):
                if y and max(y) >= V:
                    continue
                z = 2.0 * rng.normal(size=(T, V))
                cost, grad, occ, alpha, beta = CR.ctc_one(z, y)
                want, want_g = _brute(z, y)
                exact += T == need
                assert np.isfinite(want)
                assert abs(cost - want) <= 1e-12 * max(1.0, abs(want)), (y, T, V)
                assert np.abs(grad - want_g).max() <= 1e-12, (y, T, V)
                assert np.abs(occ.sum(-1) - 1.0).max() <= 1e-12
                assert not occ[~(np.isfinite(alpha) & np.isfinite(beta))].any()
    assert exact >= len(_TRANSCRIPTS)


def test_restatement_equals_torch_ctc_loss_in_float64():
    """A ragged batch with empty transcripts and adjacent repeats: costs and the gradient through log_softmax, to 1e-10."""
    rng = np.random.default_rng(1)
    B, T, U, V = 6, 11, 5, 7
    z = rng.normal(size=(B, T, V)) * 2.0
    labels = rng.integers(1, 4, size=(B, U))
    labels[0] = [2, 2, 2, 1, 1]
    act = np.array([11, 9, 1, 7, 11, 10])
    lab = np.array([5, 3, 0, 4, 0, 5])
    costs, grads, _, _ = CR.ctc_batch(z, labels, act, lab)
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    lp = torch.log_softmax(zt, -1).transpose(0, 1)
    tc = torch.nn.functional.ctc_loss(lp, torch.tensor(labels), torch.tensor(act), torch.tensor(lab), blank=0,
                                      reduction="none")
    tc.sum().backward()
    assert np.isfinite(costs).all()
    assert np.abs(costs - tc.detach().numpy()).max() <= 1e-10
    assert np.abs(grads - zt.grad.numpy()).max() <= 1e-10
    for b in range(B):
        assert not grads[b, act[b]:].any()


def test_infeasible_row_is_inf_with_a_zero_gradient():
    rng = np.random.default_rng(2)
    y = [1, 1, 2, 2]                                  # needs 4 + 2 frames
    z = rng.normal(size=(5, 4))
    cost, grad, occ, _, _ = CR.ctc_one(z, y)
    assert cost == np.inf and not grad.any() and not occ.any()
    assert np.isfinite(CR.ctc_one(rng.normal(size=(6, 4)), y)[0])
    costs, grads, _, lives = CR.ctc_batch(rng.normal(size=(2, 6, 4)), np.array([y, y]), [6, 5], [4, 4])
    assert np.isfinite(costs[0]) and costs[1] == np.inf
    assert grads[0].any() and not grads[1].any() and not lives[1].any()


def test_greedy_restatement_collapses_repeats_and_blanks():
    z = np.full((1, 7, 3), -1.0)
    for t, k in enumerate([0, 1, 1, 0, 1, 2, 2]):
        z[0, t, k] = 1.0
    (toks, frames, nl), = CR.greedy(z, [7])
    assert toks.tolist() == [1, 1, 2] and frames.tolist() == [1, 4, 5]
    assert abs(nl + 3 * CR.log_softmax(z[0, 0])[0]) <= 1e-12
    (toks, _, _), = CR.greedy(np.zeros((1, 4, 3)), [4])   # ties: the lowest index, here the blank
    assert toks.size == 0


def test_new_symbols_are_declared_and_exported(hip_lib):
    from edgedict_amd import _lib
    want = {"edgedict_ctc_workspace_bytes", "edgedict_ctc_workspace_view", "edgedict_ctc_loss_forward",
            "edgedict_ctc_loss_backward", "edgedict_ctc_greedy"}
    assert want <= set(_lib.declared_symbols())
    for name in want:
        assert hasattr(hip_lib, name), name
    assert hip_lib.edgedict_abi_version() == 2
    assert hip_lib.edgedict_ctc_workspace_bytes(0, 5, 3) == 0
    n = hip_lib.edgedict_ctc_workspace_bytes(2, 5, 3)
    assert n >= 2 * 2 * 5 * 7 * 8 and n % 256 == 0
    assert hip_lib.edgedict_ctc_workspace_bytes(2, 5, 0) > 0


def test_argument_errors_are_raised_before_any_launch(hip_lib):
    """Null pointers, U = 2000, V < 2, blank out of range, a bad dtype code: -1 with a message, no device needed."""
    f = ctypes.c_float
    buf = ctypes.create_string_buffer(64)
    fake = ctypes.cast(buf, ctypes.c_void_p)

    def fwd(logits=fake, dtype=0, labels=fake, al=fake, ll=fake, U=3, V=16, blank=0, costs=fake, ws=fake):
        return hip_lib.edgedict_ctc_loss_forward(logits, dtype, labels, al, ll, 2, 5, U, V, blank, 0, costs, None, f(1.0),
                                                 ws, None)

    def bwd(logits=fake, dtype=0, grads=fake, labels=fake, al=fake, ll=fake, U=3, V=16, blank=0, ws=fake):
        return hip_lib.edgedict_ctc_loss_backward(logits, dtype, grads, labels, al, ll, 2, 5, U, V, blank, ws, f(1.0),
                                                  None, 0, None)

    def greedy(logits=fake, dtype=0, al=fake, V=16, blank=0, tokens=fake, scratch=fake):
        return hip_lib.edgedict_ctc_greedy(logits, dtype, al, 2, 5, V, blank, tokens, fake, fake, fake, scratch, None)

    for fn, nulls in ((fwd, ("logits", "labels", "al", "ll", "costs", "ws")),
                      (bwd, ("logits", "grads", "labels", "al", "ll", "ws")),
                      (greedy, ("logits", "al", "tokens", "scratch"))):
        for name in nulls:
            assert fn(**{name: None}) == -1, (fn.__name__, name)
            assert b"null pointer" in hip_lib.edgedict_last_error(), (fn.__name__, name)
        for kw, word in ((dict(V=1), b"V = 1"), (dict(blank=16), b"blank"), (dict(blank=-1), b"blank"),
                         (dict(dtype=7), b"dtype")):
            assert fn(**kw) == -1, (fn.__name__, kw)
            assert word in hip_lib.edgedict_last_error(), (fn.__name__, kw)
    for fn in (fwd, bwd):
        assert fn(U=2000) == -1
        assert b"1023" in hip_lib.edgedict_last_error()
        assert fn(U=-1) == -1


def test_ctc_loss_refuses_cpu_tensors_and_bad_inputs():
    from edgedict_amd.loss import CTCLoss, ctc_greedy
    z = torch.zeros(2, 5, 8)
    labels = torch.ones(2, 3, dtype=torch.int32)
    al = torch.tensor([5, 4], dtype=torch.int32)
    ll = torch.tensor([3, 2], dtype=torch.int32)
    fn = CTCLoss()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fn(z, labels, al, ll)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ctc_greedy(z, al)
    with pytest.raises(TypeError, match="float32 or bfloat16"):
        fn(z.double(), labels, al, ll)
    with pytest.raises(TypeError, match="labels must be int32"):
        fn(z, labels.long(), al, ll)
    with pytest.raises(TypeError, match="act_lens must be int32"):
        fn(z, labels, al.long(), ll)
    with pytest.raises(ValueError, match="3 dimensions"):
        fn(z[0], labels, al, ll)
    with pytest.raises(ValueError, match="2 dimensions"):
        fn(z, labels[0], al, ll)
    with pytest.raises(ValueError, match="contiguous"):
        fn(z.transpose(1, 2), labels, al, ll)
    with pytest.raises(ValueError, match="length per example"):
        fn(z, labels, al[:1], ll)
    with pytest.raises(ValueError, match="label length per example"):
        fn(z, labels, al, ll[:1])
    with pytest.raises(ValueError, match="Input length mismatch"):
        fn(z, labels, al - 1, ll)
    with pytest.raises(ValueError, match="Output length mismatch"):
        fn(z, labels, al, ll - 1)
    with pytest.raises(ValueError, match="reduction"):
        CTCLoss(reduction="batchmean")
    with pytest.raises(TypeError, match="act_lens must be int32"):
        ctc_greedy(z, al.long())


def test_transducer_head_exists_iff_ctc_weight_is_positive():
    from edgedict_amd.models import Transducer
    plain = Transducer(**_KW)
    keys = list(plain.state_dict().keys())
    assert not hasattr(plain, "ctc_head") and plain.ctc_weight == 0.0
    assert not any("ctc" in k for k in keys)
    assert list(Transducer(**_KW, ctc_weight=0.0).state_dict().keys()) == keys
    with_head = Transducer(**_KW, ctc_weight=0.3)
    assert with_head.ctc_weight == 0.3
    assert list(with_head.state_dict().keys()) == keys + ["ctc_head.weight", "ctc_head.bias"]
    assert tuple(with_head.ctc_head.weight.shape) == (12, 12) and tuple(with_head.ctc_head.bias.shape) == (12,)
    assert [n for n, _ in with_head.named_parameters()][-2:] == ["ctc_head.weight", "ctc_head.bias"]
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="ctc_weight"):
            Transducer(**_KW, ctc_weight=bad)
    with pytest.raises(RuntimeError, match="no CTC head"):
        plain.ctc_greedy_decode(torch.zeros(1, 4, 16), torch.tensor([4]))
