"""CPU: the CTC forced aligner's host side.  The float64 restatement tests/ctc_align_ref.py that the GPU tests compare
against is pinned here - against the enumeration of all V^T paths, and its tie rule on constant log-probabilities - and
every argument error is raised before anything is launched."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import ctc_align_ref as AR
import ctc_ref as CR

_KW = dict(vocab_embed_size=8, vocab_size=12, input_size=16, enc_hidden_size=16, enc_layers=2, enc_dropout=0.0,
           enc_proj_size=12, dec_hidden_size=8, dec_layers=1, dec_dropout=0.0, dec_proj_size=8, joint_size=16)


def _collapse(path, blank=0):
    out, prev = [], None
    for k in path:
        if k != blank and k != prev:
            out.append(k)
        prev = k
    return out


def _brute_best(logits, y, blank=0):
    """The best log-probability among all length-T paths that collapse to y (-inf: none does)."""
    lp = CR.log_softmax(logits)
    T, V = lp.shape
    best = -np.inf
    for path in itertools.product(range(V), repeat=T):
        if _collapse(path, blank) == list(y):
            best = max(best, sum(lp[t, k] for t, k in enumerate(path)))
    return best


_TRANSCRIPTS = [[], [1], [1, 1], [2, 2, 1], [1, 1, 1], [1, 2], [2, 1, 2], [1, 2, 2]]


def test_reference_equals_the_enumeration_of_all_paths():
    """T <= 5, V = 3, U <= 3, with repeats and infeasible cases: the score is the best path's to 1e-12; the returned
    path collapses to the transcript, re-scores to the score, and its spans are those of its state sequence."""
    rng = np.random.default_rng(0)
    feasible = infeasible = 0
    for y in _TRANSCRIPTS:
        need = len(y) + CR.repeats(y)
        for T in range(1, 6):
            z = 2.0 * rng.normal(size=(T, 3))
            frames, ends, score, v, states = AR.align_one(z, y)
            want = _brute_best(z, y)
            if T < need:
                infeasible += 1
                assert want == -np.inf and score == -np.inf, (y, T)
                assert (frames == -1).all() and (ends == -1).all() and (states == -1).all()
                continue
            feasible += 1
            assert np.isfinite(want) and abs(score - want) <= 1e-12 * max(1.0, abs(want)), (y, T)
            assert _collapse(AR.path_symbols(states, y)) == y, (y, T)
            assert abs(AR.rescore(z, states, y) - score) <= 1e-12 * max(1.0, abs(score)), (y, T)
            assert (AR.states_from_spans(frames, ends, T) == states).all(), (y, T)
            assert states[0] in (0, 1) and (np.diff(states) >= 0).all() and (np.diff(states) <= 2).all()
    assert feasible >= 25 and infeasible >= 8


def test_replay_equals_the_logits_form_and_widens_float32_planes():
    rng = np.random.default_rng(1)
    y = [1, 1, 2, 3, 3]
    z = rng.normal(size=(11, 5))
    lp = CR.log_softmax(z)
    a = AR.align_one(z, y)
    b = AR.replay(lp[:, 0], lp[:, y], y)
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and a[2] == b[2] and np.array_equal(a[3], b[3])
    lp32 = lp.astype(np.float32)
    c = AR.replay(lp32[:, 0], lp32[:, y], y)
    d = AR.replay(lp32[:, 0].astype(np.float64), lp32[:, y].astype(np.float64), y)
    assert c[2] == d[2] and np.array_equal(c[3], d[3]) and c[3].dtype == np.float64


@pytest.mark.parametrize("y,T,want", [([1, 2, 3, 1], 9, [5, 6, 7, 8]), ([1, 1, 2, 2], 9, [3, 5, 6, 8]),
                                      ([1, 1, 2, 2], 6, [0, 2, 3, 5]), ([1, 1, 2, 2], 5, None)],
                         ids=["distinct", "repeats", "forced", "infeasible"])
def test_tie_rule_on_constant_log_probabilities(y, T, want):
    """All paths score equal: the later emission wins, every label lasts one frame."""
    frames, ends, score, _, _ = AR.align_one(np.zeros((T, 4)), y)
    if want is None:
        assert score == -np.inf and (frames == -1).all() and (ends == -1).all()
        return
    assert frames.tolist() == want and ends.tolist() == want
    assert abs(score - T * np.log(0.25)) <= 1e-12


def test_batch_form_pads_and_keeps_rows_apart():
    rng = np.random.default_rng(2)
    z = rng.normal(size=(3, 7, 4))
    labels = np.array([[1, 1, 2], [2, 3, 1], [1, 1, 1]])
    frames, ends, scores, states = AR.align_batch(z, labels, [7, 5, 4], [3, 2, 3])
    assert np.isfinite(scores[:2]).all() and scores[2] == -np.inf          # row 2 needs 5 frames, has 4
    assert (frames[2] == -1).all() and (ends[2] == -1).all()
    assert frames[1, 2] == -1 and ends[1, 2] == -1 and (frames[1, :2] >= 0).all()
    one = AR.align_one(z[1, :5], [2, 3])
    assert (frames[1, :2] == one[0]).all() and scores[1] == one[2] and len(states[1]) == 5
    assert AR.align_batch(z, labels, [0, 5, 4], [3, 2, 3])[2][0] == -np.inf          # T_b = 0


def test_new_symbol_is_declared_and_exported(hip_lib):
    from edgedict_amd import _lib
    assert "edgedict_ctc_align" in _lib.declared_symbols()
    assert hasattr(hip_lib, "edgedict_ctc_align")
    assert hip_lib.edgedict_abi_version() == 2


def test_argument_errors_are_raised_before_any_launch(hip_lib):
    """Null pointers, U = 1024, blank out of range, a bad dtype code, a misaligned workspace: -1 with a message, no
    device needed; U = 0 may leave labels, frames and ends null (checked up to the pointer test that follows)."""
    buf = ctypes.create_string_buffer(128)
    fake = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    odd = ctypes.c_void_p(fake.value + 4)

    def align(logits=fake, dtype=0, labels=fake, al=fake, ll=fake, U=3, V=16, blank=0, frames=fake, ends=fake,
              scores=fake, ws=fake):
        return hip_lib.edgedict_ctc_align(logits, dtype, labels, al, ll, 2, 5, U, V, blank, frames, ends, scores, ws,
                                          None)

    for name in ("logits", "labels", "al", "ll", "frames", "ends", "scores", "ws"):
        assert align(**{name: None}) == -1, name
        assert b"null pointer" in hip_lib.edgedict_last_error(), name
    for kw, word in ((dict(U=1024), b"1023"), (dict(U=-1), b"U >= 0"), (dict(V=1), b"V = 1"), (dict(blank=16), b"blank"),
                     (dict(blank=-1), b"blank"), (dict(dtype=7), b"dtype"), (dict(ws=odd), b"16-byte aligned")):
        assert align(**kw) == -1, kw
        assert word in hip_lib.edgedict_last_error(), kw
        assert b"ctc_align" in hip_lib.edgedict_last_error(), kw
    # U = 0: null labels / frames / ends pass the pointer test - the next complaint is the workspace's
    assert align(U=0, labels=None, frames=None, ends=None, ws=odd) == -1
    assert b"16-byte aligned" in hip_lib.edgedict_last_error()
    assert align(U=0, labels=None, frames=None, ends=None, scores=None) == -1
    assert b"null pointer" in hip_lib.edgedict_last_error()


def test_ctc_align_refuses_cpu_tensors_and_bad_inputs():
    from edgedict_amd.loss import ctc_align, ctc_align_debug
    z = torch.zeros(2, 5, 8)
    labels = torch.ones(2, 3, dtype=torch.int32)
    al = torch.tensor([5, 4], dtype=torch.int32)
    ll = torch.tensor([3, 2], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ctc_align(z, labels, al, ll)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ctc_align(z, labels, al - 1, ll, check_lengths=False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ctc_align_debug(z, labels, al, ll)
    with pytest.raises(TypeError, match="float32 or bfloat16"):
        ctc_align(z.double(), labels, al, ll)
    with pytest.raises(TypeError, match="labels must be int32"):
        ctc_align(z, labels.long(), al, ll)
    with pytest.raises(TypeError, match="act_lens must be int32"):
        ctc_align(z, labels, al.long(), ll)
    with pytest.raises(TypeError, match="label_lens must be int32"):
        ctc_align(z, labels, al, ll.long())
    with pytest.raises(ValueError, match="3 dimensions"):
        ctc_align(z[0], labels, al, ll)
    with pytest.raises(ValueError, match="2 dimensions"):
        ctc_align(z, labels[0], al, ll)
    with pytest.raises(ValueError, match="contiguous"):
        ctc_align(z.transpose(1, 2), labels, al, ll)
    with pytest.raises(ValueError, match="length per example"):
        ctc_align(z, labels, al[:1], ll)
    with pytest.raises(ValueError, match="label length per example"):
        ctc_align(z, labels, al, ll[:1])
    with pytest.raises(ValueError, match="Input length mismatch"):
        ctc_align(z, labels, al - 1, ll)
    with pytest.raises(ValueError, match="Output length mismatch"):
        ctc_align(z, labels, al, ll - 1)


def test_model_without_the_head_refuses_to_align():
    from edgedict_amd.models import Transducer
    plain = Transducer(**_KW)
    args = (torch.zeros(1, 4, 16), torch.ones(1, 2, dtype=torch.int32), torch.tensor([4]), torch.tensor([2]))
    with pytest.raises(RuntimeError, match="no CTC head"):
        plain.ctc_align(*args)
    with pytest.raises(RuntimeError, match="no CTC head"):
        plain.ctc_windows(*args, 2, 2)
