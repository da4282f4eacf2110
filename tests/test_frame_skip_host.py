"""CPU: the blank-frame skipping oracle tests/frame_skip_ref.py against a brute-force loop, ``separate``, and the
argument rules of the native and Python entry points (csrc/frame_skip.hip, loss.ctc_blank_skip, decode.skip_blank_frames,
``skip_blank=`` of the beam searches): everything that needs no device."""
import ctypes
import math

import numpy as np
import pytest
import torch

import frame_skip_ref as FR

_KW = dict(vocab_embed_size=8, vocab_size=12, input_size=16, enc_hidden_size=16, enc_layers=2, enc_dropout=0.0,
           enc_proj_size=12, dec_hidden_size=8, dec_layers=1, dec_dropout=0.0, dec_proj_size=8, joint_size=16)


def _logits(seed, B, T, V, dtype=torch.float32, blank=0):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, T, V, generator=g) * 2.0
    z[:, :, blank] += torch.where(torch.rand(B, T, generator=g) < 0.5, -4.0, 6.0)
    return z.to(dtype)


# ------------------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("blank", [0, 3])
def test_oracle_equals_a_brute_force_loop(blank):
    B, T, V, thr = 3, 9, 5, 0.4
    z = _logits(1, B, T, V, blank=blank)
    act = [9, 0, 6]
    frame_map, kept, lp = FR.skip(z, act, thr, blank)
    log_thr = float(np.float32(math.log(thr)))
    for b in range(B):
        want = []
        for t in range(T):
            if t >= act[b]:
                assert lp[b, t] == 0.0
                continue
            row = [float(v) for v in z[b, t].double()]
            p = math.exp(row[blank]) / sum(math.exp(v) for v in row)
            assert abs(lp[b, t] - math.log(p)) <= 1e-12
            if math.log(p) <= log_thr:
                want.append(t)
        assert kept[b] == len(want)
        assert frame_map[b, :len(want)].tolist() == want and (frame_map[b, len(want):] == -1).all()
    assert 0 < kept[0] < 9 and kept[1] == 0
    assert frame_map.dtype == np.int32 and kept.dtype == np.int32
    enc = np.arange(B * T * 2, dtype=np.float32).reshape(B, T, 2)
    out = FR.gather(enc, frame_map, kept, int(kept.max()))
    for b in range(B):
        for j in range(int(kept.max())):
            want = enc[b, frame_map[b, j]] if j < kept[b] else np.zeros(2)
            assert (out[b, j] == want).all()


def test_threshold_one_keeps_every_frame():
    z = _logits(2, 2, 7, 4)
    z[0, 3, 0] = 80.0                       # lse - z[blank] underflows: lp_blank is exactly 0
    frame_map, kept, lp = FR.skip(z, [7, 5], 1.0)
    assert lp[0, 3] == 0.0 and (lp <= 0).all()
    assert kept.tolist() == [7, 5]
    assert frame_map[0].tolist() == list(range(7)) and frame_map[1].tolist() == [0, 1, 2, 3, 4, -1, -1]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("thr", [0.5, 0.999, 1.0])
def test_separate_terminates_and_clears_the_margin(dtype, thr):
    """Logits whose blank posterior sits ON the threshold in every frame: the blank logit solved for it."""
    B, T, V = 2, 40, 6
    z = _logits(3, B, T, V).double()
    others = torch.logsumexp(z[:, :, 1:], dim=2)
    p = min(thr, 1.0 - 1e-9)
    z[:, :, 0] = others + math.log(p / (1.0 - p))
    z = z.to(dtype)
    act = [T, 17]
    if dtype == torch.float32:
        assert FR.in_margin(z, act, thr).sum() == T + 17
    out = FR.separate(z, act, thr)
    assert out.dtype == dtype and out.shape == z.shape
    assert not FR.in_margin(out, act, thr).any()
    assert torch.equal(out[:, :, 1:], z[:, :, 1:]) and torch.equal(out[1, 17:], z[1, 17:])
    if dtype == torch.float32:
        moved = (out[:, :, 0].double() - z[:, :, 0].double()).abs()
        assert (moved[0] >= 1.0 - 1e-6).all()
    # inputs that are clear already come back unchanged
    clear = _logits(4, B, T, V).to(dtype)
    clear = FR.separate(clear, act, 0.5)
    assert torch.equal(FR.separate(clear, act, 0.5), clear)


# ------------------------------------------------------------------------------------------- the entry points
def test_new_symbols_are_declared_and_exported(hip_lib):
    from edgedict_amd import _lib
    want = {"edgedict_frame_skip_scan", "edgedict_frame_skip_gather"}
    assert want <= set(_lib.declared_symbols())
    for name in want:
        assert hasattr(hip_lib, name), name


def test_native_argument_errors_are_raised_before_any_launch(hip_lib):
    f = ctypes.c_float
    buf = ctypes.create_string_buffer(64)
    fake = ctypes.cast(buf, ctypes.c_void_p)

    def scan(logits=fake, dtype=0, al=fake, B=2, T=5, V=16, blank=0, log_thr=-0.5, lp=fake, fmap=fake, kept=fake):
        return hip_lib.edgedict_frame_skip_scan(logits, dtype, al, B, T, V, blank, f(log_thr), lp, fmap, kept, None)

    def gather(enc=fake, dtype=0, fmap=fake, kept=fake, B=2, T=5, P=8, Tc=3, out=fake):
        return hip_lib.edgedict_frame_skip_gather(enc, dtype, fmap, kept, B, T, P, Tc, out, None)

    for fn, nulls in ((scan, ("logits", "al", "lp", "fmap", "kept")), (gather, ("enc", "fmap", "kept", "out"))):
        for name in nulls:
            assert fn(**{name: None}) == -1, (fn.__name__, name)
            assert b"null pointer" in hip_lib.edgedict_last_error(), (fn.__name__, name)
        for kw, word in ((dict(dtype=7), b"dtype"), (dict(B=0), b"positive"), (dict(T=0), b"positive"),
                         (dict(B=70000), b"65535"), (dict(B=65535, T=40000), b"2^31")):
            assert fn(**kw) == -1, (fn.__name__, kw)
            assert word in hip_lib.edgedict_last_error(), (fn.__name__, kw)
    for kw, word in ((dict(V=1), b"V = 1"), (dict(blank=16), b"blank"), (dict(blank=-1), b"blank"),
                     (dict(log_thr=0.25), b"log_thr"), (dict(log_thr=float("nan")), b"log_thr"),
                     (dict(log_thr=-float("inf")), b"log_thr")):
        assert scan(**kw) == -1, kw
        assert word in hip_lib.edgedict_last_error(), kw
    for kw, word in ((dict(P=0), b"P must"), (dict(Tc=0), b"Tc"), (dict(Tc=6), b"Tc")):
        assert gather(**kw) == -1, kw
        assert word in hip_lib.edgedict_last_error(), kw
    odd = ctypes.c_void_p(fake.value + 2)
    assert gather(enc=odd) == -1 and b"aligned" in hip_lib.edgedict_last_error()


def test_blank_skip_refuses_bad_thresholds_and_inputs():
    from edgedict_amd.decode import gather_frames
    from edgedict_amd.loss import ctc_blank_skip
    z = torch.zeros(2, 5, 8)
    al = torch.tensor([5, 4], dtype=torch.int32)
    for bad in (0.0, -0.5, 1.0001, float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError, match="threshold"):
            ctc_blank_skip(z, al, bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ctc_blank_skip(z, al, 0.5)
    with pytest.raises(TypeError, match="float32 or bfloat16"):
        ctc_blank_skip(z.double(), al, 0.5)
    with pytest.raises(TypeError, match="act_lens must be int32"):
        ctc_blank_skip(z, al.long(), 0.5)
    with pytest.raises(ValueError, match="3 dimensions"):
        ctc_blank_skip(z[0], al, 0.5)
    with pytest.raises(ValueError, match="contiguous"):
        ctc_blank_skip(z.transpose(1, 2), al, 0.5)
    with pytest.raises(ValueError, match="length per example"):
        ctc_blank_skip(z, al[:1], 0.5)
    with pytest.raises(ValueError, match="blank"):
        ctc_blank_skip(z, al, 0.5, blank=8)
    with pytest.raises(ValueError, match="at least the blank"):
        ctc_blank_skip(z[:, :, :1].contiguous(), al, 0.5)
    fmap = torch.zeros(2, 5, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gather_frames(z, fmap, al, 3)
    with pytest.raises(ValueError, match="Tc"):
        gather_frames(z, fmap, al, 6)
    with pytest.raises(ValueError, match="Tc"):
        gather_frames(z, fmap, al, 0)
    with pytest.raises(TypeError, match="int32"):
        gather_frames(z, fmap.long(), al, 3)
    with pytest.raises(ValueError, match="frame_map"):
        gather_frames(z, fmap[:, :4].contiguous(), al, 3)
    with pytest.raises(ValueError, match="out must"):
        gather_frames(z, fmap, al, 3, out=torch.zeros(2, 4, 8))


def _entry_points(m):
    from edgedict_amd import decode
    return [m.sync_beam_search, m.sync_beam_search_nbest, m.beam_search, m.beam_search_nbest,
            lambda *a, **k: decode.sync_beam_search_fusion(m, *a, **k),
            lambda *a, **k: decode.sync_beam_search_nbest(m, *a, **k),
            lambda *a, **k: decode.beam_search_batch(m, *a, **k),
            lambda *a, **k: decode.beam_search_nbest(m, *a, **k)]


def test_skip_blank_argument_rules_come_before_the_device():
    """CPU tensors throughout: a call that got as far as the device check would raise its "no CPU fallback" instead."""
    from edgedict_amd import decode
    from edgedict_amd.models import Transducer
    xs, xlen = torch.zeros(2, 8, 16), torch.tensor([8, 6])
    with_head = Transducer(**_KW, ctc_weight=0.3).eval()
    plain = Transducer(**_KW).eval()
    for fn in _entry_points(with_head):
        for bad in (0.0, 1.5, -1.0, float("nan")):
            with pytest.raises(ValueError, match="threshold"):
                fn(xs, xlen, W=2, skip_blank=bad)
        with pytest.raises(RuntimeError, match="no CPU fallback"):        # valid arguments: it is the device's turn
            fn(xs, xlen, W=2, skip_blank=0.5)
    for fn in _entry_points(plain):
        with pytest.raises(RuntimeError, match="no CTC head"):
            fn(xs, xlen, W=2, skip_blank=0.5)
    for fn in (with_head.beam_search, lambda *a, **k: decode.beam_search_batch(with_head, *a, **k)):
        with pytest.raises(ValueError, match="prefix"):
            fn(xs, xlen, W=2, prefix=True, skip_blank=0.5)
    enc = torch.zeros(2, 4, 12)
    with pytest.raises(ValueError, match="threshold"):
        decode.skip_blank_frames(with_head, enc, None, 2.0)
    with pytest.raises(RuntimeError, match="no CTC head"):
        decode.skip_blank_frames(plain, enc, None, 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        decode.skip_blank_frames(with_head, enc, None, 0.5)


def test_restore_maps_frames_to_the_original_numbering():
    from edgedict_amd.decode import NBestResult, SkippedFrames
    fmap = np.array([[2, 5, 9, -1], [0, 1, -1, -1]], dtype=np.int32)
    sk = SkippedFrames(None, np.array([3, 2], dtype=np.int32), fmap)
    res = [NBestResult([np.array([7, 8]), np.zeros(0, np.int64)], [np.array([0, 2], np.int32), np.zeros(0, np.int32)],
                       [np.zeros(2), np.zeros(0)], [-1.0, -2.0]),
           NBestResult([np.array([4])], [np.array([1], np.int32)], [np.zeros(1)], [-0.5])]
    out = sk.restore(res)
    assert out is res
    assert res[0].frames[0].tolist() == [2, 9] and res[0].frames[1].tolist() == [] and res[1].frames[0].tolist() == [1]
    assert all(f.dtype == np.int32 for r in res for f in r.frames)
