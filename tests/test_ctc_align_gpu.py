"""GPU: the CTC forced aligner (edgedict_ctc_align: the loss's row pass, the Viterbi walk, the back-trace) against the
float64 restatement tests/ctc_align_ref.py (pinned on the CPU by test_ctc_align_host.py).

Two references.  (1) The restatement REPLAYED on the kernel's own float32 log-probability planes: one max and one add
per cell in float64, the operations of the kernel in the kernel's order, so frames, ends, the float32 scores and the
float64 lattice v must agree bit for bit.  (2) The restatement from the logits as the dtype rounds them, through a
float64 log-softmax: the kernel differs from it by its fp32 log-sum-exp only - the loss's arithmetic and a sum of the
loss's magnitude (T_b terms) - so the project's CTC cost bound holds (tests/test_ctc_gpu.py): fp32 rtol 1e-5 / atol 1e-4,
bf16 rtol 1e-4.  Cases: the construction of test_ctc_gpu._case (3-symbol alphabet, adjacent repeats everywhere, ragged
lengths), T = max(U_b + repeats_b) + 5.  Every test prints its maximum error."""
import functools
import types

import numpy as np
import pytest
import torch

import ctc_align_ref as AR
import ctc_ref as CR
from test_ctc_gpu import _case, _dev, _model, _tiny

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])

# (B, U, V): every states-per-lane count C = 2 .. 32 (S = 2U+1 <= 128 / 256 / 512 / 1024 / above) and the lane edges
# S = 63 / 65 / 127 / 129; (1, 513, 8) is S = 1027, C = 32; a V on the scalar path (29), the workload's V (4096)
SHAPES = [(1, 0, 8), (1, 1, 8), (3, 4, 29), (2, 31, 32), (2, 32, 32), (2, 63, 40), (2, 64, 40), (2, 128, 520),
          (2, 257, 16), (1, 513, 8), (4, 9, 4096)]
SHAPE_IDS = ["%dx%dx%d" % s for s in SHAPES]
NEG = float("-inf")


def _tol(dtype, ref):
    """the project's CTC cost bound around a reference value"""
    ref = np.abs(np.asarray(ref, dtype=np.float64))
    return 1e-5 * ref + 1e-4 if dtype == F32 else 1e-4 * ref


def _logits(z, dtype):
    return torch.tensor(z, device="cuda").to(dtype)


@functools.lru_cache(maxsize=None)
def _oracle(B, U, V, dtype):
    """the float64 optimum from the logits as the dtype rounds them (test_ctc_gpu._oracle's treatment)"""
    z, labels, act, lab, _ = _case(B, U, V)
    seen = torch.tensor(z).to(dtype).double().numpy()
    return seen, AR.align_batch(seen, labels, act, lab)


def _check_invariants(frames, ends, labels, act, lab, scores):
    """point 3, on every row with a path"""
    for b in range(frames.shape[0]):
        Tb, Ub = int(act[b]), int(lab[b])
        assert (frames[b, Ub:] == -1).all() and (ends[b, Ub:] == -1).all(), b
        if scores[b] == NEG:
            assert (frames[b] == -1).all() and (ends[b] == -1).all(), b
            continue
        f, e = frames[b, :Ub], ends[b, :Ub]
        assert (f >= 0).all() and (f <= e).all(), b
        assert (e[:-1] < f[1:]).all(), b
        if Ub:
            assert e[-1] <= Tb - 1, b
        for u in range(1, Ub):
            if labels[b, u] == labels[b, u - 1]:
                assert f[u] >= e[u - 1] + 2, (b, u)


@pytest.mark.parametrize("B,U,V", SHAPES, ids=SHAPE_IDS)
@DTYPES
def test_exact_against_the_replay_and_invariants(hip_lib, B, U, V, dtype):
    """Points 1 and 3: frames, ends, float32 scores and the float64 lattice equal the replay on the kernel's own lp
    planes bit for bit; -1 padding; two runs identical; labels behind label_lens change nothing; path invariants."""
    from edgedict_amd.loss import ctc_align, ctc_align_debug
    z, labels, act, lab, _ = _case(B, U, V)
    tz = _logits(z, dtype)
    tl, ta, tb = _dev(labels, act, lab)
    frames, ends, scores, lpb, lpl, v = ctc_align_debug(tz, tl, ta, tb)
    assert frames.shape == ends.shape == (B, U) and frames.dtype == ends.dtype == torch.int32
    assert scores.shape == (B,) and scores.dtype == torch.float32
    assert lpb.shape == (B, z.shape[1]) and lpl.shape == (B, z.shape[1], U) and v.shape == (B, z.shape[1], 2 * U + 1)
    fr, en, sc = frames.cpu().numpy(), ends.cpu().numpy(), scores.cpu().numpy()
    lpb, lpl, v = lpb.cpu().numpy(), lpl.cpu().numpy(), v.cpu().numpy()
    for b in range(B):
        Tb, Ub = int(act[b]), int(lab[b])
        f, e, s, vr, _ = AR.replay(lpb[b, :Tb], lpl[b, :Tb, :Ub], labels[b, :Ub])
        assert np.isfinite(s), b
        assert (fr[b, :Ub] == f).all() and (en[b, :Ub] == e).all(), b
        assert (fr[b, Ub:] == -1).all() and (en[b, Ub:] == -1).all(), b
        assert np.float32(s).tobytes() == sc[b].tobytes(), (b, s, sc[b])
        assert np.array_equal(v[b, :Tb, :2 * Ub + 1], vr), b
        assert not v[b, Tb:].any() and not v[b, :, 2 * Ub + 1:].any(), b          # outside the box: never written
    _check_invariants(fr, en, labels, act, lab, sc)
    # the plain entry point, twice: bit-identical to the debug run and to each other
    for _ in range(2):
        f2, e2, s2 = ctc_align(tz, tl, ta, tb)
        assert torch.equal(f2, frames) and torch.equal(e2, ends) and torch.equal(s2, scores)
    # padding labels behind label_lens: no effect
    other = labels.copy()
    for b in range(B):
        other[b, lab[b]:] = V - 2
    f3, e3, s3 = ctc_align(tz, torch.tensor(other, device="cuda"), ta, tb)
    assert torch.equal(f3, frames) and torch.equal(e3, ends) and torch.equal(s3, scores)
    print("ctc align exact", (B, U, V), dtype, "T %d, scores" % z.shape[1], sc.tolist()[:4])


@pytest.mark.parametrize("B,U,V", SHAPES, ids=SHAPE_IDS)
@DTYPES
def test_independent_oracle(hip_lib, B, U, V, dtype):
    """Point 2: the score and the returned path's float64 re-score are within the CTC cost bound of the float64 optimum
    found from the rounded logits; score <= -cost of CTCLoss plus that bound."""
    from edgedict_amd.loss import CTCLoss, ctc_align
    z, labels, act, lab, _ = _case(B, U, V)
    seen, (_, _, best, _) = _oracle(B, U, V, dtype)
    tz = _logits(z, dtype)
    tl, ta, tb = _dev(labels, act, lab)
    frames, ends, scores = ctc_align(tz, tl, ta, tb)
    cost = CTCLoss(blank=0, reduction="none")(tz, tl, ta, tb).double().cpu().numpy()
    fr, en, sc = frames.cpu().numpy(), ends.cpu().numpy(), scores.double().cpu().numpy()
    assert np.isfinite(best).all() and np.isfinite(sc).all()
    worst = worst_path = 0.0
    for b in range(B):
        Tb, Ub = int(act[b]), int(lab[b])
        tol = _tol(dtype, best[b])
        states = AR.states_from_spans(fr[b, :Ub], en[b, :Ub], Tb)
        again = AR.rescore(seen[b, :Tb], states, labels[b, :Ub])
        worst, worst_path = max(worst, abs(sc[b] - best[b])), max(worst_path, abs(again - best[b]))
        assert abs(sc[b] - best[b]) <= tol, (b, sc[b], best[b])
        assert again <= best[b] + 1e-9 * abs(best[b]) and best[b] - again <= tol, (b, again, best[b])
        assert sc[b] <= -cost[b] + _tol(dtype, cost[b]), (b, sc[b], cost[b])
    print("ctc align oracle", (B, U, V), dtype, "max score err %.3g, max path deficit %.3g (|best| up to %.3g)"
          % (worst, worst_path, np.abs(best).max()))


def _forced_frames(y):
    """T_b = U_b + repeats exactly: every label lasts one frame, a blank only between adjacent repeats."""
    out, t = [], 0
    for u, k in enumerate(y):
        if u and k == y[u - 1]:
            t += 1
        out.append(t)
        t += 1
    return out


@pytest.mark.parametrize("B,U,V", SHAPES, ids=SHAPE_IDS)
@DTYPES
def test_forced_and_infeasible_row(hip_lib, B, U, V, dtype):
    """Point 4: row 0 with T_b = U_b + repeats_b exactly has one path - the literal frames; with one frame fewer it has
    score -inf and -1 everywhere while its batch neighbours keep their results.  (U = 0: one frame, then none.)"""
    from edgedict_amd.loss import ctc_align
    z, labels, act, lab, need = _case(B, U, V)
    tz = _logits(z, dtype)
    tl, ta, tb = _dev(labels, act, lab)
    frames, ends, scores = ctc_align(tz, tl, ta, tb)
    exact = act.copy()
    exact[0] = max(1, need[0])
    f1, e1, s1 = ctc_align(tz, tl, torch.tensor(exact, device="cuda"), tb, check_lengths=False)
    want = _forced_frames(list(labels[0, :lab[0]]))
    assert len(want) == 0 or want[-1] == exact[0] - 1
    assert f1[0, :lab[0]].tolist() == want and e1[0, :lab[0]].tolist() == want
    assert np.isfinite(s1[0].item())
    seen = torch.tensor(z).to(dtype).double().numpy()
    ref = AR.rescore(seen[0, :exact[0]], AR.states_from_spans(want, want, int(exact[0])), labels[0, :lab[0]])
    assert abs(s1[0].item() - ref) <= _tol(dtype, ref), (s1[0].item(), ref)
    assert torch.equal(f1[1:], frames[1:]) and torch.equal(e1[1:], ends[1:]) and torch.equal(s1[1:], scores[1:])
    short = act.copy()
    short[0] = exact[0] - 1
    f0, e0, s0 = ctc_align(tz, tl, torch.tensor(short, device="cuda"), tb, check_lengths=False)
    assert s0[0].item() == NEG
    assert (f0[0] == -1).all() and (e0[0] == -1).all()
    assert torch.equal(f0[1:], frames[1:]) and torch.equal(e0[1:], ends[1:]) and torch.equal(s0[1:], scores[1:])
    print("ctc align forced", (B, U, V), dtype, "T_0 = %d: score %.6g (fp64 %.6g)" % (exact[0], s1[0].item(), ref))


@DTYPES
def test_single_frame_rows_and_garbage_behind_the_lengths(hip_lib, dtype):
    """Point 4: T_b = 1 with one label (the label on frame 0) and with none (the blank), beside a longer row; NaN logits
    behind act_lens are never read."""
    from edgedict_amd.loss import ctc_align, ctc_align_debug
    rng = np.random.default_rng(5)
    B, T, U, V = 4, 6, 3, 8
    z = (2.0 * rng.normal(size=(B, T, V))).astype(np.float32)
    labels = np.array([[2, 1, 1], [3, 3, 3], [1, 2, 1], [1, 1, 2]], dtype=np.int32)
    act = np.array([1, 1, 6, 4], dtype=np.int32)
    lab = np.array([1, 0, 3, 3], dtype=np.int32)
    tl, ta, tb = _dev(labels, act, lab)
    frames, ends, scores, lpb, lpl, _ = ctc_align_debug(_logits(z, dtype), tl, ta, tb)
    assert frames[0].tolist() == [0, -1, -1] and ends[0].tolist() == [0, -1, -1]
    assert scores[0].item() == lpl[0, 0, 0].item()
    assert frames[1].tolist() == [-1, -1, -1] and scores[1].item() == lpb[1, 0].item()
    assert torch.isfinite(scores).all() and (frames[2] >= 0).all() and ends[3, 2].item() <= 3
    _check_invariants(frames.cpu().numpy(), ends.cpu().numpy(), labels, act, lab, scores.cpu().numpy())
    dirty = z.copy()
    for b in range(B):
        dirty[b, act[b]:] = np.nan
    f2, e2, s2 = ctc_align(_logits(dirty, dtype), tl, ta, tb)
    assert torch.equal(f2, frames) and torch.equal(e2, ends) and torch.equal(s2, scores)
    # T_b = 0 beside them: no path, the others as before
    none = act.copy()
    none[3] = 0
    f3, e3, s3 = ctc_align(_logits(dirty, dtype), tl, torch.tensor(none, device="cuda"), tb)
    assert s3[3].item() == NEG and (f3[3] == -1).all() and (e3[3] == -1).all()
    assert torch.equal(f3[:3], frames[:3]) and torch.equal(e3[:3], ends[:3]) and torch.equal(s3[:3], scores[:3])


@DTYPES
def test_tie_rule_on_zero_logits(hip_lib, dtype):
    """Point 5: constant log-probabilities, every path scores equal - the literal frames of the host test."""
    from edgedict_amd.loss import ctc_align
    labels = np.array([[1, 2, 3, 1], [1, 1, 2, 2], [1, 1, 2, 2], [1, 1, 2, 2]], dtype=np.int32)
    act = np.array([9, 9, 6, 5], dtype=np.int32)
    lab = np.full(4, 4, dtype=np.int32)
    z = torch.zeros(4, 9, 4, device="cuda", dtype=dtype)
    frames, ends, scores = ctc_align(z, *_dev(labels, act, lab))
    want = [[5, 6, 7, 8], [3, 5, 6, 8], [0, 2, 3, 5], [-1, -1, -1, -1]]
    assert frames.tolist() == want and ends.tolist() == want
    ref = act[:3] * np.log(0.25)
    np.testing.assert_allclose(scores[:3].double().cpu().numpy(), ref, rtol=1e-5 if dtype == F32 else 1e-4, atol=1e-4)
    assert scores[3].item() == NEG
    for b in range(3):
        one = AR.align_one(np.zeros((act[b], 4)), labels[b])
        assert one[0].tolist() == want[b] and one[1].tolist() == want[b]


GREEDY_SEED, GREEDY_GAP = 4, 1e-2          # (the smallest top-two gap of this seed's 120 frames is 0.043)


def test_aligning_the_greedy_transcript_returns_the_greedy_frames(hip_lib):
    """Point 6 (fp32): every frame's top-two logit gap is nonzero (asserted, with room for the fp32 subtraction of the
    log-sum-exp), so the frame-wise arg max path is the single best of ALL paths, it collapses to the greedy transcript
    and is therefore the aligner's: ctc_greedy's frames, and the sum of the per-frame maxima of the kernel's lp."""
    from edgedict_amd.loss import ctc_align_debug, ctc_greedy
    rng = np.random.default_rng(GREEDY_SEED)
    B, T, V = 3, 40, 6
    z = (2.0 * rng.normal(size=(B, T, V))).astype(np.float32)
    top = np.sort(z, axis=-1)
    gap = (top[..., -1] - top[..., -2]).min()
    assert gap > 0 and gap > GREEDY_GAP, gap
    act = np.array([T, T - 7, 1], dtype=np.int32)
    tz, ta = _logits(z, F32), torch.tensor(act, device="cuda")
    tokens, counts, gframes, _ = ctc_greedy(tz, ta)
    U = int(counts.max())
    assert U >= 10
    labels = tokens[:, :U].clamp(min=1).contiguous()
    y = labels.cpu().numpy()
    assert any(CR.repeats(list(y[b, :int(counts[b])])) for b in range(B))          # blank-separated repeats occur
    frames, ends, scores, lpb, lpl, _ = ctc_align_debug(tz, labels, ta, counts)
    assert torch.equal(frames, gframes[:, :U])
    lpb, lpl, sc = lpb.double().cpu().numpy(), lpl.double().cpu().numpy(), scores.double().cpu().numpy()
    for b in range(B):
        Tb, Ub = int(act[b]), int(counts[b])
        per_frame = lpb[b, :Tb]
        if Ub:
            per_frame = np.maximum(per_frame, lpl[b, :Tb, :Ub].max(axis=-1))
        want = per_frame.sum()
        print("ctc align greedy row %d: U_b %d, score %.6f, sum of maxima %.6f" % (b, Ub, sc[b], want))
        assert abs(sc[b] - want) <= _tol(F32, want), (b, sc[b], want)
    _check_invariants(frames.cpu().numpy(), ends.cpu().numpy(), y, act, counts.cpu().numpy(), scores.cpu().numpy())


@pytest.mark.parametrize("cd", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["tiny", "gru_tiny"])
def test_model_alignment_windows_and_times(hip_lib, name, cd):
    """Point 7: Transducer.ctc_align = loss.ctc_align on the model's own head logits, bit for bit; a model without the
    head raises; forward / align under ctc_windows(left=2, right=2) are finite and the restricted RNN-T loss is not below
    the unrestricted one (up to the RNN-T cost bound of test_arloss_gpu.py); a row without a CTC path gets the open
    windows lo = 0, hi = T - 1 and a finite loss; emission_times on frames and ends."""
    from edgedict_amd.decode import emission_times
    from edgedict_amd.loss import alignment_windows, ctc_align
    cfg, sd, (xs, ys, xlen, ylen) = _tiny(name)
    m = _model(cfg, sd, cd, 0.3).eval()
    xs_d, ys_d = xs.cuda(), ys.cuda()
    frames, ends, scores = m.ctc_align(xs_d, ys_d, xlen, ylen)
    with torch.no_grad():
        h_enc, _ = m.encoder(xs_d[:, :int(xlen.max())].contiguous())
        act = m.scale_length(h_enc, xlen).to(torch.int32).cuda()
        head_logits = m._ctc_logits(h_enc).contiguous()
    U = int(ylen.max())
    labels = ys_d[:, :U].to(torch.int32).contiguous()
    lab = ylen.to(torch.int32).cuda()
    f2, e2, s2 = ctc_align(head_logits, labels, act, lab, m.blank, check_lengths=False)
    assert frames.shape == (xs.shape[0], U) and frames.is_cuda
    assert torch.equal(frames, f2) and torch.equal(ends, e2) and torch.equal(scores, s2)
    fd, ed, sd2 = m.ctc_align(xs_d, ys_d, xlen.cuda(), ylen.cuda())                # lengths on the device
    assert torch.equal(fd, frames) and torch.equal(ed, ends) and torch.equal(sd2, scores)
    _check_invariants(frames.cpu().numpy(), ends.cpu().numpy(), labels.cpu().numpy(), act.cpu().numpy(),
                      lab.cpu().numpy(), scores.cpu().numpy())
    with pytest.raises(RuntimeError, match="no CTC head"):
        _model(cfg, sd, cd, 0.0).ctc_align(xs_d, ys_d, xlen, ylen)
    # windows: rows with a path are alignment_windows of their frames, rows without one are unrestricted
    lo, hi = m.ctc_windows(xs_d, ys_d, xlen, ylen, 2, 2)
    wl, wh = alignment_windows(frames, act, lab, 2, 2)
    live = torch.isfinite(scores)
    T = int(act.max())
    print("ctc align model", name, cd, "T %d, scores" % T, scores.tolist(), "frames", frames.tolist())
    assert lo.dtype == torch.int32 and lo.shape == frames.shape
    assert torch.equal(lo[live], wl[live]) and torch.equal(hi[live], wh[live])
    assert (lo[~live] == 0).all() and (hi[~live] == T - 1).all()
    # a row without a CTC path (one token repeated: U_0 + repeats_0 = 2 U_0 - 1 > T_0) stays unrestricted, not dead
    ys_rep = ys.clone()
    ys_rep[0, :] = ys[0, 0]
    assert 2 * int(ylen[0]) - 1 > int(act[0])
    fr_r, en_r, sc_r = m.ctc_align(xs_d, ys_rep.cuda(), xlen, ylen)
    assert sc_r[0].item() == NEG and (fr_r[0] == -1).all() and (en_r[0] == -1).all()
    assert torch.equal(fr_r[1:], frames[1:]) and torch.equal(en_r[1:], ends[1:]) and torch.equal(sc_r[1:], scores[1:])
    lo_r, hi_r = m.ctc_windows(xs_d, ys_rep.cuda(), xlen, ylen, 2, 2)
    assert (lo_r[0] == 0).all() and (hi_r[0] == T - 1).all()
    assert torch.equal(lo_r[1:], lo[1:]) and torch.equal(hi_r[1:], hi[1:])
    m.train()
    open_row = m(xs_d, ys_rep.cuda(), xlen, ylen, windows=(lo_r, hi_r))
    assert torch.isfinite(open_row).all()
    restricted = m(xs_d, ys_d, xlen, ylen, windows=(lo, hi))
    r_rnnt = m.loss_parts[0].item()
    plain = m(xs_d, ys_d, xlen, ylen)
    p_rnnt = m.loss_parts[0].item()
    assert torch.isfinite(restricted).all() and torch.isfinite(plain).all()
    bound = 1e-5 * abs(p_rnnt) + 1e-4 if cd == "fp32" else 1e-4 * abs(p_rnnt)
    print("ctc windows", name, cd, "restricted rnnt %.6f, unrestricted %.6f" % (r_rnnt, p_rnnt))
    assert r_rnnt >= p_rnnt - bound
    m.eval()
    fa, sa = m.align(xs_d, ys_d, xlen, ylen, windows=(lo, hi))
    assert torch.isfinite(sa).all()
    assert ((fa >= lo) & (fa <= hi))[fa >= 0].all()
    flags = types.SimpleNamespace(hop_length=160, downsample=3, sample_rate=16000)
    start, stop = emission_times(frames, flags), emission_times(ends, flags)
    assert start.dtype == torch.float64 and start.shape == frames.shape
    pad = (frames < 0).cpu()
    assert torch.isnan(start.cpu()[pad]).all() and torch.isnan(stop.cpu()[pad]).all()
    assert torch.equal(start.cpu()[~pad], frames.cpu()[~pad].double() * 0.06)
    assert (stop.cpu()[~pad] >= start.cpu()[~pad]).all()
