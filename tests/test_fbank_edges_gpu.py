"""GPU: the three kernels of csrc/fbank.hip against the float64 restatement of tests/fbank_ref.py, on what speech holds and
noise does not (tones, DC, silence, half-silent frames, clipping, int16-scale and 1e-6-scale amplitudes) and at the edges
of the accepted argument space (n_fft 64 ... 2048, two mel passes, window == n_fft, off-centre window, N < n_fft,
hop | N, B * frames not a multiple of the 4 frames of a workgroup, bf16 output, strided and poisoned rows).

The accuracy measure is the frame-relative error in the LINEAR mel domain (fbank_ref.frame_rel_err) against
FBANK_KERNEL_TOL = 8 * FBANK_ORACLE_ERR = 6.8e-6, a bound tied to the CPU fp32 oracle's own error against float64
(test_fbank_ref_host.py), not to the kernel's; the log output is then pinned to the linear one, which is what lets tones
and DC be checked without a log-domain tolerance.

Measured on the MI355X, worst frame-relative error of fbank_kernel over the ten signals, per n_fft (every worst case is
the DC row; the second figure is the worst of the other nine signals):
    n_fft   64: 1.75e-6   2.7e-7
    n_fft  256: 1.99e-6   2.4e-7
    n_fft  512: 2.04e-6   2.9e-7      (five geometries, N = 257 and 300 included)
    n_fft 1024: 1.89e-6   2.9e-7
    n_fft 2048: 2.07e-6   4.4e-7
The worst, 2.07e-6, sits 3.3x under FBANK_KERNEL_TOL; without DC the kernel is 15x under it and level with the CPU oracle.
DC's 1.9e-6 is the float32 rounding of the pre-emphasis coefficient (fbank_ref's docstring), not FFT error: it does not
grow with n_fft.  feat_normalize_kernel: 8.1e-6 per_feature (n = 2 frames), 5.3e-7 all_features, against 1.0e-4.
"""
import math

import numpy as np
import pytest
import torch

import fbank_ref as R

pytestmark = pytest.mark.gpu

# The log output against log(float32 linear output + 1e-20) evaluated in float64.  One fp32 ulp at |log(1e-20)| = 46.05
# is 3.8e-6, so 2e-6 asks for the correctly rounded logarithm (half an ulp: 1.9e-6) of the very same energy.
LOG_TOL = 2e-6


def _fbank(win, hop, n_fft, n_mels, **kw):
    from edgedict_amd.features import FilterbankFeatures
    kw.setdefault("dither", 0)
    return FilterbankFeatures(win_length=win, hop_length=hop, n_fft=n_fft, n_filt=n_mels, **kw).cuda()


def _stacked(win, hop, n_fft, n_mels, **kw):
    from edgedict_amd.features import StackedLogFbank
    kw.setdefault("dither", 0)
    return StackedLogFbank(win_length=win, hop_length=hop, n_fft=n_fft, n_filt=n_mels, **kw).cuda()


_CACHE = {}


def _case(geom):
    """signals, the kernel's linear output and its float64 reference for one geometry: computed once, never modified."""
    if geom not in _CACHE:
        N, win, hop, n_fft, n_mels = geom
        x = R.signals(N)
        m = _fbank(win, hop, n_fft, n_mels, log=False)
        lin = m(x.cuda()).cpu()
        ref = R.fbank64(x, m.window, m.fb, hop, n_fft, m.preemph)
        _CACHE[geom] = (x, lin, ref)
    return _CACHE[geom]


def _geom_id(g):
    return "N%d-win%d-hop%d-fft%d-mel%d" % g


@pytest.mark.parametrize("geom", R.GEOMETRIES, ids=_geom_id)
def test_linear_mel_energies_match_fp64_on_every_signal(hip_lib, geom):
    N, win, hop, n_fft, n_mels = geom
    x, lin, ref = _case(geom)
    assert lin.shape == (len(R.SIGNAL_NAMES), n_mels, 1 + N // hop) and lin.dtype == torch.float32
    assert bool(torch.isfinite(lin).all())
    errs = [R.frame_rel_err(lin[s:s + 1], ref[s:s + 1]) for s in range(len(R.SIGNAL_NAMES))]
    print("\nfbank_kernel n_fft %d %s: worst %.3e (%s); %s" % (
        n_fft, _geom_id(geom), max(errs), R.SIGNAL_NAMES[int(np.argmax(errs))],
        ", ".join("%s %.1e" % (n, e) for n, e in zip(R.SIGNAL_NAMES, errs))))
    # dead frames (all-zero input) are exactly 0, and so is every frame >= ceil(N / hop)
    assert R.dead_frames_exact(lin, ref)
    zeros = R.SIGNAL_NAMES.index("zeros")
    assert np.all(ref[zeros] == 0) and bool((lin[zeros] == 0).all())
    if N >= 2000:                                                           # the case does hold dead frames next to live ones
        assert np.any(ref[R.SIGNAL_NAMES.index("half_silent")].max(axis=0)[:-1] == 0)
    assert bool((lin[:, :, math.ceil(N / hop):] == 0).all())
    assert max(errs) <= R.FBANK_KERNEL_TOL, errs


@pytest.mark.parametrize("geom", R.GEOMETRIES, ids=_geom_id)
def test_log_output_is_the_log_of_the_linear_output(hip_lib, geom):
    """Failed before the fix on every geometry: logf(0 + 1e-20f), the value of every silent frame, came out 2 ulp high
    (6.4e-6 off); the kernel now takes the logarithm in double and rounds once."""
    N, win, hop, n_fft, n_mels = geom
    x, lin, ref = _case(geom)
    out = _fbank(win, hop, n_fft, n_mels, log=True)(x.cuda()).cpu()
    assert out.shape == lin.shape and bool(torch.isfinite(out).all())
    live = math.ceil(N / hop)
    want = np.log(lin.double().numpy() + R.LOG_FLOOR)
    assert np.abs(out.double().numpy()[:, :, :live] - want[:, :, :live]).max() <= LOG_TOL
    assert bool((out[:, :, live:] == 0).all())                              # masked frames are 0, not log(1e-20)
    zeros = R.SIGNAL_NAMES.index("zeros")
    assert np.abs(out[zeros, :, :live].double().numpy() - math.log(1e-20)).max() <= LOG_TOL
    dead = ref.max(axis=1)[:, :live] <= 0
    assert np.abs(out.double().numpy()[:, :, :live].transpose(0, 2, 1)[dead] - math.log(1e-20)).max() <= LOG_TOL


@pytest.mark.parametrize("geom", R.GEOMETRIES, ids=_geom_id)
def test_preemph_none_and_zero_agree_bitwise_and_match_fp64(hip_lib, geom):
    N, win, hop, n_fft, n_mels = geom
    x = _case(geom)[0]
    m0 = _fbank(win, hop, n_fft, n_mels, log=False, preemph=None)
    a = m0(x.cuda()).cpu()
    b = _fbank(win, hop, n_fft, n_mels, log=False, preemph=0.0)(x.cuda()).cpu()
    assert torch.equal(a, b)
    ref = R.fbank64(x, m0.window, m0.fb, hop, n_fft, None)
    assert R.dead_frames_exact(a, ref)
    assert R.frame_rel_err(a, ref) <= R.FBANK_KERNEL_TOL


@pytest.mark.parametrize("window,sr,N", [("hamming", 16000, 4000), ("blackman", 16000, 4001), ("bartlett", 8000, 2600),
                                         ("boxcar-unknown", 16000, 4000), ("hamming", 16000, 300)])
def test_parts_twin_other_windows_match_fp64(hip_lib, window, sr, N):
    """parts mode (seq_len only masks; N = 300 < n_fft is zero-padded to win_length after the pre-emphasis)."""
    from parts.features import FilterbankFeatures
    m = FilterbankFeatures(sample_rate=sr, window_size=0.02, window_stride=0.01, window=window, normalize="none",
                           nfilt=64, log=False, dither=0.0, pad_to=0).cuda()
    if window == "boxcar-unknown":
        assert bool((m.window == 1).all())
    x = R.signals(N)
    seq = [N] * x.shape[0]
    seq[0], seq[1] = max(N - 3 * m.hop_length - 1, 1), m.hop_length * 2
    out = m(x.cuda(), torch.tensor(seq, dtype=torch.int32).cuda()).cpu()
    ref = R.parts64(m, x, seq)
    assert out.shape == ref.shape
    assert R.dead_frames_exact(out, ref)
    e = R.frame_rel_err(out, ref)
    print("\nparts %s sr %d N %d: %.3e" % (window, sr, N, e))
    assert e <= R.FBANK_KERNEL_TOL


# ------------------------------------------------------------------------------------------------ stacking

STACK_GEOM = (1000, 320, 160, 512, 80)      # 7 frames: with 3 rows 21 frames, with 6 rows 42 - no multiple of 4
STACK_LENS = [1000, 800, 641]               # N, a multiple of hop (last frame masked), an odd tail
SHORT_LENS = [159, 1, 0]                    # hop - 1, 1, 0: below n_fft/2 + 1, outside what torch.stft accepts


def _stack_wave(B, N):
    g = torch.Generator(device="cpu").manual_seed(4300)
    t = torch.arange(N, dtype=torch.float64) / R.SAMPLE_RATE
    return (0.05 * torch.randn(B, N, generator=g) + 0.5 * torch.sin(2 * math.pi * 700.0 * t).float()[None]).contiguous()


@pytest.mark.parametrize("pad", [True, False], ids=["pad", "truncate"])
@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_stacked_ragged_equals_per_utterance_output_rearranged(hip_lib, k, pad):
    """Rows shorter than n_fft/2 + 1 samples need a second reflection, which torch.stft does not define: NO parity is claimed
    for them - they only have to come out finite and leave the other rows bit-identical to a batch without them."""
    N, win, hop, n_fft, M = STACK_GEOM
    x = _stack_wave(6, N)
    single = _fbank(win, hop, n_fft, M, log=True)
    mod = _stacked(win, hop, n_fft, M, n_frame=k, pad_to_divisible=pad)
    F = 1 + N // hop
    T0 = (F + k - 1) // k if pad else F // k
    xs3, xlen3 = mod(x[:3].cuda(), torch.tensor(STACK_LENS, dtype=torch.int32))
    xs6, xlen6 = mod(x.cuda(), torch.tensor(STACK_LENS + SHORT_LENS, dtype=torch.int32).cuda())
    xs3, xs6 = xs3.cpu(), xs6.cpu()
    assert xs3.shape == (3, T0, M * k) and xs6.shape == (6, T0, M * k)
    assert bool(torch.isfinite(xs6).all())
    assert torch.equal(xs6[:3], xs3)
    for b, n in enumerate(STACK_LENS):
        alone = single(x[b:b + 1, :n].contiguous().cuda()).cpu().numpy()          # [1, M, 1 + n // hop], masked at ceil(n / hop)
        Fb = alone.shape[2]
        full = np.zeros((1, M, max(F, T0 * k)), dtype=np.float32)
        full[:, :, :Fb] = alone
        want = R.stack64(full[:, :, :F], k, pad)
        assert np.array_equal(xs3[b:b + 1].numpy(), want), (b, n)
        live = math.ceil(n / hop)
        flat = xs3[b].reshape(T0 * k, M)[live:]
        assert bool((flat == 0).all())                                           # masked and padded frames: exact zeros
        assert bool((xs3[b].reshape(T0 * k, M)[:min(live, T0 * k)] != 0).all())
    for lens, xlen in ((STACK_LENS, xlen3), (STACK_LENS + SHORT_LENS, xlen6)):
        want = [(1 + n // hop + k - 1) // k if pad else (1 + n // hop) // k for n in lens]
        assert xlen.cpu().tolist() == want and xlen.dtype == torch.int32


@pytest.mark.parametrize("geom,lens", [((1000, 320, 160, 512, 80), [1000, 800, 641]),
                                       ((2600, 200, 80, 256, 41), [2600, 1999, 160, 129])],
                         ids=["fft512-mel80", "fft256-mel41"])
def test_bf16_output_is_the_rounded_fp32_output_bit_for_bit(hip_lib, geom, lens):
    """The only test that runs fbank_kernel<bf16_t>.  n_frame = 3: frame f lands at element (f % 3) * n_mels of its stacked
    row; with 41 mels that offset, and every second row of 123 elements, is odd - 2-byte stores that are not 4-byte aligned."""
    N, win, hop, n_fft, M = geom
    x = _stack_wave(len(lens), N)
    ln = torch.tensor(lens, dtype=torch.int32)
    a, alen = _stacked(win, hop, n_fft, M, n_frame=3)(x.cuda(), ln)
    b, blen = _stacked(win, hop, n_fft, M, n_frame=3, out_dtype=torch.bfloat16)(x.cuda(), ln)
    assert b.dtype == torch.bfloat16 and b.shape == a.shape and torch.equal(alen, blen)
    assert torch.equal(b.cpu().view(torch.int16), a.cpu().to(torch.bfloat16).view(torch.int16))
    assert bool((b != 0).any())


# ------------------------------------------------------------------------------------------------ out-of-row reads

def _poisoned_view(x, front=17, back=20):
    """x [B, N] as a view into a [B, N + 37] buffer whose margins (before and after every row) are NaN."""
    B, N = x.shape
    buf = torch.full((B, N + front + back), float("nan"), device="cuda")
    buf[:, front:front + N] = x.cuda()
    v = buf[:, front:front + N]
    assert v.stride(0) == N + 37 and not v.is_contiguous()
    return v


@pytest.mark.parametrize("geom", [(1000, 320, 160, 512, 80), (300, 320, 160, 512, 80), (3000, 64, 32, 64, 16)], ids=_geom_id)
def test_nothing_outside_the_row_is_read(hip_lib, geom):
    N, win, hop, n_fft, M = geom
    x = _stack_wave(4, N)
    # whole rows
    m = _fbank(win, hop, n_fft, M, log=True)
    got = m(_poisoned_view(x)).cpu()
    assert bool(torch.isfinite(got).all()) and torch.equal(got, m(x.cuda()).cpu())
    # rows that end at lengths[b]: the samples past it are poison too
    lens = [N, N - hop, n_fft // 2 + 1 + 3, N - 1]
    ln = torch.tensor(lens, dtype=torch.int32)
    xp = x.clone()
    for b, n in enumerate(lens):
        xp[b, n:] = float("nan")
    s = _stacked(win, hop, n_fft, M, n_frame=3)
    got, _ = s(_poisoned_view(xp), ln)
    clean, _ = s(x.cuda(), ln)
    assert bool(torch.isfinite(got).all()) and torch.equal(got.cpu(), clean.cpu())


def test_parts_mode_reads_nothing_outside_the_padded_row(hip_lib):
    """mask_only = 1 legitimately reads the whole padded row (seq_len only masks): margin poison only."""
    from parts.features import FilterbankFeatures
    x = _stack_wave(3, 2000)
    seq = torch.tensor([2000, 1500, 700], dtype=torch.int32).cuda()
    for norm in ("none", "per_feature"):
        m = FilterbankFeatures(sample_rate=16000, window_size=0.02, window_stride=0.01, window="hann", normalize=norm,
                               nfilt=64, dither=0.0, pad_to=8, frame_splicing=2).cuda()
        got = m(_poisoned_view(x), seq).cpu()
        assert bool(torch.isfinite(got).all()) and torch.equal(got, m(x.cuda(), seq).cpu())


# ------------------------------------------------------------------------------------------------ feat_normalize_kernel

def _parts(normalize, splice, **kw):
    from parts.features import FilterbankFeatures
    return FilterbankFeatures(sample_rate=16000, window_size=0.02, window_stride=0.01, window="hann", normalize=normalize,
                              nfilt=64, dither=0.0, pad_to=0, frame_splicing=splice, **kw).cuda()


@pytest.mark.parametrize("splice", [1, 3])
def test_feat_normalize_matches_fp64_on_ragged_frame_counts(hip_lib, splice):
    """frame counts 2, 3, 255, 256, 257, 300: per_feature puts n, all_features rows * n on both sides of the 256-thread
    stride.  B = 6 rows of 48000 samples: 257 frames of hop 160 need that many."""
    x = R.norm_wave().cuda()
    seq = torch.tensor(R.NORM_SEQ, dtype=torch.int32).cuda()
    raw = _parts("none", splice)(x, seq).cpu()
    assert raw.shape == (6, 64 * splice, 301)
    assert torch.equal(raw, _parts("none", splice)(x, seq).cpu())          # dither 0: reproducible bit for bit
    for mode in ("per_feature", "all_features"):
        got = _parts(mode, splice)(x, seq).cpu().double().numpy()
        ref = R.normalize_batch64(raw, R.NORM_SEQ, R.NORM_HOP, mode)
        assert np.all(np.isfinite(got))
        worst = 0.0
        for b, n in enumerate(R.NORM_FRAMES):
            assert np.all(got[b, :, n:] == 0), (mode, n)                   # frames past n: exactly 0
            worst = max(worst, float(np.abs(got[b, :, :n] - ref[b, :, :n]).max()))
        print("\nfeat_normalize %s splice %d: worst |diff| %.3e" % (mode, splice, worst))
        assert worst <= R.NORM_KERNEL_TOL, (mode, worst)


def test_feat_normalize_single_frame_and_constant_row(hip_lib):
    g = torch.Generator(device="cpu").manual_seed(4400)
    x = 0.1 * torch.randn(3, 4000, generator=g)
    x[1] = 0.0                                                              # silence: every row constant log(1e-20)
    seq_list = [100, 4000, 3999]                                            # row 0: n = 1 frame
    seq = torch.tensor(seq_list, dtype=torch.int32).cuda()
    raw = _parts("none", 1)(x.cuda(), seq).cpu()
    per = _parts("per_feature", 1)(x.cuda(), seq).cpu().numpy()
    # one frame has no unbiased std: NaN in exactly that frame of that row, as torch.std gives - and nowhere else
    assert np.all(np.isnan(per[0, :, 0])) and np.all(per[0, :, 1:] == 0)
    assert np.all(np.isfinite(per[1:]))
    ref = R.normalize_batch64(raw, seq_list, 160, "per_feature")
    assert np.all(np.isnan(ref[0, :, 0]))
    assert np.abs(per[2] - ref[2]).max() <= R.NORM_KERNEL_TOL
    assert np.all(per[1, :, 25:] == 0) and np.all(per[2, :, 25:] == 0)
    # all_features: 64 rows of one frame do have a std
    alls = _parts("all_features", 1)(x.cuda(), seq).cpu().numpy()
    refa = R.normalize_batch64(raw, seq_list, 160, "all_features")
    assert np.all(np.isfinite(alls))
    assert np.abs(alls[0] - refa[0]).max() <= R.NORM_KERNEL_TOL and np.abs(alls[2] - refa[2]).max() <= R.NORM_KERNEL_TOL


# ------------------------------------------------------------------------------------------------ dither_kernel

DITHER_N = 65536
DITHER_LENS = [65536, 40000, 12345, 1000]
DITHER_AMP = 1e-3


def _dither_run(mod, base, lens, rows):
    """Run mod on a strided [rows, N] view of a copy of base [4, N + 5]; returns the whole buffer afterwards (CPU)."""
    buf = base[:rows].clone().cuda()
    view = buf[:, 2:2 + DITHER_N]
    assert view.stride(0) == DITHER_N + 5
    mod(view, torch.tensor(lens[:rows], dtype=torch.int32).cuda())
    return buf.cpu()


def test_dither_ragged_strided_rows_statistics_and_independence(hip_lib):
    """Five-sigma bounds for independent unit Gaussians over n samples: |mean| < 5 / sqrt(n), |var - 1| < 5 sqrt(2 / n),
    |lag-1 autocorrelation| < 5 / sqrt(n), |correlation of two rows| < 5 / sqrt(n).  Derived, not tuned."""
    g = torch.Generator(device="cpu").manual_seed(4500)
    base = 0.1 * torch.randn(4, DITHER_N + 5, generator=g)                  # non-zero audio, margins included

    def fresh():
        return _stacked(320, 160, 512, 80, n_frame=3, dither=DITHER_AMP)

    m = fresh()
    out = _dither_run(m, base, DITHER_LENS, 4)
    assert bool(torch.isfinite(out).all())
    # margins and samples >= lengths[b] are bit-untouched
    assert torch.equal(out[:, :2], base[:, :2]) and torch.equal(out[:, 2 + DITHER_N:], base[:, 2 + DITHER_N:])
    for b, n in enumerate(DITHER_LENS):
        assert torch.equal(out[b, 2 + n:], base[b, 2 + n:]), b
    # same call on a fresh instance: identical noise; a second call on the same instance: different noise
    assert torch.equal(_dither_run(fresh(), base, DITHER_LENS, 4), out)
    again = _dither_run(m, base, DITHER_LENS, 4)
    assert not torch.equal(again[:, 2:1002], out[:, 2:1002])
    # a row's noise depends on its index b, not on the batch around it (nor on the launch shape that batch implies)
    two = _dither_run(fresh(), base, DITHER_LENS, 2)
    assert torch.equal(two, out[:2])
    noise = ((out.double() - base.double()) / DITHER_AMP)[:, 2:2 + DITHER_N].numpy()
    unit = []
    for b, n in enumerate(DITHER_LENS):
        v = noise[b, :n]
        assert np.count_nonzero(v) > 0.99 * n                               # noise was added to the (non-zero) audio
        mean, var = v.mean(), v.var()
        lag1 = float(np.mean((v[1:] - mean) * (v[:-1] - mean)) / var)
        print("\ndither row %d n %d: mean %+.4f var %.4f lag1 %+.4f" % (b, n, mean, var, lag1))
        assert abs(mean) <= 5 / math.sqrt(n)
        assert abs(var - 1.0) <= 5 * math.sqrt(2.0 / n)
        assert abs(lag1) <= 5 / math.sqrt(n)
        unit.append((v - mean) / math.sqrt(var))
    for i in range(4):
        for j in range(i + 1, 4):
            n = min(DITHER_LENS[i], DITHER_LENS[j])
            c = float(np.mean(unit[i][:n] * unit[j][:n]))
            assert abs(c) <= 5 / math.sqrt(n), (i, j, c)
