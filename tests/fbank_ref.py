"""float64 restatement of the log-mel front-end, shared by test_fbank_ref_host.py and test_fbank_edges_gpu.py (test-local
code, never imported by the product path).

What csrc/fbank.hip computes, written a second time with nothing in common but the definition:

    y[0] = x[0], y[n] = x[n] - a x[n-1]                         pre-emphasis, a = preemph as given (a double)
    frame f covers y[f hop - n_fft/2 + i], i < n_fft            reflect padding WITHOUT edge repeat (index -n -> n,
                                                                N-1+n -> N-1-n), as torch.stft(center=True)
    window of win_length centred in n_fft at (n_fft - win)//2   zero outside
    P[k] = |sum_i frame[i] exp(-2 pi i k / n_fft)|^2            a DIRECT DFT: cos/sin matrix product, no FFT
    mel[m] = sum_k fb[m, k] P[k];  optional log(mel + 1e-20)
    frames f >= min(1 + N_b // hop, ceil(len_b / hop)) are 0    get_seq_len masking
    stacking of k consecutive frames, zero-padded or truncated  Downsample

Everything is float64, but the TABLES are the module's own float32 ``window`` and ``fb`` buffers, cast up: the kernel
and the reference then differ by arithmetic only (with an fp64 Hann window an impulse next to a window edge makes a
correct fp32 implementation look 1e-4 wrong).  The pre-emphasis coefficient is NOT shared: it is the constructor's double,
so rounding it to float32 counts as error of the fp32 implementation, oracle and kernel alike.  Only a DC input sees it:
its pre-emphasised level x (1 - a) moves by 9.5e-7 relative, its energies by 1.9e-6, which is inside the oracle's figure
below (there it partly cancels the rounding of a * x) and inside the kernel's tolerance.

Three input modes, as the kernel has them:
    whole row                   lengths=None
    row ENDS at lengths[b]      lengths given, mask_only=False   (reflection happens at lengths[b] - 1)
    parts mode                  lengths given, mask_only=True    (lengths only masks frames; ``n_signal`` zeroes the
                                                                  pre-emphasised samples at and past it)

The error measure of both test files is the FRAME-RELATIVE error in the linear (pre-log) mel domain,

    e = max over live frames f and mel rows m of |got[m, f] - ref[m, f]| / max_m ref[m, f],

a frame being live when its float64 peak is > 0; a dead frame (all-zero input) must come out as exactly 0.
"""
import math

import numpy as np
import torch

SAMPLE_RATE = 16000
LOG_FLOOR = 1e-20

# Worst frame-relative error of the CPU fp32 oracle (oracle.features_ref.log_fbank(log=False): torch.stft) against this
# file over SIGNAL_NAMES x GEOMETRIES.  test_fbank_ref_host.py re-measures it on every run, prints it and asserts it.
# measured: 8.468e-7 (dc at win 400 / n_fft 512); per signal noise 3.4e-7, tones 2.7e-7, impulse 2.8e-7, clipped 3.1e-7
FBANK_ORACLE_ERR = 8.5e-7
# The kernel's bound is tied to the oracle's error, never to the kernel's own: a radix-2 FFT with tabulated fp32
# twiddles has 6 to 11 stages whose error grows like log2(n_fft) * eps, the oracle's library FFT grows more slowly; 8 is
# of the order of the stage count.
FBANK_KERNEL_TOL = 8 * FBANK_ORACLE_ERR

# Worst |oracle fp32 normalize_batch - normalize_batch64| over the NORM_SEQ cases below, frame_splicing 1 and 3, on the same fp32 features (normalised
# features are O(1), so this is absolute); constant rows excluded.  Re-measured, printed and asserted like the above.
# measured: 1.230e-5 (per_feature, n = 2 frames: the fp32 difference of two nearly equal log-energies)
NORM_ORACLE_ERR = 1.25e-5
NORM_KERNEL_TOL = 8 * NORM_ORACLE_ERR

# (N, win_length, hop_length, n_fft, n_mels)
GEOMETRIES = [
    (4000, 320, 160, 512, 80),      # the trainer's / bench's geometry; hop | N: last frame masked
    (4001, 400, 160, 512, 64),
    (3000, 64, 32, 64, 16),         # smallest n_fft (half a wave of butterflies per stage), window == n_fft
    (2600, 200, 80, 256, 40),
    (5000, 1024, 256, 1024, 128),   # two passes of the mel loop
    (9000, 2048, 512, 2048, 80),    # exactly 64 KiB of dynamic LDS
    (300, 320, 160, 512, 80),       # n_fft/2 < N < n_fft: both reflections in one frame
    (257, 320, 100, 512, 80),       # the smallest N torch.stft accepts at n_fft = 512
    (1280, 401, 160, 512, 80),      # odd n_fft - win: off-centre window
]

SIGNAL_NAMES = ("noise", "tone_offbin", "tone_onbin", "dc", "impulse", "half_silent", "zeros", "clipped",
                "noise_x3000", "noise_x1e-6")


def signals(N, seed=0):
    """float32 [len(SIGNAL_NAMES), N]: one row per signal, so that one launch runs them all."""
    g = torch.Generator(device="cpu").manual_seed(4100 + seed)
    z = torch.randn(4, N, generator=g)
    t = torch.arange(N, dtype=torch.float64) / SAMPLE_RATE
    half = torch.cat([torch.zeros(N // 2), 0.1 * z[1, N // 2:]])
    imp = torch.zeros(N)
    imp[N // 2] = 1.0
    rows = [0.1 * z[0],
            (0.9 * torch.sin(2 * math.pi * 1234.5 * t)).float(),
            (0.5 * torch.sin(2 * math.pi * 1000.0 * t)).float(),
            torch.full((N,), 0.3),
            imp,
            half,
            torch.zeros(N),
            (3.0 * torch.sin(2 * math.pi * 440.0 * t)).clamp(-1.0, 1.0).float(),
            3000.0 * z[2],
            1e-6 * z[3]]
    assert len(rows) == len(SIGNAL_NAMES)
    return torch.stack(rows).contiguous()


_DFT = {}


def _dft(n_fft):
    if n_fft not in _DFT:
        n = np.arange(n_fft, dtype=np.int64)[:, None]
        k = np.arange(n_fft // 2 + 1, dtype=np.int64)[None, :]
        ang = (2.0 * np.pi / n_fft) * ((n * k) % n_fft)       # reduced before the multiply: exact periodicity
        _DFT[n_fft] = (np.cos(ang), np.sin(ang))
    return _DFT[n_fft]


def _np64(t):
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().double().numpy()
    return np.asarray(t, dtype=np.float64)


def centred_window(window, n_fft):
    w = _np64(window).reshape(-1)
    lo = (n_fft - len(w)) // 2
    full = np.zeros(n_fft)
    full[lo:lo + len(w)] = w
    return full


def _power_frames(y, n_live, win_full, hop, n_fft):
    """y: float64 pre-emphasised row (its length is where the reflection happens) -> [n_live, n_fft/2+1] power."""
    Nb, half = len(y), n_fft // 2
    idx = np.arange(n_live)[:, None] * hop - half + np.arange(n_fft)[None, :]
    idx = np.where(idx < 0, -idx, idx)
    idx = np.where(idx >= Nb, 2 * (Nb - 1) - idx, idx)
    used = (win_full != 0)[None, :]
    if np.any(((idx < 0) | (idx >= Nb)) & used):
        raise ValueError("a window tap needs a second reflection (N = %d, n_fft = %d): not defined by torch.stft" % (Nb, n_fft))
    fr = y[np.where(used, idx, 0)] * win_full[None, :]
    C, S = _dft(n_fft)
    return (fr @ C) ** 2 + (fr @ S) ** 2


def fbank64(x, window, fb, hop, n_fft, preemph=0.97, log=False, lengths=None, mask_only=False, n_signal=None):
    """x [B, N]; window: the module's fp32 ``window`` [win_length]; fb: its fp32 ``fb`` [(1,) n_mels, n_fft/2+1]
    -> float64 [B, n_mels, 1 + N // hop]."""
    x = _np64(x)
    B, N = x.shape
    fb = _np64(fb).reshape(-1, n_fft // 2 + 1)
    win_full = centred_window(window, n_fft)
    a = float(preemph) if preemph else 0.0
    out = np.zeros((B, fb.shape[0], 1 + N // hop))
    for b in range(B):
        Lb = N if lengths is None else min(int(lengths[b]), N)
        Nb = N if (lengths is None or mask_only) else Lb
        if Nb <= 0:
            continue
        live = min(1 + Nb // hop, -(-Lb // hop))
        if live <= 0:
            continue
        y = x[b, :Nb].copy()
        y[1:] -= a * x[b, :Nb - 1]
        if n_signal is not None:
            y[n_signal:] = 0.0
        mel = _power_frames(y, live, win_full, hop, n_fft) @ fb.T
        out[b, :, :live] = (np.log(mel + LOG_FLOOR) if log else mel).T
    return out


def stack64(feat, n_frame, pad_to_divisible=True):
    """[B, M, F] -> [B, T0, M * n_frame] with out[b, t, k * M + m] = feat[b, m, t * n_frame + k]."""
    feat = np.asarray(feat)
    B, M, F = feat.shape
    T0 = (F + n_frame - 1) // n_frame if pad_to_divisible else F // n_frame
    buf = np.zeros((B, M, T0 * n_frame), dtype=feat.dtype)
    keep = min(F, T0 * n_frame)
    buf[:, :, :keep] = feat[:, :, :keep]
    return buf.reshape(B, M, T0, n_frame).transpose(0, 2, 3, 1).reshape(B, T0, n_frame * M)


def normalize_batch64(x, seq_len, hop, mode):
    """x [B, rows, F] (any float) -> float64: mean / UNBIASED std over the first n_b = min(ceil(len_b / hop), F) frames,
    per row ('per_feature') or over all rows ('all_features'), (x - mean) / (std + 1e-5) on those frames, 0 after them.
    One sample (n_b = 1 per row) has no unbiased std: NaN, as torch.std gives."""
    x = _np64(x)
    B, R, F = x.shape
    out = np.zeros_like(x)
    for b in range(B):
        n = min(-(-int(seq_len[b]) // hop), F)
        if n <= 0:
            continue
        v = x[b, :, :n]
        if mode == "per_feature":
            mean = v.mean(axis=1, keepdims=True)
            std = np.sqrt(((v - mean) ** 2).sum(axis=1, keepdims=True) / (n - 1)) if n > 1 else np.full((R, 1), np.nan)
        elif mode == "all_features":
            mean = v.mean()
            std = np.sqrt(((v - mean) ** 2).sum() / (v.size - 1)) if v.size > 1 else np.nan
        else:
            out[b, :, :n] = v
            continue
        out[b, :, :n] = (v - mean) / (std + 1e-5)
    return out


def parts64(m, x, seq_len, normalize=None):
    """The parts twin (``forward(x, seq_len)``) of module ``m`` in float64, from m's own buffers and attributes:
    inputs shorter than n_fft are zero-padded to win_length AFTER the pre-emphasis, seq_len only masks, the feature rows
    are repeated frame_splicing times, then normalisation, then padding of the frame axis."""
    x = _np64(x)
    B, N = x.shape
    n_signal = None
    if N < m.n_fft:
        assert N <= m.win_length
        x = np.concatenate([x, np.zeros((B, m.win_length - N))], axis=1)
        n_signal = N
    feat = fbank64(x, m.window, m.fb, m.hop_length, m.n_fft, m.preemph, bool(m.log), lengths=seq_len, mask_only=True,
                   n_signal=n_signal)
    feat = np.concatenate([feat] * m.frame_splicing, axis=1)
    feat = normalize_batch64(feat, seq_len, m.hop_length, m.normalize if normalize is None else normalize)
    F = feat.shape[-1]
    if m.pad_to < 0:
        Fp = max(m.max_length, F)
    elif m.pad_to > 0:
        Fp = F + m.pad_to - F % m.pad_to
    else:
        Fp = F
    return np.concatenate([feat, np.zeros((B, feat.shape[1], Fp - F))], axis=2)


def frame_rel_err(got, ref):
    """Worst frame-relative error of got against the float64 ref, both [B, M, F] linear mel energies; live frames only."""
    got, ref = _np64(got), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    peak = ref.max(axis=1)
    live = peak > 0
    if not live.any():
        return 0.0
    err = np.abs(got - ref).max(axis=1)
    return float((err[live] / peak[live]).max())


def dead_frames_exact(got, ref):
    """True when every frame whose float64 reference is all zero is exactly zero in got."""
    got = _np64(got)
    dead = np.asarray(ref).max(axis=1) <= 0
    return bool(np.all(got.transpose(0, 2, 1)[dead] == 0))


# feat_normalize cases on the geometry sr 16000 / win 320 / hop 160 / n_fft 512 / 64 mels with N = 48000 samples
# (301 frames): ragged seq_len whose frame counts n = ceil(len / hop) are 2, 3, 255, 256, 257 and the full length,
# so that with all_features rows * n falls on both sides of the kernel's 256-thread stride and with per_feature n does.
NORM_N = 48000
NORM_HOP = 160
NORM_SEQ = [2 * 160, 3 * 160 - 1, 255 * 160 - 7, 256 * 160, 257 * 160 - 100, NORM_N]
NORM_FRAMES = [2, 3, 255, 256, 257, 300]


def norm_wave(seed=0):
    g = torch.Generator(device="cpu").manual_seed(4200 + seed)
    return 0.1 * torch.randn(len(NORM_SEQ), NORM_N, generator=g)
