"""Numpy fp64 oracle of blank-frame skipping (csrc/frame_skip.hip; loss.ctc_blank_skip, decode.gather_frames):
``lp_blank``, the keep decision, ``frame_map`` / ``kept`` and the gather - and ``separate``, which moves the inputs of a
test away from the decision threshold.

The device compares its fp32 ``lp_blank`` with ``float32(log(threshold))``; the oracle compares the fp64 value with the
same fp32 number.  The two decide alike wherever the fp64 value is further from the threshold than the device's error.
The project holds these fp32 row passes to an absolute 1e-4 (tests/test_ctc_gpu.py); ``MARGIN`` = 1e-3 is ten times
that, and every test asserts - as a condition on its INPUTS, not a tolerance on a result - that no frame lies inside."""
import math

import numpy as np
import torch

MARGIN = 1e-3


def f64(x):
    """The stored values of a float32 / bfloat16 torch tensor (or any array) as fp64 numpy."""
    if torch.is_tensor(x):
        return x.detach().to("cpu", torch.float64).numpy()
    return np.asarray(x, dtype=np.float64)


def log_threshold(threshold):
    """float32(log(threshold)) as the host forms it once, as a Python float."""
    return float(np.float32(math.log(float(threshold))))


def lp_blank(logits, act_lens, blank=0):
    """fp64 [B, T]: ``log_softmax(logits[b, t])[blank]`` for ``t < act_lens[b]`` (clamped to <= 0), 0 behind."""
    z = f64(logits)
    B, T, _ = z.shape
    m = z.max(axis=2)
    lp = np.minimum(z[:, :, blank] - (m + np.log(np.exp(z - m[:, :, None]).sum(axis=2))), 0.0)
    live = np.arange(T)[None, :] < np.clip(np.asarray(act_lens), 0, T)[:, None]
    return np.where(live, lp, 0.0)


def skip(logits, act_lens, threshold, blank=0):
    """(frame_map int32 [B, T], kept int32 [B], lp_blank fp64 [B, T]): frame ``t < act_lens[b]`` is kept iff
    ``lp_blank[b, t] <= float32(log(threshold))``; the kept frames' indices in ascending order, -1 behind."""
    lp = lp_blank(logits, act_lens, blank)
    B, T = lp.shape
    live = np.arange(T)[None, :] < np.clip(np.asarray(act_lens), 0, T)[:, None]
    keep = live & (lp <= log_threshold(threshold))
    frame_map = np.full((B, T), -1, dtype=np.int32)
    kept = keep.sum(axis=1).astype(np.int32)
    for b in range(B):
        frame_map[b, :kept[b]] = np.nonzero(keep[b])[0]
    return frame_map, kept, lp


def gather(enc, frame_map, kept, Tc):
    """numpy [B, Tc, P] of enc's dtype: ``enc[b, frame_map[b, j]]`` for ``j < kept[b]``, zeros behind."""
    enc = np.asarray(enc)
    B, _, P = enc.shape
    out = np.zeros((B, Tc, P), dtype=enc.dtype)
    for b in range(B):
        n = min(int(kept[b]), Tc)
        out[b, :n] = enc[b, frame_map[b, :n]]
    return out


def in_margin(logits, act_lens, threshold, blank=0, margin=MARGIN):
    """bool [B, T]: the frames ``t < act_lens[b]`` whose fp64 ``lp_blank`` lies within ``margin`` of the threshold."""
    lp = lp_blank(logits, act_lens, blank)
    T = lp.shape[1]
    live = np.arange(T)[None, :] < np.clip(np.asarray(act_lens), 0, T)[:, None]
    return live & (np.abs(lp - log_threshold(threshold)) <= margin)


def separate(logits, act_lens, threshold, blank=0, margin=MARGIN, max_rounds=200):
    """A copy of ``logits`` (a float32 / bfloat16 CPU tensor [B, T, V]) in which no frame is inside the margin: every
    frame that is gets its blank logit moved by 1.0 AWAY from the threshold (down where the frame is kept, up where it
    is dropped - unless the margin reaches ``lp_blank = 0``, then down as well), the tensor is stored in its dtype again - so a bfloat16 tensor is judged on its rounded values - and
    the check repeats until no frame is left.  A move changes ``lp_blank`` by at least ``(1 - p_blank) (1 - 1 / e)``
    towards its side, so the loop ends; ``max_rounds`` turns a failure to into an error."""
    out = logits.detach().clone()
    thr = log_threshold(threshold)
    for _ in range(max_rounds):
        near = in_margin(out, act_lens, threshold, blank, margin)
        if not near.any():
            return out
        lp = lp_blank(out, act_lens, blank)
        # (a threshold so close to 1 that the margin reaches lp = 0 leaves no room above it: every move goes down)
        step = np.where((lp <= thr) | (thr + margin >= 0.0), -1.0, 1.0) * near
        col = f64(out[:, :, blank]) + step
        out[:, :, blank] = torch.from_numpy(col).to(out.dtype)
    raise RuntimeError("separate: frames are still inside the margin after %d rounds" % max_rounds)
