"""RNN-T loss operator backed by the hand-written gfx950 kernels in csrc/rnnt_loss.hip.

Mirrors the call surface of ``warprnnt_pytorch.RNNTLoss`` as the reference uses it
(``rnnt/models.py:221,238``; ``cli/lightning.py:40,91``)::

    loss_fn = RNNTLoss(blank=0)
    loss = loss_fn(acts, labels, act_lens, label_lens)      # Tensor[1], differentiable wrt acts

* ``acts``        float32 / bfloat16 ``[B, T, U+1, V]`` raw logits, contiguous
* ``labels``      int32 ``[B, U]``
* ``act_lens``    int32 ``[B]``, ``max == T``
* ``label_lens``  int32 ``[B]``, ``max == U``

Difference from upstream that is deliberate: upstream computes the full gradient tensor in
``forward`` and rescales it by ``grad_output`` in ``backward`` (a second pass over
``B*T*(U+1)*V`` elements).  Here ``forward`` only fills the small alpha/beta workspace and
``backward`` writes the already-scaled gradient once.

``fastemit_lambda`` (FastEmit, Yu et al. 2021; the argument of the same name of the warp-transducer
forks) scales the gradient that flows through the label emissions by ``1 + lambda``.  The returned
costs stay the plain negative log-likelihood: only the gradient changes.  ``rnnt_align`` is the forced
aligner over the same lattice (the frames on which a known transcript is emitted).

``windows=(lo, hi)`` (alignment-restricted RNN-T, Mahadeokar et al. 2021): int32 ``[B, U]`` device tensors; label ``u``
of utterance ``b`` may be emitted only on the frames ``lo[b, u] <= t <= hi[b, u]`` and the loss sums over the alignments
that respect every window (entries behind ``label_lens[b]`` are ignored, blanks are never restricted, values outside
``[0, T_b)`` match no frame).  Windows that admit no alignment give that utterance the cost ``+inf`` and a zero
gradient - a ``'mean'`` or ``'sum'`` reduction is then ``+inf`` as well - decided on the device, without a host sync.
``alignment_windows`` builds windows from an alignment (``rnnt_align``'s frames, or an outside aligner's),
``rnnt_band`` the table of lattice cells that stay alive under them, ``rnnt_band_plan`` the row layout that packs the
joint and the loss onto those cells (``BandPlan``; used by ``Transducer.forward`` under ``config.BAND_LATTICE``).

``CTCLoss`` / ``ctc_greedy`` (csrc/ctc_loss.hip) are the loss and the greedy decoder of the encoder's CTC auxiliary head
(``Transducer(ctc_weight=...)``): raw head logits ``[B, T, V]``, not in the reference.  ``ctc_prefix_beam``
(csrc/ctc_decode.hip) searches the same logits with a beam: ranked N-best prefixes with token frames, optionally biased
towards a phrase list (``bias.ContextGraph``).  ``ctc_blank_skip`` (csrc/frame_skip.hip) marks the frames whose blank
posterior is at most a threshold and compacts their indices: the front of ``decode.skip_blank_frames``.
``ctc_align`` (csrc/ctc_loss.hip) is the head's forced aligner - Viterbi over the loss's lattice: per label the first and
the last frame of the best path, from the encoder alone.  Its ``frames`` are an "outside aligner's" for
``alignment_windows`` (``Transducer.ctc_windows``): windows for the restricted RNN-T loss that need no trained joint.
``ctc_score_nbest`` (csrc/ctc_score.hip) scores N-best lists with the head: the CTC log-likelihood of up to 32
hypotheses per utterance, one log-sum-exp per frame shared by all of them, no lattice plane stored - the device side of
``decode.ctc_rescore``.

``SoftmaxNLLLoss`` / ``softmax_nll_rows`` (csrc/lm_loss.hip) are the language model's loss and sentence scorer:
``log_softmax`` + ``NLLLoss(ignore_index)`` on raw logits ``[M, V]``, the gradient written into the logits in place.

``mwer_risk`` / ``MWERLoss`` (csrc/mwer.hip) are the risk layer of minimum word error rate training: the expected number
of errors of an N-best list under the list's own renormalised posterior, differentiable in the hypotheses' costs.
``mwer_rows`` packs the lists for the two consumers of one upload - the lattice batch whose per-row costs the packed
joint returns, and ``metrics.edit_distance``; ``Transducer.mwer_loss`` puts the pieces together.
"""
import collections
import ctypes
import math

import numpy as np
import torch

from . import _lib


def _certify_inputs(acts, labels, act_lens, label_lens, check_lengths):
    # same error classes / wording style as warprnnt_pytorch.certify_inputs
    if acts.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("acts must be float32 or bfloat16, got %s" % acts.dtype)
    for name, t in (("labels", labels), ("act_lens", act_lens), ("label_lens", label_lens)):
        if t.dtype != torch.int32:
            raise TypeError("%s must be int32, got %s" % (name, t.dtype))
    for name, t in (("acts", acts), ("labels", labels), ("act_lens", act_lens),
                    ("label_lens", label_lens)):
        if not t.is_contiguous():
            raise ValueError("%s must be contiguous" % name)
    if acts.dim() != 4:
        raise ValueError("acts must have 4 dimensions [B,T,U+1,V], got %d" % acts.dim())
    if labels.dim() != 2:
        raise ValueError("labels must have 2 dimensions [B,U], got %d" % labels.dim())
    if act_lens.dim() != 1 or label_lens.dim() != 1:
        raise ValueError("act_lens and label_lens must have 1 dimension")
    B, T, U1, _ = acts.shape
    if act_lens.shape[0] != B:
        raise ValueError("must have a length per example (act_lens has %d, batch is %d)"
                         % (act_lens.shape[0], B))
    if label_lens.shape[0] != B or labels.shape[0] != B:
        raise ValueError("must have a label length per example")
    if labels.shape[1] != U1 - 1:
        raise ValueError("Output length mismatch: labels has U=%d but acts has U+1=%d"
                         % (labels.shape[1], U1))
    if check_lengths:  # one host sync, exactly what upstream does
        if int(act_lens.max()) != T:
            raise ValueError("Input length mismatch")
        if int(label_lens.max()) != U1 - 1:
            raise ValueError("Output length mismatch")


def check_windows(windows, B, U, device, name="windows"):
    """``windows`` as the loss takes them: a pair ``(lo, hi)`` of contiguous int32 ``[B, U]`` tensors on ``device``.
    Returns the pair; TypeError / ValueError otherwise (the classes ``_certify_inputs`` uses for the labels)."""
    if not isinstance(windows, (tuple, list)) or len(windows) != 2:
        raise TypeError("%s must be a pair (lo, hi) of int32 [B, U] tensors" % name)
    lo, hi = windows
    for part, t in (("lo", lo), ("hi", hi)):
        if not torch.is_tensor(t):
            raise TypeError("%s %s must be a tensor, got %s" % (name, part, type(t).__name__))
        if t.dtype != torch.int32:
            raise TypeError("%s %s must be int32, got %s" % (name, part, t.dtype))
        if t.dim() != 2 or t.shape[0] != B or t.shape[1] != U:
            raise ValueError("%s %s must have shape [B,U] = [%d,%d], got %s" % (name, part, B, U, tuple(t.shape)))
        if not t.is_contiguous():
            raise ValueError("%s %s must be contiguous" % (name, part))
        if t.device != device:
            raise ValueError("%s %s must be on %s, got %s" % (name, part, device, t.device))
    return lo, hi


def check_fastemit_lambda(value):
    """``float(value)``; ValueError unless it is finite and >= 0."""
    lam = float(value)
    if not (lam >= 0.0 and math.isfinite(lam)):
        raise ValueError("fastemit_lambda must be finite and >= 0, got %r" % (value,))
    return lam


class _RNNTLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, acts, labels, act_lens, label_lens, blank, reduction, fastemit_lambda=0.0, win_lo=None,
                win_hi=None):
        _lib.require_cuda(acts, labels, act_lens, label_lens, win_lo, win_hi)
        B, T, U1, V = acts.shape
        lib = _lib.load()
        ws = torch.empty(lib.edgedict_rnnt_workspace_bytes(B, T, U1), dtype=torch.uint8,
                         device=acts.device)
        costs = torch.empty(B, dtype=torch.float32, device=acts.device)
        reduced = torch.empty(1, dtype=torch.float32, device=acts.device)
        scale = 1.0 / B if reduction == "mean" else 1.0
        if win_lo is None:
            _lib.call("rnnt_loss_forward", acts, _lib.dtype_code(acts.dtype), labels, act_lens,
                      label_lens, B, T, U1, V, int(blank), costs, reduced, float(scale), ws)
        else:
            _lib.call("rnnt_loss_forward_ar", acts, _lib.dtype_code(acts.dtype), labels, act_lens, label_lens,
                      win_lo, win_hi, B, T, U1, V, int(blank), costs, reduced, float(scale), ws)
        ctx.save_for_backward(acts, labels, act_lens, label_lens, ws)
        ctx.restricted = win_lo is not None
        ctx.blank = int(blank)
        ctx.reduction = reduction
        ctx.fastemit_lambda = float(fastemit_lambda)
        ctx.costs = costs
        return costs if reduction == "none" else reduced

    @staticmethod
    def backward(ctx, grad_output):
        acts, labels, act_lens, label_lens, ws = ctx.saved_tensors
        B, T, U1, V = acts.shape
        grads = torch.empty_like(acts)
        go = grad_output.contiguous().float()
        host_scale = 1.0 / B if ctx.reduction == "mean" else 1.0
        stride = 1 if ctx.reduction == "none" else 0
        if ctx.restricted:
            # (the windows are in the workspace: masked label log-probabilities are -inf there)
            _lib.call("rnnt_loss_backward_ar", acts, _lib.dtype_code(acts.dtype), grads, labels,
                      act_lens, label_lens, B, T, U1, V, ctx.blank, ws, float(host_scale), go, stride,
                      ctx.fastemit_lambda)
        elif ctx.fastemit_lambda == 0.0:
            _lib.call("rnnt_loss_backward", acts, _lib.dtype_code(acts.dtype), grads, labels,
                      act_lens, label_lens, B, T, U1, V, ctx.blank, ws, float(host_scale), go, stride)
        else:
            _lib.call("rnnt_loss_backward_fe", acts, _lib.dtype_code(acts.dtype), grads, labels,
                      act_lens, label_lens, B, T, U1, V, ctx.blank, ws, float(host_scale), go, stride,
                      ctx.fastemit_lambda)
        return grads, None, None, None, None, None, None, None, None


class RNNTLoss(torch.nn.Module):
    """Drop-in for ``warprnnt_pytorch.RNNTLoss``.

    ``reduction``: ``'mean'`` (default; ``sum_b cost_b / B`` with shape ``(1,)``), ``'sum'``
    (shape ``(1,)``) or ``'none'`` (shape ``(B,)``).

    ``fastemit_lambda`` >= 0 (default 0: the plain loss, bit for bit): FastEmit regularisation.  The
    gradient through the label emissions is scaled by ``1 + lambda``; the returned value stays the plain
    negative log-likelihood, so losses are comparable across lambdas.

    ``forward(..., windows=(lo, hi))`` (keyword only; default ``None``: the plain loss, the same kernels as before) is
    the alignment-restricted loss of the module docstring.  An utterance whose windows admit no alignment has cost
    ``+inf`` and a zero gradient, and makes a ``'mean'`` / ``'sum'`` result ``+inf`` while the gradient of the batch
    stays finite (the other utterances' usual share): check the returned loss to drop such a step, or build windows
    that are feasible (``alignment_windows`` of a valid alignment always are).
    """

    def __init__(self, blank=0, reduction="mean", check_lengths=True, fastemit_lambda=0.0):
        super().__init__()
        if reduction not in ("mean", "sum", "none"):
            raise ValueError("reduction must be 'mean', 'sum' or 'none'")
        self.fastemit_lambda = check_fastemit_lambda(fastemit_lambda)
        self.blank = blank
        self.reduction = reduction
        self.check_lengths = check_lengths

    def forward(self, acts, labels, act_lens, label_lens, *, windows=None):
        _certify_inputs(acts, labels, act_lens, label_lens, self.check_lengths)
        if windows is None:
            return _RNNTLossFn.apply(acts, labels, act_lens, label_lens, self.blank, self.reduction,
                                     self.fastemit_lambda)
        lo, hi = check_windows(windows, labels.shape[0], labels.shape[1], acts.device)
        return _RNNTLossFn.apply(acts, labels, act_lens, label_lens, self.blank, self.reduction,
                                 self.fastemit_lambda, lo, hi)


@torch.no_grad()
def rnnt_align(acts, labels, act_lens, label_lens, blank=0, *, windows=None):
    """Forced alignment: the single most probable alignment of the transcripts ``labels`` (Viterbi over
    the lattice of the loss).  Arguments as ``RNNTLoss.forward`` (validated the same way).  Returns
    ``(frames, scores)``: ``frames`` int32 ``[B, U]``, ``frames[b, u]`` the frame on which label ``u`` of
    utterance ``b`` is emitted (non-decreasing in ``u``; -1 for ``u >= label_lens[b]``), and ``scores``
    float32 ``[B]``, the log-probability of that alignment (``<= -cost``).  Where two alignments score
    equal, the one that waits (takes the blank predecessor) wins.  ``windows=(lo, hi)`` (as ``RNNTLoss.forward``): the
    best alignment among those that respect the windows; a row whose windows admit none has score ``-inf`` and frames
    of all -1."""
    _certify_inputs(acts, labels, act_lens, label_lens, True)
    _lib.require_cuda(acts, labels, act_lens, label_lens)
    B, T, U1, V = acts.shape
    lib = _lib.load()
    ws = torch.empty(lib.edgedict_rnnt_workspace_bytes(B, T, U1), dtype=torch.uint8, device=acts.device)
    frames = torch.empty(B, U1 - 1, dtype=torch.int32, device=acts.device)
    scores = torch.empty(B, dtype=torch.float32, device=acts.device)
    if windows is None:
        _lib.call("rnnt_align", acts.detach(), _lib.dtype_code(acts.dtype), labels, act_lens, label_lens, B, T, U1, V,
                  int(blank), frames, scores, ws)
    else:
        lo, hi = check_windows(windows, B, U1 - 1, acts.device)
        _lib.call("rnnt_align_ar", acts.detach(), _lib.dtype_code(acts.dtype), labels, act_lens, label_lens, lo, hi,
                  B, T, U1, V, int(blank), frames, scores, ws)
    return frames, scores


def _check_lens(act_lens, label_lens, B, device):
    for name, t in (("act_lens", act_lens), ("label_lens", label_lens)):
        if not torch.is_tensor(t) or t.dtype != torch.int32 or t.dim() != 1 or t.shape[0] != B:
            raise ValueError("%s must be an int32 tensor of shape [%d]" % (name, B))
        if not t.is_contiguous() or t.device != device:
            raise ValueError("%s must be contiguous and on %s" % (name, device))


@torch.no_grad()
def alignment_windows(frames, act_lens, label_lens, left, right):
    """Windows for ``RNNTLoss.forward(..., windows=)`` around an alignment: ``frames`` int32 ``[B, U]`` as ``rnnt_align``
    returns them (device), ``left``, ``right`` >= 0 frames of slack.  Returns ``(lo, hi)`` with
    ``lo = max(0, f - left)``, ``hi = min(T_b - 1, f + right)``; behind ``label_lens[b]``: ``lo = 0, hi = T - 1`` with
    ``T = max(act_lens)``, found on the device.  One small kernel, no host sync."""
    if not torch.is_tensor(frames) or frames.dtype != torch.int32 or frames.dim() != 2 or not frames.is_contiguous():
        raise ValueError("frames must be a contiguous int32 tensor [B, U]")
    left, right = int(left), int(right)
    if left < 0 or right < 0:
        raise ValueError("left and right must be >= 0, got %d, %d" % (left, right))
    _lib.require_cuda(frames, act_lens, label_lens)
    B, U = frames.shape
    _check_lens(act_lens, label_lens, B, frames.device)
    lo = torch.empty_like(frames)
    hi = torch.empty_like(frames)
    _lib.call("rnnt_alignment_windows", frames, act_lens, label_lens, B, 0, U, left, right, lo, hi)
    return lo, hi


@torch.no_grad()
def rnnt_band(lo, hi, act_lens, label_lens, T):
    """The lattice cells that stay alive under the windows ``(lo, hi)`` - those a window-respecting alignment can pass
    through, i.e. with finite alpha and finite beta - from the windows alone.  Returns ``(band, cells)``: ``band``
    int32 ``[B, T, 2]``, ``band[b, t] = (first, last)`` live label column of frame ``t`` (``(0, -1)`` where the frame
    has none: behind ``act_lens[b]``, or everywhere when the windows admit no alignment), and ``cells`` int64 ``[B]``,
    the number of live cells.  One small kernel, no host sync."""
    if not torch.is_tensor(lo):
        raise TypeError("lo must be a tensor")
    B, U = lo.shape[0], lo.shape[1] if lo.dim() == 2 else -1
    lo, hi = check_windows((lo, hi), B, U, lo.device)
    _lib.require_cuda(lo, hi, act_lens, label_lens)
    _check_lens(act_lens, label_lens, B, lo.device)
    T = int(T)
    band = torch.empty(B, T, 2, dtype=torch.int32, device=lo.device)
    cells = torch.empty(B, dtype=torch.int64, device=lo.device)
    _lib.call("rnnt_band", lo, hi, act_lens, label_lens, B, T, U + 1, band, cells)
    return band, cells


class BandPlan:
    """Row layout of the band-packed lattice: only the live cells of the band table exist as rows of the joint's
    ``[M_band, .]`` matrices, ``row(b, t, u) = row_off[b, t] + (u - ulo[b, t])`` for ``ulo <= u <= uhi``.

    ``band`` int32 ``[B, T, 2]`` and ``cells`` int64 ``[B]`` as ``rnnt_band`` returns them, ``row_off`` int64 ``[B, T]``
    (exclusive prefix sum of the frame widths in ``(b, t)`` order), ``row_tu`` int32 ``[M_band]`` (``t << 16 | u`` of
    every row) and ``rows``, the host int ``M_band = cells.sum()``.  ``rows`` and ``row_tu`` exist after ``finish()``:
    the band table and the scan are device work, the total reaches the host through one asynchronous copy into pinned
    memory, and ``finish()`` waits for the event recorded behind that copy only - work enqueued after the plan was
    started (the encoder) is not waited for."""

    def __init__(self, band, cells, row_off, total_host, event, U1):
        self.band, self.cells, self.row_off = band, cells, row_off
        self.row_tu = None
        self.rows = None
        self.U1 = U1
        self._total_host, self._event = total_host, event

    def wait(self):
        """The one host read: wait for the event behind the copy of the total.  Returns ``M_band``."""
        self._event.synchronize()
        return int(self._total_host.item())

    def finish(self):
        """``wait()``, then fill ``row_tu`` on the current stream.  Returns ``self``."""
        if self.rows is None:
            self.rows = self.wait()
            B, T = self.band.shape[0], self.band.shape[1]
            self.row_tu = torch.empty(self.rows, dtype=torch.int32, device=self.band.device)
            if self.rows:
                _lib.call("rnnt_band_rows", self.band, self.row_off, B, T, self.U1, ctypes.c_longlong(self.rows),
                          self.row_tu)
        return self


@torch.no_grad()
def rnnt_band_plan(lo, hi, act_lens, label_lens, T, *, finish=True):
    """``BandPlan`` of the windows ``(lo, hi)`` (arguments as ``rnnt_band``; the lengths on the device).  Device work
    plus exactly one host read, which depends on the windows and the lengths only.  ``finish=False`` returns right
    behind the asynchronous copy of the total - enqueue other work, then call ``plan.finish()``."""
    band, cells = rnnt_band(lo, hi, act_lens, label_lens, T)
    B, T, U1 = band.shape[0], band.shape[1], lo.shape[1] + 1
    if T >= 65536 or U1 >= 65536:
        raise ValueError("rnnt_band_plan: T and U + 1 must be below 65536 (got %d, %d)" % (T, U1))
    row_off = torch.empty(B, T, dtype=torch.int64, device=band.device)
    total = torch.empty(1, dtype=torch.int64, device=band.device)
    _lib.call("rnnt_band_offsets", band, cells, B, T, row_off, total)
    total_host = torch.empty(1, dtype=torch.int64, pin_memory=True)
    total_host.copy_(total, non_blocking=True)
    event = torch.cuda.Event()
    event.record()
    plan = BandPlan(band, cells, row_off, total_host, event, U1)
    return plan.finish() if finish else plan


def rnnt_loss_debug(acts, labels, act_lens, label_lens, blank=0, *, windows=None):
    """Test hook: run forward and return (costs, denominators, alphas, betas, loglikes[B,2])."""
    _lib.require_cuda(acts)
    B, T, U1, V = acts.shape
    lib = _lib.load()
    nbytes = lib.edgedict_rnnt_workspace_bytes(B, T, U1)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=acts.device)
    costs = torch.empty(B, dtype=torch.float32, device=acts.device)
    if windows is None:
        _lib.call("rnnt_loss_forward", acts, _lib.dtype_code(acts.dtype), labels, act_lens,
                  label_lens, B, T, U1, V, int(blank), costs, None, 1.0, ws)
    else:
        lo, hi = check_windows(windows, B, U1 - 1, acts.device)
        _lib.call("rnnt_loss_forward_ar", acts, _lib.dtype_code(acts.dtype), labels, act_lens, label_lens, lo, hi,
                  B, T, U1, V, int(blank), costs, None, 1.0, ws)
    base = ws.data_ptr()

    def view(which, shape, dtype):
        p = lib.edgedict_rnnt_workspace_view(_lib.ptr(ws), B, T, U1, which)
        esz = 8 if dtype == torch.float64 else 4
        off = (p - base) // esz
        n = 1
        for s in shape:
            n *= s
        return ws.view(dtype)[off:off + n].view(*shape).clone()

    return (costs, view(0, (B, T, U1), torch.float32), view(1, (B, T, U1), torch.float64),
            view(2, (B, T, U1), torch.float64), view(3, (B, 2), torch.float64))


# ------------------------------------------------------------------------------------------------ CTC
# The auxiliary head's loss (csrc/ctc_loss.hip): raw head logits [B, T, V], the extended sequence of 2 U + 1 states.


def _certify_ctc_inputs(logits, labels, act_lens, label_lens, check_lengths):
    # error classes / wording of _certify_inputs
    if logits.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("logits must be float32 or bfloat16, got %s" % logits.dtype)
    for name, t in (("labels", labels), ("act_lens", act_lens), ("label_lens", label_lens)):
        if t.dtype != torch.int32:
            raise TypeError("%s must be int32, got %s" % (name, t.dtype))
    for name, t in (("logits", logits), ("labels", labels), ("act_lens", act_lens), ("label_lens", label_lens)):
        if not t.is_contiguous():
            raise ValueError("%s must be contiguous" % name)
    if logits.dim() != 3:
        raise ValueError("logits must have 3 dimensions [B,T,V], got %d" % logits.dim())
    if labels.dim() != 2:
        raise ValueError("labels must have 2 dimensions [B,U], got %d" % labels.dim())
    if act_lens.dim() != 1 or label_lens.dim() != 1:
        raise ValueError("act_lens and label_lens must have 1 dimension")
    B, T, _ = logits.shape
    if act_lens.shape[0] != B:
        raise ValueError("must have a length per example (act_lens has %d, batch is %d)" % (act_lens.shape[0], B))
    if label_lens.shape[0] != B or labels.shape[0] != B:
        raise ValueError("must have a label length per example")
    if check_lengths:  # one host sync, as _certify_inputs
        if int(act_lens.max()) != T:
            raise ValueError("Input length mismatch")
        if int(label_lens.max()) != labels.shape[1]:
            raise ValueError("Output length mismatch")


class _CTCLossFn(torch.autograd.Function):
    """The shape of ``_RNNTLossFn``: forward fills the workspace, backward writes the scaled gradient once."""

    @staticmethod
    def forward(ctx, logits, labels, act_lens, label_lens, blank, reduction, zero_infinity):
        _lib.require_cuda(logits, labels, act_lens, label_lens)
        B, T, V = logits.shape
        U = labels.shape[1]
        lib = _lib.load()
        ws = torch.empty(lib.edgedict_ctc_workspace_bytes(B, T, U), dtype=torch.uint8, device=logits.device)
        costs = torch.empty(B, dtype=torch.float32, device=logits.device)
        reduced = torch.empty(1, dtype=torch.float32, device=logits.device)
        scale = 1.0 / B if reduction == "mean" else 1.0
        _lib.call("ctc_loss_forward", logits, _lib.dtype_code(logits.dtype), labels if U else None, act_lens,
                  label_lens, B, T, U, V, int(blank), bool(zero_infinity), costs, reduced, float(scale), ws)
        ctx.save_for_backward(logits, labels, act_lens, label_lens, ws)
        ctx.blank = int(blank)
        ctx.reduction = reduction
        ctx.costs = costs
        return costs if reduction == "none" else reduced

    @staticmethod
    def backward(ctx, grad_output):
        logits, labels, act_lens, label_lens, ws = ctx.saved_tensors
        B, T, V = logits.shape
        U = labels.shape[1]
        grads = torch.empty_like(logits)
        go = grad_output.contiguous().float()
        host_scale = 1.0 / B if ctx.reduction == "mean" else 1.0
        stride = 1 if ctx.reduction == "none" else 0
        _lib.call("ctc_loss_backward", logits, _lib.dtype_code(logits.dtype), grads, labels if U else None, act_lens,
                  label_lens, B, T, U, V, ctx.blank, ws, float(host_scale), go, stride)
        return grads, None, None, None, None, None, None


class CTCLoss(torch.nn.Module):
    """CTC loss on raw logits (the auxiliary head of ``Transducer(ctc_weight=...)``).

    ``forward(logits, labels, act_lens, label_lens)``: ``logits`` float32 / bfloat16 ``[B, T, V]`` raw (NOT
    log-softmaxed) and contiguous, ``labels`` int32 ``[B, U]`` (symbols other than ``blank``), ``act_lens`` /
    ``label_lens`` int32 ``[B]``; differentiable with respect to ``logits``.  Device tensors only: there is no CPU
    fallback.

    ``reduction``: ``'mean'`` (default) is ``sum_b cost_b / B`` with shape ``(1,)`` - what ``RNNTLoss`` calls the mean,
    NOT ``torch.nn.functional.ctc_loss``'s mean, which first divides every cost by its target length; ``'sum'`` (shape
    ``(1,)``) or ``'none'`` (shape ``(B,)``).

    An utterance with no path (fewer frames than labels plus adjacent repeats) has cost ``+inf`` and a zero gradient;
    ``zero_infinity=True`` makes that cost 0 (the gradient stays zero), decided on the device without a host sync.
    ``check_lengths=True`` asks ``max(act_lens) == T`` and ``max(label_lens) == U`` (one host sync), as ``RNNTLoss``.
    """

    def __init__(self, blank=0, reduction="mean", check_lengths=True, zero_infinity=False):
        super().__init__()
        if reduction not in ("mean", "sum", "none"):
            raise ValueError("reduction must be 'mean', 'sum' or 'none'")
        self.blank = blank
        self.reduction = reduction
        self.check_lengths = check_lengths
        self.zero_infinity = bool(zero_infinity)

    def forward(self, logits, labels, act_lens, label_lens):
        _certify_ctc_inputs(logits, labels, act_lens, label_lens, self.check_lengths)
        return _CTCLossFn.apply(logits, labels, act_lens, label_lens, self.blank, self.reduction, self.zero_infinity)


@torch.no_grad()
def ctc_greedy(logits, act_lens, blank=0):
    """CTC greedy decoding of head logits ``[B, T, V]`` (float32 / bfloat16, contiguous, device): per frame
    ``t < act_lens[b]`` the arg max (lowest index on ties); a frame is kept iff its symbol is not ``blank`` and differs
    from the frame before.  Returns device tensors ``(tokens, counts, frames, neglogp)``: ``tokens`` / ``frames`` int32
    ``[B, T]`` (kept symbols and their frame indices, -1 behind ``counts[b]``), ``counts`` int32 ``[B]``, ``neglogp``
    float32 ``[B]`` (minus the summed log-probabilities of the kept frames' symbols).  No host sync."""
    if logits.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("logits must be float32 or bfloat16, got %s" % logits.dtype)
    if act_lens.dtype != torch.int32:
        raise TypeError("act_lens must be int32, got %s" % act_lens.dtype)
    if logits.dim() != 3:
        raise ValueError("logits must have 3 dimensions [B,T,V], got %d" % logits.dim())
    if not logits.is_contiguous() or not act_lens.is_contiguous():
        raise ValueError("logits and act_lens must be contiguous")
    if act_lens.dim() != 1 or act_lens.shape[0] != logits.shape[0]:
        raise ValueError("must have a length per example (act_lens has %s, batch is %d)"
                         % (tuple(act_lens.shape), logits.shape[0]))
    _lib.require_cuda(logits, act_lens)
    B, T, V = logits.shape
    dev = logits.device
    tokens = torch.empty(B, T, dtype=torch.int32, device=dev)
    frames = torch.empty(B, T, dtype=torch.int32, device=dev)
    counts = torch.empty(B, dtype=torch.int32, device=dev)
    neglogp = torch.empty(B, dtype=torch.float32, device=dev)
    scratch = torch.empty(2 * B * T, dtype=torch.int32, device=dev)
    _lib.call("ctc_greedy", logits.detach(), _lib.dtype_code(logits.dtype), act_lens, B, T, V, int(blank), tokens,
              counts, frames, neglogp, scratch)
    return tokens, counts, frames, neglogp


def check_skip_threshold(threshold):
    """The blank-skip threshold as a float in (0, 1], else ``ValueError`` (a NaN fails both comparisons)."""
    try:
        thr = float(threshold)
    except (TypeError, ValueError):
        raise ValueError("the blank-skip threshold must be a number in (0, 1], got %r" % (threshold,)) from None
    if not 0.0 < thr <= 1.0:
        raise ValueError("the blank-skip threshold must lie in (0, 1], got %r" % (threshold,))
    return thr


@torch.no_grad()
def ctc_blank_skip(logits, act_lens, threshold, blank=0):
    """Which frames of head logits ``[B, T, V]`` (float32 / bfloat16, contiguous, device) CTC is NOT sure are blank
    (csrc/frame_skip.hip): with ``lp_blank[b, t] = log_softmax(logits[b, t])[blank]`` frame ``t < act_lens[b]`` is kept
    iff ``lp_blank[b, t] <= float32(log(threshold))``, i.e. the blank holds at most ``threshold`` of the frame's mass.
    ``threshold`` in (0, 1], else ``ValueError``; 1.0 keeps every frame.  Returns device tensors
    ``(frame_map, kept, lp_blank)``: ``frame_map`` int32 ``[B, T]`` (the original index of the j-th kept frame, ascending,
    -1 behind ``kept[b]``), ``kept`` int32 ``[B]``, ``lp_blank`` float32 ``[B, T]`` (clamped to <= 0; 0 behind
    ``act_lens[b]``).  No host sync."""
    thr = check_skip_threshold(threshold)
    if logits.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("logits must be float32 or bfloat16, got %s" % logits.dtype)
    if act_lens.dtype != torch.int32:
        raise TypeError("act_lens must be int32, got %s" % act_lens.dtype)
    if logits.dim() != 3:
        raise ValueError("logits must have 3 dimensions [B,T,V], got %d" % logits.dim())
    if not logits.is_contiguous() or not act_lens.is_contiguous():
        raise ValueError("logits and act_lens must be contiguous")
    if act_lens.dim() != 1 or act_lens.shape[0] != logits.shape[0]:
        raise ValueError("must have a length per example (act_lens has %s, batch is %d)"
                         % (tuple(act_lens.shape), logits.shape[0]))
    B, T, V = logits.shape
    blank = int(blank)
    if B < 1 or T < 1:
        raise ValueError("logits must hold at least one utterance and one frame (B = %d, T = %d)" % (B, T))
    if V < 2:
        raise ValueError("V = %d: need at least the blank and one symbol" % V)
    if not 0 <= blank < V:
        raise ValueError("blank %d outside [0, %d)" % (blank, V))
    _lib.require_cuda(logits, act_lens)
    dev = logits.device
    # the comparison's right-hand side is formed once, here, in the precision the kernel compares in
    log_thr = ctypes.c_float(math.log(thr)).value
    frame_map = torch.empty(B, T, dtype=torch.int32, device=dev)
    kept = torch.empty(B, dtype=torch.int32, device=dev)
    lp_blank = torch.empty(B, T, dtype=torch.float32, device=dev)
    _lib.call("frame_skip_scan", logits.detach(), _lib.dtype_code(logits.dtype), act_lens, B, T, V, blank, log_thr,
              lp_blank, frame_map, kept)
    return frame_map, kept, lp_blank


CTC_BEAM_MAX_W = 32
CTC_BEAM_MAX_CAND = 64


@torch.no_grad()
def ctc_prefix_beam(logits, act_lens, W=10, blank=0, cand=None, bias=None, *, lm=None, lm_weight=None,
                    length_bonus=0.0):
    """CTC prefix beam search of head logits ``[B, T, V]`` (float32 / bfloat16, contiguous, device), the counterpart of
    ``ctc_greedy`` with a beam (csrc/ctc_decode.hip states the search): per frame ``t < act_lens[b]`` every prefix of
    the beam stays or is extended with one of the ``min(cand, V - 1)`` most probable non-blank tokens of the frame, a
    prefix's score is the sum over its paths (``pb`` / ``pnb``), the ``W`` best prefixes survive, ranked.

    ``W`` in 1 .. 32, ``cand`` in 1 .. 64 (default ``min(V - 1, 32)``); anything else raises ``ValueError`` naming the
    argument before a launch.  ``bias``: an ``edgedict_amd.bias.ContextGraph`` - every prefix then carries the phrase
    automaton's state and its total bias ``graph.score(tokens)``, which enters the ranking and ``logp`` only.  The
    candidate list is cut BEFORE the bias is seen: a boosted token outside a frame's top ``cand`` is not rescued.
    ``bias=None`` and an empty graph run the plain kernel.

    ``lm``: an ``edgedict_amd.ngram.NGramLM`` (a back-off n-gram in device tables; an LSTM ``LMModel`` raises
    ``TypeError``: its step cannot run inside the walk), with ``lm_weight`` (required, finite, ``>= 0``) and
    ``length_bonus`` (per token).  Every prefix then carries one LM state and the total
    ``Ln = sum (lm_weight * lm.step(...) + length_bonus)`` over its tokens, which enters the ranking and ``logp``
    beside the bias total: ``logp = (logadd(pb, pnb) + bias total) + Ln``.  No end-of-sentence term.  The candidate
    list is cut before the LM is seen as well.  ``lm=None`` calls exactly what is called without the keyword.

    Returns device tensors ``(tokens, frames, token_lp, ntok, n_hyp, logp)``: ``tokens`` / ``frames`` int32
    ``[B, W, T]`` (hypothesis h's tokens and the frame each token's node was created on; -1 behind ``ntok[b, h]``),
    ``token_lp`` float32 ``[B, W, T]`` (``log_softmax(logits[b, frame])[token]``, 0 behind), ``ntok`` int32 ``[B, W]``,
    ``n_hyp`` int32 ``[B]``, ``logp`` float64 ``[B, W]`` descending (-inf behind ``n_hyp[b]``; with a bias list it
    includes the bias total).  Entry 0 is the answer; ``act_lens[b] == 0`` gives the empty prefix with ``logp`` 0.
    No host sync."""
    from .bias import active, check_bias_args
    if logits.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("logits must be float32 or bfloat16, got %s" % logits.dtype)
    if act_lens.dtype != torch.int32:
        raise TypeError("act_lens must be int32, got %s" % act_lens.dtype)
    if logits.dim() != 3:
        raise ValueError("logits must have 3 dimensions [B,T,V], got %d" % logits.dim())
    if not logits.is_contiguous() or not act_lens.is_contiguous():
        raise ValueError("logits and act_lens must be contiguous")
    if act_lens.dim() != 1 or act_lens.shape[0] != logits.shape[0]:
        raise ValueError("must have a length per example (act_lens has %s, batch is %d)"
                         % (tuple(act_lens.shape), logits.shape[0]))
    B, T, V = logits.shape
    W, blank = int(W), int(blank)
    if B < 1 or T < 1:
        raise ValueError("logits must hold at least one utterance and one frame (B = %d, T = %d)" % (B, T))
    if V < 2:
        raise ValueError("V = %d: need at least the blank and one symbol" % V)
    if not 0 <= blank < V:
        raise ValueError("blank %d outside [0, %d)" % (blank, V))
    if not 1 <= W <= CTC_BEAM_MAX_W:
        raise ValueError("W = %d outside [1, %d]" % (W, CTC_BEAM_MAX_W))
    cand = min(V - 1, 32) if cand is None else int(cand)
    if not 1 <= cand <= CTC_BEAM_MAX_CAND:
        raise ValueError("cand = %d outside [1, %d]" % (cand, CTC_BEAM_MAX_CAND))
    check_bias_args(bias, V, False)
    from .ngram import CtcBeamOpts, check_ngram_args
    check_ngram_args(lm, lm_weight, length_bonus, V, blank)
    _lib.require_cuda(logits, act_lens)
    dev = logits.device
    graph = active(bias)
    bref = graph.ref(dev) if graph is not None else None
    lib = _lib.load()
    tokens = torch.empty(B, W, T, dtype=torch.int32, device=dev)
    frames = torch.empty(B, W, T, dtype=torch.int32, device=dev)
    token_lp = torch.empty(B, W, T, dtype=torch.float32, device=dev)
    ntok = torch.empty(B, W, dtype=torch.int32, device=dev)
    n_hyp = torch.empty(B, dtype=torch.int32, device=dev)
    logp = torch.empty(B, W, dtype=torch.float64, device=dev)
    ws = torch.empty(lib.edgedict_ctc_beam_workspace_bytes(B, T, W, cand), dtype=torch.uint8, device=dev)
    if lm is None:
        _lib.call("ctc_beam_search", logits.detach(), _lib.dtype_code(logits.dtype), act_lens, B, T, V, blank, W, cand,
                  bref, tokens, frames, token_lp, ntok, n_hyp, logp, ws)
        return tokens, frames, token_lp, ntok, n_hyp, logp
    lms = lm.struct(dev, lm_weight, length_bonus)
    opts = CtcBeamOpts()
    opts.bias = ctypes.addressof(graph.tables(dev)["struct"]) if graph is not None else None
    opts.ngram = ctypes.addressof(lms)
    _lib.call("ctc_beam_search_fused", logits.detach(), _lib.dtype_code(logits.dtype), act_lens, B, T, V, blank, W, cand,
              ctypes.byref(opts), tokens, frames, token_lp, ntok, n_hyp, logp, ws)
    return tokens, frames, token_lp, ntok, n_hyp, logp


def _ctc_align_call(logits, labels, act_lens, label_lens, blank, ws):
    B, T, V = logits.shape
    U = labels.shape[1]
    frames = torch.empty(B, U, dtype=torch.int32, device=logits.device)
    ends = torch.empty(B, U, dtype=torch.int32, device=logits.device)
    scores = torch.empty(B, dtype=torch.float32, device=logits.device)
    _lib.call("ctc_align", logits.detach(), _lib.dtype_code(logits.dtype), labels if U else None, act_lens, label_lens,
              B, T, U, V, int(blank), frames if U else None, ends if U else None, scores, ws)
    return frames, ends, scores


@torch.no_grad()
def ctc_align(logits, labels, act_lens, label_lens, blank=0, *, check_lengths=True):
    """CTC forced alignment of the transcripts ``labels`` on head logits: the single most probable path of the loss's
    lattice (Viterbi over the ``2 U + 1`` states, float64 carry on the loss's float32 log-probabilities).  Arguments as
    ``CTCLoss.forward`` (validated the same way; ``check_lengths=True`` is its one host sync).  Returns device tensors
    ``(frames, ends, scores)``: ``frames`` / ``ends`` int32 ``[B, U]``, the first and the last frame the path spends in
    label ``u``'s state (``0 <= frames[u] <= ends[u] < frames[u+1]``, ``ends[U_b-1] <= T_b - 1``; -1 behind
    ``label_lens[b]``), ``scores`` float32 ``[B]``, the path's log-probability (``<= -cost``).  ``frames`` is what
    ``alignment_windows`` and ``decode.emission_times`` take; ``frames`` and ``ends`` together are a label's span.

    Unlike the loss's lengths check, a row without a path (``act_lens[b] == 0``, or fewer frames than labels plus
    adjacent repeats) is not an error: its score is ``-inf`` and its frames and ends are all -1; the other rows are
    unaffected.  Tie rule (the later emission wins, as ``rnnt_align`` waits): the path ends in the last label's state
    when that scores at least the final blank's, and among the equally good predecessors of a state it comes from the
    label two states back (where CTC allows the skip), else from the state before, else it stays."""
    _certify_ctc_inputs(logits, labels, act_lens, label_lens, check_lengths)
    _lib.require_cuda(logits, labels, act_lens, label_lens)
    B, T, _ = logits.shape
    ws = torch.empty(_lib.load().edgedict_ctc_workspace_bytes(B, T, labels.shape[1]), dtype=torch.uint8,
                     device=logits.device)
    return _ctc_align_call(logits, labels, act_lens, label_lens, blank, ws)


def ctc_align_debug(logits, labels, act_lens, label_lens, blank=0):
    """Test hook: run ``ctc_align`` and return (frames, ends, scores, lp_blank [B,T] f32, lp_label [B,T,U] f32,
    v [B,T,2U+1] f64) - clones; entries outside an utterance's ``[T_b, U_b]`` / ``[T_b, 2 U_b + 1]`` box are zeros."""
    _lib.require_cuda(logits, labels, act_lens, label_lens)
    B, T, V = logits.shape
    U = labels.shape[1]
    lib = _lib.load()
    ws = torch.zeros(lib.edgedict_ctc_workspace_bytes(B, T, U), dtype=torch.uint8, device=logits.device)
    frames, ends, scores = _ctc_align_call(logits, labels, act_lens, label_lens, blank, ws)
    base = ws.data_ptr()

    def view(which, shape, dtype):
        p = lib.edgedict_ctc_workspace_view(_lib.ptr(ws), B, T, U, which)
        esz = 8 if dtype == torch.float64 else 4
        off = (p - base) // esz
        n = 1
        for s in shape:
            n *= s
        return ws.view(dtype)[off:off + n].view(*shape).clone()

    return (frames, ends, scores, view(4, (B, T), torch.float32), view(5, (B, T, U), torch.float32),
            view(1, (B, T, 2 * U + 1), torch.float64))


CTC_SCORE_MAX_N = 32
CTC_SCORE_MAX_U = 1023


def _certify_ctc_score_inputs(logits, act_lens, hyps, hyp_lens, n_hyp, blank):
    # error classes / wording of _certify_ctc_inputs
    if logits.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("logits must be float32 or bfloat16, got %s" % logits.dtype)
    named = (("act_lens", act_lens), ("hyps", hyps), ("hyp_lens", hyp_lens), ("n_hyp", n_hyp))
    for name, t in named:
        if t is not None and t.dtype != torch.int32:
            raise TypeError("%s must be int32, got %s" % (name, t.dtype))
    for name, t in (("logits", logits),) + named:
        if t is not None and not t.is_contiguous():
            raise ValueError("%s must be contiguous" % name)
    if logits.dim() != 3:
        raise ValueError("logits must have 3 dimensions [B,T,V], got %d" % logits.dim())
    if hyps.dim() != 3:
        raise ValueError("hyps must have 3 dimensions [B,N,U], got %d" % hyps.dim())
    if hyp_lens.dim() != 2:
        raise ValueError("hyp_lens must have 2 dimensions [B,N], got %d" % hyp_lens.dim())
    if act_lens.dim() != 1 or (n_hyp is not None and n_hyp.dim() != 1):
        raise ValueError("act_lens and n_hyp must have 1 dimension")
    B, T, V = logits.shape
    N, U = hyps.shape[1], hyps.shape[2]
    if act_lens.shape[0] != B:
        raise ValueError("must have a length per example (act_lens has %d, batch is %d)" % (act_lens.shape[0], B))
    if hyps.shape[0] != B or tuple(hyp_lens.shape) != (B, N):
        raise ValueError("must have a hypothesis length per slot (hyps is %s, hyp_lens %s, batch is %d)"
                         % (tuple(hyps.shape), tuple(hyp_lens.shape), B))
    if n_hyp is not None and n_hyp.shape[0] != B:
        raise ValueError("must have a hypothesis count per example (n_hyp has %d, batch is %d)" % (n_hyp.shape[0], B))
    if B < 1 or T < 1:
        raise ValueError("logits must hold at least one utterance and one frame (B = %d, T = %d)" % (B, T))
    if V < 2:
        raise ValueError("V = %d: need at least the blank and one symbol" % V)
    if not 0 <= blank < V:
        raise ValueError("blank %d outside [0, %d)" % (blank, V))
    if not 1 <= N <= CTC_SCORE_MAX_N:
        raise ValueError("N = %d hypotheses per utterance outside [1, %d]" % (N, CTC_SCORE_MAX_N))
    if U > CTC_SCORE_MAX_U:
        raise ValueError("U = %d exceeds the supported maximum of %d tokens per hypothesis" % (U, CTC_SCORE_MAX_U))


@torch.no_grad()
def ctc_score_nbest(logits, act_lens, hyps, hyp_lens, n_hyp=None, blank=0):
    """CTC log-likelihoods of N-best lists on head logits (csrc/ctc_score.hip): ``logits`` float32 / bfloat16
    ``[B, T, V]`` raw and contiguous, ``act_lens`` int32 ``[B]``, ``hyps`` int32 ``[B, N, U]`` (token sequences without
    blanks, ``1 <= N <= 32``, ``U <= 1023``; ``U = 0``: every hypothesis is empty), ``hyp_lens`` int32 ``[B, N]``,
    ``n_hyp`` int32 ``[B]`` (live slots per utterance; None: all ``N``).  Device tensors only.  Returns a float64
    ``[B, N]`` device tensor: ``scores[b, n]`` is the log of the total probability of all CTC paths of
    ``hyps[b, n, :hyp_lens[b, n]]`` over the frames ``t < act_lens[b]`` - minus what ``CTCLoss(reduction='none')`` costs
    that transcript, in the loss's arithmetic (float32 log-sum-exp per frame, float64 carry).  ``-inf``: a hypothesis
    without a path (``act_lens[b] == 0``, fewer frames than tokens plus adjacent repeats, a token outside ``[0, V)``)
    and every slot ``n >= n_hyp[b]``.  Tokens behind ``hyp_lens`` and slots behind ``n_hyp`` are never read.

    The frame's log-sum-exp is computed once per utterance, not once per hypothesis, and nothing is stored per lattice
    state: the workspace is two float32 ``[B, T]`` arrays.  No gradient, no host sync."""
    blank = int(blank)
    _certify_ctc_score_inputs(logits, act_lens, hyps, hyp_lens, n_hyp, blank)
    _lib.require_cuda(logits, act_lens, hyps, hyp_lens, n_hyp)
    B, T, V = logits.shape
    N, U = hyps.shape[1], hyps.shape[2]
    dev = logits.device
    scores = torch.empty(B, N, dtype=torch.float64, device=dev)
    ws = torch.empty(_lib.load().edgedict_ctc_score_workspace_bytes(B, T, N, U), dtype=torch.uint8, device=dev)
    _lib.call("ctc_score_nbest", logits.detach(), _lib.dtype_code(logits.dtype), act_lens, hyps if U else None,
              hyp_lens, n_hyp, B, T, N, U, V, blank, scores, ws)
    return scores


def ctc_loss_debug(logits, labels, act_lens, label_lens, blank=0):
    """Test hook: run the CTC forward and return (costs, log-sum-exps [B,T], alphas, betas [B,T,2U+1], loglikes [B,2]).
    beta(t,s) does not contain frame t's own log-probability (csrc/ctc_loss.hip); entries outside an utterance's
    ``[T_b, 2 U_b + 1]`` box are zeros."""
    _lib.require_cuda(logits)
    B, T, V = logits.shape
    U = labels.shape[1]
    lib = _lib.load()
    ws = torch.zeros(lib.edgedict_ctc_workspace_bytes(B, T, U), dtype=torch.uint8, device=logits.device)
    costs = torch.empty(B, dtype=torch.float32, device=logits.device)
    _lib.call("ctc_loss_forward", logits, _lib.dtype_code(logits.dtype), labels if U else None, act_lens, label_lens,
              B, T, U, V, int(blank), False, costs, None, 1.0, ws)
    base = ws.data_ptr()

    def view(which, shape, dtype):
        p = lib.edgedict_ctc_workspace_view(_lib.ptr(ws), B, T, U, which)
        esz = 8 if dtype == torch.float64 else 4
        off = (p - base) // esz
        n = 1
        for s in shape:
            n *= s
        return ws.view(dtype)[off:off + n].view(*shape).clone()

    S = 2 * U + 1
    return (costs, view(0, (B, T), torch.float32), view(1, (B, T, S), torch.float64),
            view(2, (B, T, S), torch.float64), view(3, (B, 2), torch.float64))


# ------------------------------------------------------------------------------------------------ softmax NLL
# The language model's loss (csrc/lm_loss.hip): log_softmax + NLLLoss(ignore_index) on raw logits [M, V] in two passes.


def _nll_ld(logits):
    M, V = logits.shape
    return ctypes.c_longlong(int(logits.stride(0)) if M > 1 else V)


def softmax_nll_rows(logits, targets, ignore_index=-100):
    """Forward-only scoring: ``nll[m] = logsumexp(logits[m]) - logits[m, targets[m]]`` (fp32 ``[M]``; exactly 0 where
    ``targets[m]`` equals ``ignore_index`` or lies outside ``[0, V)``).  ``logits`` float32 / bfloat16 ``[M, V]`` with
    unit column stride, ``targets`` int32 ``[M]``, both on the device.  One kernel, no reduction, nothing else written;
    not differentiable."""
    _lib.require_cuda(logits, targets)
    logits = logits.detach()
    M, V = logits.shape
    nll = torch.empty(M, dtype=torch.float32, device=logits.device)
    _lib.call("softmax_nll_forward", _lib.dtype_code(logits.dtype), logits, _nll_ld(logits), targets, M, V,
              int(ignore_index), None, nll, None, None, 0)
    return nll


class _SoftmaxNLLFn(torch.autograd.Function):
    """forward: lse / nll per row and the fixed-order fp64 reduction; backward: the gradient overwrites the logits."""

    @staticmethod
    def forward(ctx, logits, targets, ignore_index, reduction):
        _lib.require_cuda(logits, targets)
        M, V = logits.shape
        # one allocation: {sum, count} fp64 | reduced fp32 (+ pad) | lse [M] | nll [M]
        ws = torch.empty(6 + 2 * M, dtype=torch.float32, device=logits.device)
        stats, reduced, lse, nll = ws[:4].view(torch.float64), ws[4:5], ws[6:6 + M], ws[6 + M:]
        z = logits.detach()
        _lib.call("softmax_nll_forward", _lib.dtype_code(z.dtype), z, _nll_ld(z), targets, M, V, int(ignore_index),
                  lse, nll, stats, reduced, reduction == "mean")
        ctx.z = z                     # not save_for_backward: backward writes into it
        ctx.rest = (targets, lse, stats)
        ctx.cfg = (int(ignore_index), reduction)
        return nll if reduction == "none" else reduced.view(())

    @staticmethod
    def backward(ctx, grad_output):
        if ctx.z is None:
            raise RuntimeError("edgedict_amd: this loss's logits were consumed by a previous backward (the gradient "
                               "overwrote them; retain_graph is not supported)")
        z, ctx.z = ctx.z, None
        targets, lse, stats = ctx.rest
        ignore_index, reduction = ctx.cfg
        M, V = z.shape
        go = grad_output
        if go.dtype != torch.float32 or not go.is_contiguous():
            go = go.contiguous().float()
        _lib.call("softmax_nll_backward", _lib.dtype_code(z.dtype), z, _nll_ld(z), targets, M, V, ignore_index, lse, go,
                  1 if reduction == "none" else 0, stats, reduction == "mean")
        return z, None, None, None


class SoftmaxNLLLoss(torch.nn.Module):
    """``log_softmax`` + ``NLLLoss(ignore_index)`` on RAW logits, fused (csrc/lm_loss.hip): what
    ``torch.nn.functional.cross_entropy(logits, targets, ignore_index=..., reduction=...)`` computes.

    ``forward(logits, targets)``: ``logits`` float32 / bfloat16 ``[..., V]``, ``targets`` integer ``[...]`` (one per
    row).  Device tensors only: there is no CPU fallback.  A row is ignored when its target equals ``ignore_index`` OR
    lies outside ``[0, V)`` (torch raises for the latter; ``check_targets=True`` - one host read - raises ``ValueError``
    for it here too, before anything is launched).  ``reduction``: ``'mean'`` (over the valid rows) and ``'sum'`` return
    a 0-dim fp32 tensor, ``'none'`` fp32 of ``targets``' shape with exact zeros at ignored rows.

    ``'mean'`` over ZERO valid rows is 0 with a zero gradient (torch returns NaN): a batch that happens to be all padding
    must not poison the optimiser state, the reason ``CTCLoss`` departs from torch's reductions as well.

    The loss CONSUMES its logits: backward writes the gradient into the logits' own buffer, in their dtype (no
    ``[M, V]`` tensor is allocated in either pass), so the logits must not be read after ``backward`` and a second
    backward raises.  Forward and backward make no host synchronisation; sum and count are added in a fixed order in
    fp64, and loss and gradient are bit-identical from run to run."""

    def __init__(self, ignore_index=-100, reduction="mean", check_targets=False):
        super().__init__()
        if reduction not in ("mean", "sum", "none"):
            raise ValueError("reduction must be 'mean', 'sum' or 'none'")
        self.ignore_index = int(ignore_index)
        self.reduction = reduction
        self.check_targets = bool(check_targets)

    def forward(self, logits, targets):
        if logits.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError("logits must be float32 or bfloat16, got %s" % logits.dtype)
        if targets.dtype.is_floating_point or targets.dtype == torch.bool:
            raise TypeError("targets must be an integer tensor, got %s" % targets.dtype)
        if logits.dim() < 1 or tuple(targets.shape) != tuple(logits.shape[:-1]):
            raise ValueError("targets %s must have the shape of logits %s without its last dimension"
                             % (tuple(targets.shape), tuple(logits.shape)))
        V = logits.shape[-1]
        if V < 1:
            raise ValueError("logits need at least one class")
        if self.check_targets and targets.numel():     # one host read
            bad = (targets != self.ignore_index) & ((targets < 0) | (targets >= V))
            if bool(bad.any()):
                raise ValueError("a target lies outside [0, %d) and is not ignore_index = %d" % (V, self.ignore_index))
        _lib.require_cuda(logits, targets)
        z = logits.reshape(-1, V)
        if z.stride(1) != 1 or (z.shape[0] > 1 and z.stride(0) < V):
            z = z.contiguous()
        t = targets.reshape(-1)
        if t.dtype != torch.int32 or not t.is_contiguous():      # int32 targets spare this cast kernel
            t = t.to(torch.int32).contiguous()
        out = _SoftmaxNLLFn.apply(z, t, self.ignore_index, self.reduction)
        return out.view(targets.shape) if self.reduction == "none" else out


# ------------------------------------------------------------------------------------------------ MWER
# The risk layer of minimum word error rate training (csrc/mwer.hip): N-best costs and error counts in, the expected
# number of errors and its derivative with respect to the costs out.

MWER_MAX_N = 32


def _certify_mwer_inputs(costs, errs, n_hyp, ref_costs):
    # error classes / wording of _certify_ctc_score_inputs.  Returns the element stride of errs.
    named = (("costs", costs), ("errs", errs), ("n_hyp", n_hyp), ("ref_costs", ref_costs))
    for name, t in named:
        if t is not None and not torch.is_tensor(t):
            raise TypeError("%s must be a tensor, got %s" % (name, type(t).__name__))
    for name, t in (("costs", costs), ("ref_costs", ref_costs)):
        if t is not None and t.dtype != torch.float32:
            raise TypeError("%s must be float32, got %s" % (name, t.dtype))
    for name, t in (("errs", errs), ("n_hyp", n_hyp)):
        if t is not None and t.dtype != torch.int32:
            raise TypeError("%s must be int32, got %s" % (name, t.dtype))
    for name, t in named:
        if t is not None and not t.is_contiguous():
            raise ValueError("%s must be contiguous" % name)
    if costs.dim() != 2:
        raise ValueError("costs must have 2 dimensions [B,N], got %d" % costs.dim())
    if errs.dim() not in (2, 3):
        raise ValueError("errs must have 2 dimensions [B,N] or 3, [B,N,4] as metrics.edit_distance returns them, got %d"
                         % errs.dim())
    if (n_hyp is not None and n_hyp.dim() != 1) or (ref_costs is not None and ref_costs.dim() != 1):
        raise ValueError("n_hyp and ref_costs must have 1 dimension")
    B, N = costs.shape
    if tuple(errs.shape[:2]) != (B, N) or (errs.dim() == 3 and errs.shape[2] != 4):
        raise ValueError("must have an error count per slot (costs is %s, errs %s)"
                         % (tuple(costs.shape), tuple(errs.shape)))
    if n_hyp is not None and n_hyp.shape[0] != B:
        raise ValueError("must have a hypothesis count per example (n_hyp has %d, batch is %d)" % (n_hyp.shape[0], B))
    if ref_costs is not None and ref_costs.shape[0] != B:
        raise ValueError("must have a reference cost per example (ref_costs has %d, batch is %d)"
                         % (ref_costs.shape[0], B))
    if B < 1:
        raise ValueError("costs must hold at least one utterance (B = %d)" % B)
    if not 1 <= N <= MWER_MAX_N:
        raise ValueError("N = %d hypotheses per utterance outside [1, %d]" % (N, MWER_MAX_N))
    return 4 if errs.dim() == 3 else 1


def check_nll_weight(value):
    """``float(value)``; ValueError unless it is finite and >= 0."""
    w = float(value)
    if not (w >= 0.0 and math.isfinite(w)):
        raise ValueError("nll_weight must be finite and >= 0, got %r" % (value,))
    return w


class _MWERRiskFn(torch.autograd.Function):
    """forward: one ``edgedict_mwer_risk`` call that leaves the risk, the posterior, the coefficients ``d(scale risk_b) /
    d costs[b, n]`` and (unless ``reduction == 'none'``) the reduced value; backward: the coefficients times the incoming
    gradient.  Returns ``(risk [B], post)`` for ``reduction == 'none'``, else ``(reduced (1,), post, risk)``; only the first is
    differentiable."""

    @staticmethod
    def forward(ctx, costs, errs, n_hyp, ref_costs, nll_weight, reduction, stride):
        _lib.require_cuda(costs, errs, n_hyp, ref_costs)
        B, N = costs.shape
        dev = costs.device
        risk = torch.empty(B, dtype=torch.float32, device=dev)
        post = torch.empty(B, N, dtype=torch.float32, device=dev)
        coef = torch.empty(B, N, dtype=torch.float32, device=dev)
        reduced = None if reduction == "none" else torch.empty(1, dtype=torch.float32, device=dev)
        scale = 1.0 / B if reduction == "mean" else 1.0
        _lib.call("mwer_risk", costs.detach(), errs, stride, n_hyp, None if ref_costs is None else ref_costs.detach(), B,
                  N, ctypes.c_double(nll_weight), ctypes.c_double(scale), risk, post, coef, reduced)
        ctx.save_for_backward(coef)
        ctx.ref_grad = scale * nll_weight if ref_costs is not None else None
        ctx.per_row = reduced is None
        if reduced is None:
            ctx.mark_non_differentiable(post)
            return risk, post
        ctx.mark_non_differentiable(post, risk)              # (one call: a second one replaces the first)
        return reduced, post, risk

    @staticmethod
    def backward(ctx, grad_out, *_unused):
        coef, = ctx.saved_tensors
        go = grad_out.float()
        grad_costs = (go[:, None] if ctx.per_row else go) * coef
        grad_ref = None
        if ctx.ref_grad is not None and ctx.needs_input_grad[3]:
            grad_ref = (go * ctx.ref_grad).expand(coef.shape[0])
        return grad_costs, None, None, grad_ref, None, None, None


def mwer_risk(costs, errs, n_hyp=None):
    """The MWER risk of N-best lists (csrc/mwer.hip): ``costs`` float32 ``[B, N]``, the negative log-likelihood of every
    hypothesis (finite, or ``+inf`` for a slot to leave out; ``1 <= N <= 32``), ``errs`` int32 ``[B, N]`` or the
    ``[B, N, 4]`` of ``metrics.edit_distance`` (its ``dist`` is read in place), ``n_hyp`` int32 ``[B]`` (live slots; None:
    all ``N``).  Contiguous device tensors.  Returns ``(risk [B], post [B, N])`` float32: ``post`` is the softmax of
    ``-costs`` over the live slots (0 on the others), ``risk[b] = sum_n post[b, n] * errs[b, n]`` the expected number of
    errors (0 for an utterance without a live slot).  ``risk`` is differentiable in ``costs``: ``d risk[b] /
    d costs[b, n] = -post[b, n] (errs[b, n] - risk[b])``, formed in fp64 by the kernel with the errors taken relative to
    the list's minimum - exactly 0 where all live hypotheses have the same error count; ``post`` carries no gradient.
    One launch, no host sync, bit-identical from run to run."""
    stride = _certify_mwer_inputs(costs, errs, n_hyp, None)
    return _MWERRiskFn.apply(costs, errs, n_hyp, None, 0.0, "none", stride)


class MWERLoss(torch.nn.Module):
    """Minimum word error rate loss on N-best lists (Prabhavalkar et al. 2018): ``mean_b risk_b + nll_weight *
    mean_b ref_costs_b`` with ``risk`` as ``mwer_risk`` defines it.

    ``forward(costs, errs, n_hyp=None, ref_costs=None)``: ``costs`` / ``errs`` / ``n_hyp`` as ``mwer_risk`` takes them,
    ``ref_costs`` float32 ``[B]`` the negative log-likelihood of the reference transcripts - the interpolated
    cross-entropy term that keeps the posterior from drifting; it receives the gradient ``scale * nll_weight``.
    ``nll_weight > 0`` without ``ref_costs`` is a ``ValueError``.  ``reduction``: ``'mean'`` (default; ``sum / B`` with
    shape ``(1,)``, as ``RNNTLoss``), ``'sum'`` (shape ``(1,)``) or ``'none'`` (shape ``(B,)``).  Sums run in a fixed order
    in fp64 on the device; no host sync.  The per-utterance risk and the posterior of the last call stay in
    ``last_risk`` / ``last_posterior`` (detached device tensors)."""

    def __init__(self, nll_weight=0.0, reduction="mean"):
        super().__init__()
        if reduction not in ("mean", "sum", "none"):
            raise ValueError("reduction must be 'mean', 'sum' or 'none'")
        self.nll_weight = check_nll_weight(nll_weight)
        self.reduction = reduction
        self.last_risk = self.last_posterior = None

    def forward(self, costs, errs, n_hyp=None, ref_costs=None):
        if self.nll_weight > 0 and ref_costs is None:
            raise ValueError("nll_weight = %g needs ref_costs" % self.nll_weight)
        stride = _certify_mwer_inputs(costs, errs, n_hyp, ref_costs)
        if self.reduction == "none":
            risk, post = _MWERRiskFn.apply(costs, errs, n_hyp, None, 0.0, "none", stride)
            self.last_risk, self.last_posterior = risk.detach(), post
            return risk if ref_costs is None else risk + self.nll_weight * ref_costs
        out, post, risk = _MWERRiskFn.apply(costs, errs, n_hyp, ref_costs, self.nll_weight, self.reduction, stride)
        self.last_risk, self.last_posterior = risk, post
        return out


class MWERRows:
    """What ``mwer_rows`` packed: ONE host int32 buffer ``host`` holding, back to back, the arrays ``views()`` names.

    The lattice batch (a row per live hypothesis in ``(b, n)`` order - the first ``Rh`` rows - then, with references,
    a row per utterance; ``R`` rows in all):
      ``labels`` ``[R, Umax]`` (0 behind a row's length; ``Umax >= 1``), ``label_lens`` ``[R]``, ``row_utt`` ``[R]`` (the
      utterance of each row), ``row_slot`` ``[R]`` (its slot ``n`` in the dense layout, -1 for a reference row),
      ``row_dense`` ``[R]`` (``b * N + n``, -1 for a reference row);
    the layout of ``metrics.edit_distance``:
      ``hyps`` ``[B, N, Uh]``, ``hyp_lens`` ``[B, N]``, ``n_hyp`` ``[B]``, ``refs`` ``[B, Ur]``, ``ref_lens`` ``[B]``.
    ``lists[b]``: the distinct token sequences of utterance ``b`` (int64 arrays), slot by slot."""

    def __init__(self, host, R, Rh, Umax, B, N, Uh, Ur, lists):
        self.host, self.lists = host, lists
        self.R, self.Rh, self.Umax, self.B, self.N, self.Uh, self.Ur = R, Rh, Umax, B, N, Uh, Ur

    def _shapes(self):
        R, B, N = self.R, self.B, self.N
        return (("labels", (R, self.Umax)), ("label_lens", (R,)), ("row_utt", (R,)), ("row_slot", (R,)),
                ("row_dense", (R,)), ("hyps", (B, N, self.Uh)), ("hyp_lens", (B, N)), ("n_hyp", (B,)),
                ("refs", (B, self.Ur)), ("ref_lens", (B,)))

    def size(self):
        return sum(int(np.prod(shape)) for _, shape in self._shapes())

    def views(self, buf=None):
        """The named arrays as views of ``buf``: the host buffer (None), or its copy on a device (a 1-D tensor)."""
        buf = self.host if buf is None else buf
        out, o = {}, 0
        for name, shape in self._shapes():
            n = int(np.prod(shape))
            out[name] = buf[o:o + n].reshape(shape)
            o += n
        return out


def mwer_rows(lists, ys, ylen, with_reference):
    """The host-side packer of MWER training, one int32 upload like ``metrics.edit_distance_lists``'s: ``lists[b]`` the
    token sequences (ints, no blanks) hypothesised for utterance ``b``, ``ys`` ``[B, U]`` / ``ylen`` ``[B]`` the reference
    labels (host arrays or CPU tensors).  Sequences are de-duplicated (the first occurrence keeps its place); an empty
    list stands for the single empty hypothesis (as in ``metrics.oracle_error_rate``); more than 32 distinct sequences
    per utterance raise ``ValueError``.  Only live hypotheses become lattice rows; ``with_reference`` adds one row per
    utterance holding its reference.  Returns an ``MWERRows``."""
    from .metrics import EDIT_MAX_U, _seq
    ys = np.asarray(ys.detach().cpu() if torch.is_tensor(ys) else ys)
    ylen = np.asarray(ylen.detach().cpu() if torch.is_tensor(ylen) else ylen).reshape(-1)
    if ys.ndim != 2 or ys.shape[0] != ylen.shape[0]:
        raise ValueError("mwer_rows: ys must be [B, U] with one length per row (ys is %s, ylen has %d)"
                         % (tuple(ys.shape), ylen.shape[0]))
    B = ys.shape[0]
    if len(lists) != B:
        raise ValueError("mwer_rows: %d lists for %d references" % (len(lists), B))
    if B < 1:
        raise ValueError("mwer_rows: need at least one utterance")
    refs = [_seq(ys[b, :max(0, min(int(ylen[b]), ys.shape[1]))], "a reference") for b in range(B)]
    distinct = []
    for b, seqs in enumerate(lists):
        seen, own = set(), []
        for t in seqs:
            t = _seq(t, "a hypothesis")
            key = t.tobytes()
            if key not in seen:
                seen.add(key)
                own.append(t)
        if not own:
            own.append(np.zeros(0, dtype=np.int64))
        if len(own) > MWER_MAX_N:
            raise ValueError("mwer_rows: utterance %d has %d distinct hypotheses, more than the supported %d"
                             % (b, len(own), MWER_MAX_N))
        distinct.append(own)
    N = max(len(own) for own in distinct)
    Rh = sum(len(own) for own in distinct)
    R = Rh + (B if with_reference else 0)
    Uh = max(t.size for own in distinct for t in own)
    Ur = max(r.size for r in refs)
    Umax = max(1, Uh, Ur if with_reference else 0)
    assert Umax <= EDIT_MAX_U
    rows = MWERRows(None, R, Rh, Umax, B, N, Uh, Ur, distinct)
    rows.host = np.zeros(rows.size(), dtype=np.int32)
    v = rows.views()
    r = 0
    for b, own in enumerate(distinct):
        v["n_hyp"][b] = len(own)
        v["refs"][b, :refs[b].size] = refs[b]
        v["ref_lens"][b] = refs[b].size
        for n, t in enumerate(own):
            v["hyps"][b, n, :t.size] = t
            v["hyp_lens"][b, n] = t.size
            v["labels"][r, :t.size] = t
            v["label_lens"][r], v["row_utt"][r], v["row_slot"][r], v["row_dense"][r] = t.size, b, n, b * N + n
            r += 1
    if with_reference:
        for b in range(B):
            v["labels"][r, :refs[b].size] = refs[b]
            v["label_lens"][r], v["row_utt"][r], v["row_slot"][r], v["row_dense"][r] = refs[b].size, b, -1, -1
            r += 1
    return rows


CONF_COLUMNS = ("logp", "logp_max", "logp_blank", "entropy", "log_sum_p_alpha")


def row_confidence(logits, tokens, rows=None, alpha=1.0 / 3.0, ld=None, blank=0):
    """The five statistics of rows of logits that the confidence measures are built from (csrc/confidence.hip
    ``conf_row_stats``; ``decode.confidence_measure`` turns them into a number in ``[0, 1]``).  ``logits`` float32 /
    bfloat16 ``[N, V]`` raw, unit column stride, on the device; ``ld`` the distance between rows in elements (None:
    ``logits.stride(0)``, so a ``[:, :V]`` view of a wider buffer reads as it should; nothing behind column ``V`` is
    read).  ``tokens`` int32 ``[R]``; ``rows`` int32 ``[R]`` or None: output row ``r`` reads ``logits[rows[r]]``
    (repeats and any order allowed), None: row ``r`` with ``R <= N``.  ``0 < alpha < 1``.  Returns ``(stats, top)``
    on the device, no host sync: ``stats`` float32 ``[R, 5]`` in the order of ``CONF_COLUMNS`` -

        ``logp``       log-softmax at ``tokens[r]``, as ``(z[k] - max z) - log sum exp(z - max z)``: the searches' form
        ``logp_max``   the largest log-probability of the row
        ``logp_blank`` the blank's
        ``entropy``    the Shannon entropy of the row's softmax in nats, over all ``V`` symbols
        ``log_sum_p_alpha``   ``log sum_v p_v^alpha``, the sum inside the Tsallis and Renyi entropies of order ``alpha``

    - and ``top`` int32 ``[R]``, the arg max (lowest index on ties).  A ``-inf`` logit has probability 0 and adds nothing
    to any sum.  A token outside ``[0, V)`` gives NaN in ``logp`` only; a row holding a NaN or no logit above ``-inf``,
    and a ``rows[r]`` outside ``[0, N)`` (nothing is read for it), give five NaN and ``top = -1``.  One wave per row, no
    atomics: the same bits on every run.  Needs ``V >= 2``."""
    _lib.require_cuda(logits, tokens, rows)
    if logits.dim() != 2 or logits.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("row_confidence: logits must be float32 / bfloat16 [N, V]")
    N, V = logits.shape
    if V < 2 or (V > 1 and logits.stride(1) != 1):
        raise ValueError("row_confidence: logits need V >= 2 columns of unit stride")
    ld = int(logits.stride(0) if N > 1 else max(logits.stride(0), V)) if ld is None else int(ld)
    if ld < V:
        raise ValueError("row_confidence: ld = %d is below V = %d" % (ld, V))
    if tokens.dtype != torch.int32 or tokens.dim() != 1 or not tokens.is_contiguous():
        raise ValueError("row_confidence: tokens must be contiguous int32 [R]")
    R = tokens.shape[0]
    if rows is not None and (rows.dtype != torch.int32 or rows.shape != (R,) or not rows.is_contiguous()):
        raise ValueError("row_confidence: rows must be contiguous int32 [R]")
    if rows is None and R > N:
        raise ValueError("row_confidence: %d tokens for %d rows of logits" % (R, N))
    alpha, blank = float(alpha), int(blank)
    if not 0.0 < alpha < 1.0:
        raise ValueError("row_confidence: alpha must lie inside (0, 1), got %r" % (alpha,))
    if not 0 <= blank < V:
        raise ValueError("row_confidence: blank %d outside [0, %d)" % (blank, V))
    stats = torch.empty(R, 5, dtype=torch.float32, device=logits.device)
    top = torch.empty(R, dtype=torch.int32, device=logits.device)
    if R:
        _conf_row_stats(logits, ld, N, rows, tokens, R, V, blank, alpha, stats, top)
    return stats, top


def _conf_row_stats(logits, ld, N, rows, tokens, R, V, blank, alpha, stats, top):
    """The launch of ``row_confidence`` into given outputs (``decode.hypothesis_confidence`` fills slices of one)."""
    _lib.call("conf_row_stats", logits.detach(), _lib.dtype_code(logits.dtype), ctypes.c_longlong(ld), N, rows, tokens,
              R, V, blank, float(alpha), stats, top)
