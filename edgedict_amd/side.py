"""Off-critical-path work on the library's low-priority stream.

Weight gradients never feed the rest of the backward pass, so they do not have to run where
autograd runs: ``deferred(...)`` executes a block on the library's weight-gradient stream
(``edgedict_aux_stream(2)``, the same one the encoder stack uses — no additional HIP stream is
created, see include/edgedict_hip.h), after everything enqueued so far on the current stream, and
registers ONE autograd end-of-backward callback that makes the current stream wait for it.  The
block must ACCUMULATE into existing ``.grad`` buffers (the autograd node returns ``None`` for
those inputs); tensors it reads are ``record_stream``-ed so the caching allocator keeps them
alive until the side stream is done with them.  ``WeightGrads`` is the one place where an
autograd Function's backward decides between that and returning its weight gradients.
"""
import contextlib
import threading

import torch

from . import _lib, config, dp, ops

_streams = {}
_tls = threading.local()


def stream(device):
    dev = torch.device(device)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    s = _streams.get(idx)
    if s is None:
        with torch.cuda.device(idx):
            p = _lib.load().edgedict_aux_stream(2)
        if not p:
            raise RuntimeError("edgedict_amd: could not obtain the auxiliary stream")
        s = _streams[idx] = torch.cuda.ExternalStream(p, device=idx)
    return s


def peek(device):
    """The auxiliary stream of ``device`` if it has been created already, else None."""
    dev = torch.device(device)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    return _streams.get(idx)


def _join(idx):
    def cb():
        torch.cuda.current_stream(idx).wait_stream(_streams[idx])
        _tls.pending.discard(idx)
    return cb


@contextlib.contextmanager
def deferred(device, *reads):
    """Run the body on the auxiliary stream, ordered after the current stream's work so far.
    Only valid inside an autograd backward (the join is an end-of-backward callback)."""
    dev = torch.device(device)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    side = stream(idx)
    side.wait_stream(torch.cuda.current_stream(idx))
    for t in reads:
        if t is not None:
            t.record_stream(side)
    with torch.cuda.stream(side):
        yield side
    pending = getattr(_tls, "pending", None)
    if pending is None:
        pending = _tls.pending = set()
    if idx not in pending:
        pending.add(idx)
        torch.autograd.Variable._execution_engine.queue_callback(_join(idx))


def accumulates_in_place(p):
    """May the weight gradient of ``p`` be added straight into its existing .grad (flat-buffer training)?"""
    return p.grad is not None and p.grad.dtype == torch.float32 and p.grad.is_contiguous()


class WeightGrads:
    """The weight-gradient products of one autograd Function's backward, each written once for both destinations.

    ``params`` are the Function's weight parameters (``None`` for an absent bias), forward inputs ``first``,
    ``first + 1``, ...  A parameter autograd does not ask for (frozen after FlatParams gave it a .grad) gets nothing,
    as plain autograd would do.  When every live parameter accumulates in place and ``config.DEFER_WEIGHT_GRADS`` is
    set, the products issued inside ``with`` accumulate into the ``.grad`` buffers on the auxiliary stream
    (``deferred``; ``reads`` are the tensors they read) and, after the block, the live parameters are reported once to
    the data-parallel exchange (dp.BucketedAllReduce.ready): no autograd hook fires for them.  Otherwise each
    parameter's products write one fresh fp32 tensor on the current stream, and ``grads`` holds them (or ``None``)
    for the Function's return tuple."""

    def __init__(self, ctx, first, params, *reads):
        self.params = params
        self.need = [p is not None and n for p, n in zip(params, ctx.needs_input_grad[first:first + len(params)])]
        self.live = tuple(p for p, n in zip(params, self.need) if n)
        self.defer = bool(self.live) and config.DEFER_WEIGHT_GRADS and all(accumulates_in_place(p) for p in self.live)
        self.grads = [None] * len(params)
        self._reads = reads
        self._block = None

    def __enter__(self):
        if self.defer:
            self._block = deferred(self.live[0].device, *self._reads)
            self._block.__enter__()
        return self

    def __exit__(self, *exc):
        if self._block is not None:
            self._block.__exit__(*exc)
            if exc[0] is None and dp.READY_HOOK is not None:
                dp.READY_HOOK(self.live, stream(self.live[0].device))
        return False

    def _out(self, i, fresh):
        if self.defer:
            return self.params[i].grad
        g = self.grads[i]
        if g is None:
            p = self.params[i]
            g = self.grads[i] = fresh(p.shape, dtype=torch.float32, device=p.device)
        return g

    def gemm(self, i, a, b, cols=None, split_k=1, aux=None):
        """grad_i[:, cols] (+)= a @ b^T; ``aux``: the launch settings on the auxiliary stream where they differ."""
        if self.need[i]:
            out = self._out(i, torch.empty)
            kw = aux if self.defer and aux is not None else {"split_k": split_k}
            ops.gemm(a, b, out=out if cols is None else out[:, cols], accumulate=self.defer, **kw)

    def zero(self, i):
        """grad_i (+)= 0: a fresh zero tensor, or the .grad buffer as it is."""
        if self.need[i]:
            self._out(i, torch.zeros)

    def colsum(self, i, x):
        """grad_i (+)= the column sums of ``x``."""
        if self.need[i]:
            ops.colsum(x, out=self._out(i, torch.zeros))
