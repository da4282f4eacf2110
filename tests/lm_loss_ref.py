"""float64 numpy oracle of the softmax negative log-likelihood with ``ignore_index`` (edgedict_amd.loss.SoftmaxNLLLoss,
csrc/lm_loss.hip) and of the row log-softmax's backward.  Test infrastructure only; pinned against
torch.nn.functional.cross_entropy in float64 by tests/test_lm_loss_host.py.

A row is IGNORED when its target equals ``ignore_index`` or lies outside ``[0, V)``: its nll is 0 and its gradient row
is zero.  ``'mean'`` divides by the number of valid rows; with no valid row the loss is 0 and the gradient zero (torch
gives NaN there - the one deliberate difference)."""
import numpy as np


def valid_rows(targets, V, ignore_index):
    t = np.asarray(targets, dtype=np.int64)
    return (t != ignore_index) & (t >= 0) & (t < V)


def log_softmax(z):
    z = np.asarray(z, dtype=np.float64)
    m = z.max(axis=-1, keepdims=True)
    return (z - m) - np.log(np.exp(z - m).sum(axis=-1, keepdims=True))


def softmax_nll(z, targets, ignore_index=-100, reduction="mean", grad_out=None):
    """z [M, V], targets [M] -> (loss, nll [M], lse [M], dz [M, V]), all float64.

    ``loss`` is ``nll`` for ``'none'``, else a float.  ``grad_out``: the incoming gradient (``[M]`` for ``'none'``, a
    scalar otherwise; default ones / 1)."""
    z = np.asarray(z, dtype=np.float64)
    t = np.asarray(targets, dtype=np.int64)
    M, V = z.shape
    ok = valid_rows(t, V, ignore_index)
    logp = log_softmax(z)
    m = z.max(axis=1)
    lse = m + np.log(np.exp(z - m[:, None]).sum(axis=1))
    tc = np.where(ok, t, 0)
    nll = np.where(ok, -logp[np.arange(M), tc], 0.0)
    n = int(ok.sum())
    if reduction == "none":
        loss = nll
        g = np.ones(M) if grad_out is None else np.asarray(grad_out, dtype=np.float64).reshape(M)
    elif reduction == "sum":
        loss = float(nll.sum())
        g = np.full(M, 1.0 if grad_out is None else float(grad_out))
    elif reduction == "mean":
        loss = float(nll.sum() / n) if n else 0.0
        g = np.full(M, (1.0 if grad_out is None else float(grad_out)) / n) if n else np.zeros(M)
    else:
        raise ValueError(reduction)
    onehot = np.zeros((M, V))
    onehot[np.arange(M), tc] = 1.0
    dz = np.where(ok[:, None], g[:, None] * (np.exp(logp) - onehot), 0.0)
    return loss, nll, lse, dz


def log_softmax_bwd(y, dy):
    """dx = dy - exp(y) * rowsum(dy) for y = log_softmax(x)."""
    y = np.asarray(y, dtype=np.float64)
    dy = np.asarray(dy, dtype=np.float64)
    return dy - np.exp(y) * dy.sum(axis=-1, keepdims=True)
