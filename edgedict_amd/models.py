"""MI355X-native RNN-Transducer with the class surface of the reference's ``rnnt/models.py``.

Same constructor arguments, sub-module call signatures, state-dict keys/shapes and return types
as the reference, so ``cli/train.py`` / ``cli/baseline.py`` / ``rnnt/stream.py``
style callers run unchanged — but every piece of arithmetic on the path is a hand-written
gfx950 kernel reached through the C ABI in ``include/edgedict_hip.h``:

=====================  =====================================  ==============================
reference (file:line)  what                                   here
=====================  =====================================  ==============================
rnnt/models.py:131-136 Encoder.forward                        ``Encoder.forward``
rnnt/models.py:55-75   ResLayerNormLSTM.forward               ``_LSTMBlockFn`` per layer
rnnt/models.py:21-29   TimeReduction                          fused in ``layernorm_fwd``
rnnt/models.py:150-157 Decoder.forward                        ``Decoder.forward``
rnnt/models.py:169-179 Joint.forward                          ``_JointFn``
rnnt/models.py:223-241 Transducer.scale_length / forward      ``Transducer``
rnnt/models.py:243-269 Transducer.greedy_decode               ``Transducer.greedy_decode``
cli/train.py:294-319   Trainer.evaluate_step (behind the      ``Transducer.evaluate_step``
                       front-end)
=====================  =====================================  ==============================

PyTorch is the container/plumbing layer only: ``nn.Parameter`` holds the fp32 master weights,
``torch.autograd.Function`` routes gradients into ``.grad``, the caching allocator owns memory.
There is no CPU or eager-PyTorch fallback: tensors must live on an MI355X.
"""
import math
import weakref

import torch
from torch import nn

from . import config, encoder_stack, ops, side
from . import _lib
from ._lib import require_cuda
from .loss import _RNNTLossFn
from .tokenizer import BOS, NUL, PAD

F32 = torch.float32


# ----------------------------------------------------------------------------------------
# compute-dtype weight copies (fp32 master -> bf16 / transposed), refreshed when the
# parameter's version counter or the engine's parameter epoch changes
class _WeightCache:
    def __init__(self):
        self._store = {}

    def get(self, p, dtype, transposed=False):
        key = (id(p), dtype, transposed)
        ver = (p.data_ptr(), p._version, config.param_epoch())
        hit = self._store.get(key)
        # ids (and device addresses) are recycled once a tensor dies: the entry must belong to
        # THIS tensor object, not to a dead one that happened to share id, address and version
        # (the entry also holds the tensor it was built from, hit[3]: while it lives the allocator cannot hand that
        # address to another `.data` of the same parameter, so an equal address means the same storage)
        if hit is not None and hit[0] == ver and hit[2]() is p:
            return hit[1]
        # a miss: drop the copies of parameters that no longer exist (replicas of nn.DataParallel,
        # rebuilt models) - each holds a device tensor
        dead = [k for k, v in self._store.items() if v[2]() is None]
        for k in dead:
            del self._store[k]
        src = pinned = p.detach()
        if not src.is_contiguous():
            src = src.contiguous()
        if transposed == "lstm_fwd":
            t = ops.lstm_pack_weights(src, True, False)[0]
        elif transposed == "lstm_bwd":
            t = ops.lstm_pack_weights(src, False, True)[1]
        elif transposed:
            t = ops.transpose(src, dtype)
        elif dtype == src.dtype:
            t = src
        else:
            t = ops.cast(src, dtype)
        if t is not src and t.is_cuda:
            # the copy is made on whichever stream asked first and read from the other one too (caller's /
            # auxiliary): its block must not be recycled under a reader when the entry is replaced
            from . import side
            for s in (torch.cuda.current_stream(t.device), side.peek(t.device)):
                if s is not None:
                    t.record_stream(s)
        # `pinned` shares p's storage: `p.data = a; p.data = b` cannot put b where this image's source was (set_data keeps
        # the version counter, so an address match would return the old image)
        self._store[key] = (ver, t, weakref.ref(p), pinned)
        return t

    def clear(self):
        self._store.clear()


WEIGHTS = _WeightCache()


def _lstm_fast(cd, H):
    """bf16 fragment-order recurrence kernels (csrc/lstm_fast.hip) apply?"""
    return cd == torch.bfloat16 and H % 32 == 0 and not config.FORCE_GENERIC_LSTM


def _to_cd(x, cd):
    """Bring an activation into the compute dtype (device cast kernel, no-op if already there)."""
    if x.dtype == cd:
        return x.contiguous()
    if x.dtype not in (torch.float32, torch.bfloat16):
        x = x.float()
    return ops.cast(x.contiguous(), cd)


def _state(t):
    """Recurrent state slice -> contiguous fp32 [B,H] (or None)."""
    if t is None:
        return None
    t = t.detach()
    if t.dtype != F32:
        t = ops.cast(t.contiguous(), F32)
    return t.contiguous()


# ----------------------------------------------------------------------------------------
# autograd plumbing around the kernels
class _InputNormFn(torch.autograd.Function):
    """LayerNorm(input_size) on the stacked log-mel input (rnnt/models.py:124,132)."""

    @staticmethod
    def forward(ctx, xs, gamma, beta, cd):
        x = _to_cd(xs, cd)
        y, mean, rstd = ops.layernorm_fwd(x, None, gamma.detach(), beta.detach(), 1)
        ctx.save_for_backward(x, gamma, mean, rstd)
        ctx.in_dtype = xs.dtype
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, mean, rstd = ctx.saved_tensors
        ds, dgamma, dbeta = ops.layernorm_bwd(dy, x, None, gamma.detach(), mean, rstd, 1)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = ds if ds.dtype == ctx.in_dtype else ops.cast(ds, ctx.in_dtype)
        return dx, dgamma, dbeta, None


class _LSTMBlockFn(torch.autograd.Function):
    """One 1-layer LSTM over the whole sequence, optionally followed by the encoder's
    residual add + LayerNorm (+ TimeReduction).

    forward : G = x W_ih^T + b_ih + b_hh (one MFMA GEMM) -> T step kernels -> fused LN epilogue
    backward: LN backward -> T BPTT step kernels (G becomes dG in place) -> dX, dW_ih, dW_hh as
              GEMMs reading dG / x / h_{t-1} transposed in place, db as a column sum.
    """

    @staticmethod
    def forward(ctx, x, w_ih, w_hh, b_ih, b_hh, ln_w, ln_b, h0, c0, residual, reduce, cd):
        B, T, I = x.shape
        H = w_hh.shape[1]
        wih = WEIGHTS.get(w_ih, cd)
        fast = _lstm_fast(cd, H)
        whh = None if fast else WEIGHTS.get(w_hh, cd)
        whh_p = WEIGHTS.get(w_hh, cd, "lstm_fwd") if fast else None
        G = ops.gemm(x.view(B * T, I), wih, bias=b_ih.detach(), bias2=b_hh.detach())
        G = G.view(B, T, 4 * H)
        with ops.timed("lstm_fwd_T%d_H%d" % (T, H)):
            Y, Hprev, Cst, hN, cN = ops.lstm_forward(G, whh, h0, c0, whh_p)
        if ln_w is not None:
            out, mean, rstd = ops.layernorm_fwd(Y, x if residual else None, ln_w.detach(),
                                                ln_b.detach(), reduce)
        else:
            out, mean, rstd = Y, None, None
        ctx.save_for_backward(x, w_ih, w_hh, ln_w, c0)
        ctx.biases = (b_ih, b_hh)
        ctx.inter = (G, Y, Hprev, Cst, mean, rstd)
        ctx.cfg = (residual, reduce, cd, ln_w is not None)
        ctx.mark_non_differentiable(hN, cN)
        return out, hN, cN

    @staticmethod
    def backward(ctx, dout, _dh, _dc):
        if ctx.inter is None:
            raise RuntimeError("edgedict_amd: this LSTM block's saved gates were consumed by a "
                               "previous backward (retain_graph is not supported)")
        x, w_ih, w_hh, ln_w, c0 = ctx.saved_tensors
        G, Y, Hprev, Cst, mean, rstd = ctx.inter
        ctx.inter = None
        residual, reduce, cd, has_ln = ctx.cfg
        B, T, I = x.shape
        H = w_hh.shape[1]
        dgamma = dbeta = None
        if has_ln:
            ds, dgamma, dbeta = ops.layernorm_bwd(dout, Y, x if residual else None,
                                                  ln_w.detach(), mean, rstd, reduce)
        else:
            ds = dout.contiguous()
        with ops.timed("lstm_bwd_T%d_H%d" % (T, H)):
            if _lstm_fast(cd, H):
                ops.lstm_backward(G, ds, Cst, c0, None, WEIGHTS.get(w_hh, cd, "lstm_bwd"))
            else:
                ops.lstm_backward(G, ds, Cst, c0, WEIGHTS.get(w_hh, cd, transposed=True))
        dG = G.view(B * T, 4 * H)
        x2 = x.view(B * T, I)
        M = B * T
        # the layer below waits for dx only: it goes first; the weight gradients feed nothing downstream
        dx = None
        if ctx.needs_input_grad[0]:
            wih = WEIGHTS.get(w_ih, cd)
            if residual and has_ln:
                dx = ds  # d(residual) + dG W_ih, accumulated in place by the GEMM epilogue
                ops.gemm(dG, wih.t(), out=ds.view(M, I), accumulate=True)
            else:
                dx = ops.gemm(dG, wih.t()).view(B, T, I)
        # ... so they may accumulate into the .grad buffers on the auxiliary stream, under the next layer's BPTT (side.py)
        with side.WeightGrads(ctx, 1, (w_ih, w_hh) + ctx.biases, G, x, Hprev) as wg:
            wg.gemm(0, dG.t(), x2.t(), split_k=ops.pick_split_k(4 * H, I, M))
            wg.gemm(1, dG.t(), Hprev.view(M, H).t(), split_k=ops.pick_split_k(4 * H, H, M))
            wg.colsum(2, dG)
            wg.colsum(3, dG)
        return (dx, *wg.grads, dgamma, dbeta, None, None, None, None, None)


class _GRUBlockFn(torch.autograd.Function):
    """One 1-layer GRU over the whole sequence + the encoder's residual add / LayerNorm /
    TimeReduction, as ``_LSTMBlockFn`` (ResLayerNormGRU.forward, rnnt/models.py:99-116).

    forward : G = x W_ih^T + b_ih (one MFMA GEMM) -> T step kernels (csrc/gru.hip) -> fused LN epilogue
    backward: LN backward -> T BPTT step kernels (G -> input-side, DH -> hidden-side pre-activation
              gradients) -> dX, dW_ih, dW_hh as GEMMs, both biases as column sums."""

    @staticmethod
    def forward(ctx, x, w_ih, w_hh, b_ih, b_hh, ln_w, ln_b, h0, residual, reduce, cd):
        B, T, I = x.shape
        H = w_hh.shape[1]
        G = ops.gemm(x.view(B * T, I), WEIGHTS.get(w_ih, cd), bias=b_ih.detach()).view(B, T, 3 * H)
        with ops.timed("gru_fwd_T%d_H%d" % (T, H)):
            Y, Hprev, HN, hN = ops.gru_forward(G, WEIGHTS.get(w_hh, cd), b_hh.detach(), h0)
        if ln_w is not None:
            out, mean, rstd = ops.layernorm_fwd(Y, x if residual else None, ln_w.detach(),
                                                ln_b.detach(), reduce)
        else:
            out, mean, rstd = Y, None, None
        ctx.save_for_backward(x, w_ih, w_hh, ln_w)
        ctx.inter = (G, Y, Hprev, HN, mean, rstd)
        ctx.cfg = (residual, reduce, cd, ln_w is not None)
        ctx.mark_non_differentiable(hN)
        return out, hN

    @staticmethod
    def backward(ctx, dout, _dh):
        if ctx.inter is None:
            raise RuntimeError("edgedict_amd: this GRU block's saved gates were consumed by a "
                               "previous backward (retain_graph is not supported)")
        x, w_ih, w_hh, ln_w = ctx.saved_tensors
        G, Y, Hprev, HN, mean, rstd = ctx.inter
        ctx.inter = None
        residual, reduce, cd, has_ln = ctx.cfg
        B, T, I = x.shape
        H = w_hh.shape[1]
        dgamma = dbeta = None
        if has_ln:
            ds, dgamma, dbeta = ops.layernorm_bwd(dout, Y, x if residual else None,
                                                  ln_w.detach(), mean, rstd, reduce)
        else:
            ds = dout.contiguous()
        with ops.timed("gru_bwd_T%d_H%d" % (T, H)):
            DH = ops.gru_backward(G, ds, Hprev, HN, WEIGHTS.get(w_hh, cd, transposed=True))
        M = B * T
        dG, dH2, x2 = G.view(M, 3 * H), DH.view(M, 3 * H), x.view(M, I)
        dw_ih = ops.gemm(dG.t(), x2.t(), out_dtype=F32, split_k=ops.pick_split_k(3 * H, I, M))
        dw_hh = ops.gemm(dH2.t(), Hprev.view(M, H).t(), out_dtype=F32,
                         split_k=ops.pick_split_k(3 * H, H, M))
        db_ih, db_hh = ops.colsum(dG), ops.colsum(dH2)
        dx = None
        if ctx.needs_input_grad[0]:
            wih = WEIGHTS.get(w_ih, cd)
            if residual and has_ln:
                dx = ds  # d(residual) + dG W_ih, accumulated in place by the GEMM epilogue
                ops.gemm(dG, wih.t(), out=ds.view(M, I), accumulate=True)
            else:
                dx = ops.gemm(dG, wih.t()).view(B, T, I)
        return (dx, dw_ih, dw_hh, db_ih, db_hh, dgamma, dbeta, None, None, None, None)


class _DropoutFn(torch.autograd.Function):
    """Training-mode dropout with a counter-based mask (csrc/elementwise.hip): the backward pass
    re-applies the same (p, seed) to the gradient, no mask tensor is kept."""

    @staticmethod
    def forward(ctx, x, p, seed):
        ctx.cfg = (float(p), int(seed))
        return ops.dropout(x, p, seed)

    @staticmethod
    def backward(ctx, dy):
        p, seed = ctx.cfg
        return ops.dropout(dy.contiguous(), p, seed), None, None


_dropout_calls = [0]


def _next_dropout_seed():
    """A fresh mask per call: seed = torch's RNG stream (so torch.manual_seed governs it) mixed with
    a call counter."""
    _dropout_calls[0] += 1
    return (torch.initial_seed() * 0x9E3779B1 + _dropout_calls[0] * 0x85EBCA6B) & 0xFFFFFFFF


def _dropout(x, p):
    return _DropoutFn.apply(x, p, _next_dropout_seed())


class _LinearFn(torch.autograd.Function):
    """y = x W^T + b on the last dimension (nn.Linear: rnnt/models.py:129,135,148,156)."""

    @staticmethod
    def forward(ctx, x, w, b, cd):
        shp = x.shape
        x2 = x.reshape(-1, shp[-1])
        wc = WEIGHTS.get(w, cd)
        y = ops.gemm(x2, wc, bias=b.detach() if b is not None else None)
        ctx.save_for_backward(x2, w)
        ctx.bias = b
        ctx.cfg = (cd, shp)
        return y.view(*shp[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2, w = ctx.saved_tensors
        cd, shp = ctx.cfg
        dy2 = dy.reshape(-1, w.shape[0])
        if not dy2.is_contiguous():
            dy2 = dy2.contiguous()
        M = x2.shape[0]
        # dx first: it is what the rest of the backward pass waits for (the encoder's projection sits between the joint
        # and the stack's BPTT); dW / db go to the auxiliary stream when they can accumulate in place (side.py)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = ops.gemm(dy2, WEIGHTS.get(w, cd).t()).view(*shp)
        with side.WeightGrads(ctx, 1, (w, ctx.bias), dy2, x2) as wg:
            wg.gemm(0, dy2.t(), x2.t(), split_k=ops.pick_split_k(w.shape[0], w.shape[1], M))
            wg.colsum(1, dy2)
        return (dx, *wg.grads, None)


class _EmbeddingFn(torch.autograd.Function):
    """BOS left-pad + nn.Embedding(padding_idx=PAD) (rnnt/models.py:150-153)."""

    @staticmethod
    def forward(ctx, tokens, weight, prepend_bos, cd):
        out = ops.embedding_fwd(tokens, weight.detach(), cd, prepend_bos, BOS)
        ctx.save_for_backward(tokens)
        ctx.cfg = (weight.shape[0], prepend_bos)
        return out

    @staticmethod
    def backward(ctx, dout):
        (tokens,) = ctx.saved_tensors
        V, prepend_bos = ctx.cfg
        return None, ops.embedding_bwd(tokens, dout, V, prepend_bos, BOS, PAD), None, None


class _JointFn(torch.autograd.Function):
    """logits[b,t,u,:] = W2 tanh(W1 [enc[b,t]; dec[b,u]] + b1) + b2 (rnnt/models.py:169-179).

    W1 is applied as two small GEMMs (W1[:, :P_enc] on enc, W1[:, P_enc:] on dec) followed by a
    broadcast-add+tanh kernel, so the reference's [B,T,U+1,P_enc+P_dec] concat is never built.
    """

    @staticmethod
    def forward(ctx, enc, dec, w1, b1, w2, b2, cd):
        B, T, P = enc.shape
        U1, P2 = dec.shape[1], dec.shape[2]
        J, V = w1.shape[0], w2.shape[0]
        w1c = WEIGHTS.get(w1, cd)
        w2c = WEIGHTS.get(w2, cd)
        enc2 = enc.reshape(B * T, P)
        dec2 = dec.reshape(B * U1, P2)
        E1 = ops.gemm(enc2, w1c[:, :P])
        D1 = ops.gemm(dec2, w1c[:, P:], bias=b1.detach())
        hid = ops.joint_hidden_fwd(E1.view(B, T, J), D1.view(B, U1, J))
        with ops.timed("joint_logits_gemm"):
            logits = ops.gemm(hid.view(B * T * U1, J), w2c, bias=b2.detach())
        ctx.save_for_backward(enc2, dec2, w1, w2, hid)
        ctx.b1, ctx.b2 = b1, b2
        ctx.cfg = (cd, B, T, U1, P, P2, J, V)
        return logits.view(B, T, U1, V)

    @staticmethod
    def backward(ctx, dlogits):
        ops.mark("joint_bwd:enter")
        enc2, dec2, w1, w2, hid = ctx.saved_tensors
        cd, B, T, U1, P, P2, J, V = ctx.cfg
        M = B * T * U1
        dl = dlogits.reshape(M, V)
        if not dl.is_contiguous():
            dl = dl.contiguous()
        hid2 = hid.view(M, J)
        w1c = WEIGHTS.get(w1, cd)
        w2c = WEIGHTS.get(w2, cd)
        with ops.timed("joint_dhid_gemm"):
            # dl x W2 with W2^T materialised once per optimiser step (1.3 M elements): both
            # operands K-contiguous -> the direct-to-LDS kernel (gemm_nt.hip)
            dhid = ops.gemm(dl, WEIGHTS.get(w2, cd, transposed=True))
        dE1, dD1 = ops.joint_hidden_bwd(dhid.view(B, T, U1, J), hid)
        del dhid
        dE1c = ops.cast(dE1, cd).view(B * T, J)
        dD1c = ops.cast(dD1, cd).view(B * U1, J)
        denc = ops.gemm(dE1c, w1c[:, :P].t()).view(B, T, P)
        ddec = ops.gemm(dD1c, w1c[:, P:].t()).view(B, U1, P2)
        # the weight gradients feed nothing downstream: enqueued AFTER the critical-path products above, so that on the
        # auxiliary stream (side.py) they start when those are done and their MFMA work runs under the latency-bound
        # recurrences that follow
        with side.WeightGrads(ctx, 2, (w1, ctx.b1, w2, ctx.b2), dl, hid, dE1c, dD1c, dD1, enc2, dec2) as wg:
            wg.gemm(2, dl.t(), hid2.t(), split_k=ops.pick_split_k(V, J, M), aux=dict(split_k=8, max_wg_per_cu=2))
            wg.colsum(3, dl)
            wg.gemm(0, dE1c.t(), enc2.t(), cols=slice(None, P), split_k=ops.pick_split_k(J, P, B * T))
            wg.gemm(0, dD1c.t(), dec2.t(), cols=slice(P, None), split_k=ops.pick_split_k(J, P2, B * U1))
            wg.colsum(1, dD1.view(B * U1, J))
        ops.mark("joint_bwd:exit")
        return (denc, ddec, *wg.grads, None)


class _JointLossFn(torch.autograd.Function):
    """Joint network + RNN-T loss on the PACKED lattice (training path of Transducer.forward).

    Same arithmetic as ``_JointFn`` followed by ``_RNNTLossFn`` (rnnt/models.py:169-179,
    221,238), but only the cells inside each utterance's (T_b, U_b+1) box exist: hid, logits and
    their gradients are [M_valid, .] matrices (row of (b,t,u) = off[b] + t (U_b+1) + u).  Cells
    outside the box have zero gradient and no influence on the loss, so nothing changes
    numerically; the two big products and the loss kernels just do not touch padding
    (35 % of the rows on the bench batch).  Needs the lengths on the HOST (they size M_valid).
    ``fastemit_lambda`` > 0 scales the gradient through the label emissions by 1 + lambda (loss.py);
    the returned loss stays the plain negative log-likelihood.
    ``win_lo`` / ``win_hi`` (int32 [B, U] on the device, or None): the alignment-restricted loss (loss.py).  The joint
    still runs on every cell of the boxes; only the loss gradient skips the cells the windows kill, and
    ``ops.LAST["joint_band_rows"]`` holds how many of the ``joint_rows`` stay alive (device tensor, no sync).
    ``plan`` (a finished ``loss.BandPlan`` of the same windows and lengths, or None): joint and loss on the BAND rows -
    hid, logits and their gradients are [M_band, .] matrices of the live cells only, the same products with a smaller
    M; the dense workspace planes of the loss get -inf log-probabilities on the dead cells of the boxes, which is what
    the lattice walks saw of them before (an alpha or a beta of -inf), so the loss is the box path's.  With
    ``plan.rows == 0`` (no utterance has an alignment) nothing is launched: the loss is +inf, every gradient zero.
    ``ops.LAST["joint_packed_rows"]`` is the number of rows materialised (``joint_rows`` without a plan).
    ``row_costs=True`` (MWER training, ``Transducer.mwer_loss``): the same forward, but the per-row costs ``[B]`` are
    returned instead of their mean, differentiable - backward hands the incoming ``[B]`` gradient to the packed gradient
    kernels as their per-utterance scale (stride 1, host scale 1).  The batch's rows need not reach ``T`` and ``U``
    (they are an N-best list's hypotheses).  Not with windows, a band plan or FastEmit: ``ValueError``."""

    @staticmethod
    def forward(ctx, enc, dec, w1, b1, w2, b2, labels, act_lens, label_lens, blank, cd, fastemit_lambda=0.0,
                win_lo=None, win_hi=None, plan=None, row_costs=False):
        from ._staging import to_device
        B, T, P = enc.shape
        U1, P2 = dec.shape[1], dec.shape[2]
        J, V = w1.shape[0], w2.shape[0]
        dev = enc.device
        al = act_lens.to(torch.int64).cpu()
        ll = label_lens.to(torch.int64).cpu()
        ctx.row_costs = bool(row_costs)
        if row_costs:
            if win_lo is not None or win_hi is not None or plan is not None or float(fastemit_lambda) != 0.0:
                raise ValueError("per-row costs of the packed joint take no windows, no band plan and no FastEmit")
            if int(al.max()) > T or int(ll.max()) > U1 - 1 or int(al.min()) < 1 or int(ll.min()) < 0:
                raise ValueError("Input length mismatch")
        elif int(al.max()) != T or int(ll.max()) != U1 - 1 or int(al.min()) < 1 or int(ll.min()) < 0:
            raise ValueError("Input length mismatch")     # wording of warprnnt_pytorch's checks
        rows = al * (ll + 1)
        off = torch.zeros(B, dtype=torch.int64)
        off[1:] = torch.cumsum(rows, 0)[:-1]
        M = int(rows.sum())
        off_d = to_device(off, dev)
        al_d = to_device(al.to(torch.int32), dev)
        ll_d = to_device(ll.to(torch.int32), dev)
        ops.LAST["joint_rows"] = M
        if plan is not None:
            if win_lo is None or plan.rows is None or tuple(plan.band.shape) != (B, T, 2) or plan.U1 != U1:
                raise ValueError("the band plan needs windows, finish() and the lattice's shape [%d, %d, %d]" % (B, T, U1))
            return _JointLossFn._forward_band(ctx, enc, dec, w1, b1, w2, b2, labels, al_d, ll_d, blank, cd,
                                              fastemit_lambda, win_lo, win_hi, plan, M)
        ops.LAST["joint_packed_rows"] = M
        ctx.plan = None
        w1c = WEIGHTS.get(w1, cd)
        w2c = WEIGHTS.get(w2, cd)
        enc2 = enc.reshape(B * T, P)
        dec2 = dec.reshape(B * U1, P2)
        E1 = ops.gemm(enc2, w1c[:, :P])
        D1 = ops.gemm(dec2, w1c[:, P:], bias=b1.detach())
        hid = torch.empty(M, J, dtype=cd, device=dev)
        with ops.timed("joint_hidden_fwd"):
            _lib.call("joint_hidden_fwd_packed", _lib.dtype_code(cd), E1, D1, hid, al_d, ll_d, off_d,
                      B, T, U1, J)
        restricted = win_lo is not None
        if restricted:
            band = torch.empty(B, T, 2, dtype=torch.int32, device=dev)
            cells = torch.empty(B, dtype=torch.int64, device=dev)
            _lib.call("rnnt_band", win_lo, win_hi, al_d, ll_d, B, T, U1, band, cells)
            ops.LAST["joint_band_rows"] = cells.sum()
        else:
            ops.LAST.pop("joint_band_rows", None)
        lib = _lib.load()
        ws = torch.empty(lib.edgedict_rnnt_workspace_bytes(B, T, U1), dtype=torch.uint8, device=dev)
        costs = torch.empty(B, dtype=F32, device=dev)
        reduced = torch.empty(1, dtype=F32, device=dev)
        if config.FUSED_LSE and cd == torch.bfloat16 and J >= 128 and J % 64 == 0 and V % 8 == 0 and M >= 256:
            # logits product with the log-softmax partials in its epilogue (gemm_nt256.hip): the loss
            # finishes the denominators from M x V/64 pairs instead of re-reading the logits
            slots = (V + 63) // 64
            parts = torch.empty(M, slots, 2, dtype=F32, device=dev)
            logits = torch.empty(M, V, dtype=cd, device=dev)
            # (TrainEngine hangs the next batch's front-end here: beside this matrix-bound product it is nearly free;
            # beside the encoder's recurrence, or beside the bandwidth-bound tanh kernel above, it cost what it saved)
            ops.fire("before_logits_gemm")
            with ops.timed("joint_logits_gemm"):
                _lib.call("gemm_nt_lse", hid, ops._ll(J), w2c, ops._ll(J), logits, ops._ll(V), M, V, J,
                          b2.detach(), parts)
            with ops.timed("rnnt_loss_fwd"):
                if restricted:
                    _lib.call("rnnt_loss_forward_packed_parts_ar", logits, labels, al_d, ll_d, win_lo, win_hi, off_d,
                              B, T, U1, V, int(blank), costs, reduced, 1.0 / B, ws, parts, slots)
                else:
                    _lib.call("rnnt_loss_forward_packed_parts", logits, labels, al_d, ll_d, off_d, B, T, U1, V,
                              int(blank), costs, reduced, 1.0 / B, ws, parts, slots)
        else:
            with ops.timed("joint_logits_gemm"):
                logits = ops.gemm(hid, w2c, bias=b2.detach())
            if restricted:
                _lib.call("rnnt_loss_forward_packed_ar", logits, _lib.dtype_code(cd), labels, al_d, ll_d, win_lo,
                          win_hi, off_d, B, T, U1, V, int(blank), costs, reduced, 1.0 / B, ws)
            else:
                _lib.call("rnnt_loss_forward_packed", logits, _lib.dtype_code(cd), labels, al_d, ll_d, off_d,
                          B, T, U1, V, int(blank), costs, reduced, 1.0 / B, ws)
        # per-utterance costs of the last packed joint + loss ([B], device; detached: the returned tensor of the
        # row_costs form carries this node, and a reference to it would keep the lattice alive)
        ops.LAST["joint_costs"] = costs.detach()
        ctx.save_for_backward(enc2, dec2, w1, w2, hid, logits, labels, al_d, ll_d, off_d, ws)
        ctx.b1, ctx.b2 = b1, b2
        ctx.cfg = (cd, B, T, U1, P, P2, J, V, M, int(blank))
        ctx.fastemit_lambda = float(fastemit_lambda)
        ctx.restricted = restricted
        return costs if row_costs else reduced

    @staticmethod
    def _forward_band(ctx, enc, dec, w1, b1, w2, b2, labels, al_d, ll_d, blank, cd, fastemit_lambda, win_lo, win_hi,
                      plan, M_box):
        """forward() on the band rows of ``plan``: the same chain with M = plan.rows and the *_band entry points."""
        B, T, P = enc.shape
        U1, P2 = dec.shape[1], dec.shape[2]
        J, V = w1.shape[0], w2.shape[0]
        dev = enc.device
        M = plan.rows
        ops.LAST["joint_packed_rows"] = M
        ops.LAST["joint_band_rows"] = plan.cells.sum()
        ctx.plan = plan
        ctx.b1, ctx.b2 = b1, b2
        ctx.cfg = (cd, B, T, U1, P, P2, J, V, M, int(blank))
        ctx.fastemit_lambda = float(fastemit_lambda)
        ctx.restricted = True
        enc2 = enc.reshape(B * T, P)
        dec2 = dec.reshape(B * U1, P2)
        if M == 0:
            # no utterance has a window-respecting alignment: no product, no band kernel; +inf and zero gradients
            ops.LAST["joint_costs"] = torch.full((B,), float("inf"), dtype=F32, device=dev)
            ctx.save_for_backward(enc2, dec2, w1, w2)
            return torch.full((1,), float("inf"), dtype=F32, device=dev)
        w1c = WEIGHTS.get(w1, cd)
        w2c = WEIGHTS.get(w2, cd)
        E1 = ops.gemm(enc2, w1c[:, :P])
        D1 = ops.gemm(dec2, w1c[:, P:], bias=b1.detach())
        hid = torch.empty(M, J, dtype=cd, device=dev)
        with ops.timed("joint_hidden_fwd"):
            _lib.call("joint_hidden_fwd_band", _lib.dtype_code(cd), E1, D1, hid, plan.band, plan.row_off, ops._ll(M),
                      B, T, U1, J)
        lib = _lib.load()
        ws = torch.empty(lib.edgedict_rnnt_workspace_bytes(B, T, U1), dtype=torch.uint8, device=dev)
        costs = torch.empty(B, dtype=F32, device=dev)
        reduced = torch.empty(1, dtype=F32, device=dev)
        tables = (plan.band, plan.row_off, plan.row_tu, plan.cells)
        if config.FUSED_LSE and cd == torch.bfloat16 and J >= 128 and J % 64 == 0 and V % 8 == 0 and M >= 256:
            slots = (V + 63) // 64
            parts = torch.empty(M, slots, 2, dtype=F32, device=dev)
            logits = torch.empty(M, V, dtype=cd, device=dev)
            ops.fire("before_logits_gemm")
            with ops.timed("joint_logits_gemm"):
                _lib.call("gemm_nt_lse", hid, ops._ll(J), w2c, ops._ll(J), logits, ops._ll(V), M, V, J,
                          b2.detach(), parts)
            with ops.timed("rnnt_loss_fwd"):
                _lib.call("rnnt_loss_forward_band_parts", logits, labels, al_d, ll_d, win_lo, win_hi, *tables,
                          B, T, U1, V, int(blank), costs, reduced, 1.0 / B, ws, parts, slots)
        else:
            with ops.timed("joint_logits_gemm"):
                logits = ops.gemm(hid, w2c, bias=b2.detach())
            _lib.call("rnnt_loss_forward_band", logits, _lib.dtype_code(cd), labels, al_d, ll_d, win_lo, win_hi, *tables,
                      B, T, U1, V, int(blank), costs, reduced, 1.0 / B, ws)
        ops.LAST["joint_costs"] = costs
        ctx.save_for_backward(enc2, dec2, w1, w2, hid, logits, labels, al_d, ll_d, ws)
        return reduced

    @staticmethod
    def _backward_band(ctx, gout):
        plan = ctx.plan
        cd, B, T, U1, P, P2, J, V, M, blank = ctx.cfg
        tail = (None,) * 10
        if M == 0:
            enc2, dec2, w1, w2 = ctx.saved_tensors
            with side.WeightGrads(ctx, 2, (w1, ctx.b1, w2, ctx.b2)) as wg:
                for i in range(4):
                    wg.zero(i)
            ops.mark("joint_bwd:exit")
            return (torch.zeros(B, T, P, dtype=enc2.dtype, device=enc2.device),
                    torch.zeros(B, U1, P2, dtype=dec2.dtype, device=dec2.device), *wg.grads, *tail)
        enc2, dec2, w1, w2, hid, logits, labels, al_d, ll_d, ws = ctx.saved_tensors
        dl = torch.empty_like(logits)
        gscale = gout.contiguous().float()
        w1c = WEIGHTS.get(w1, cd)
        w2t = WEIGHTS.get(w2, cd, transposed=True)
        dE1 = torch.empty(B, T, J, dtype=F32, device=dl.device)
        dD1 = torch.empty(B, U1, J, dtype=F32, device=dl.device)
        cs_rows = _lib.load().edgedict_rnnt_grad_colsum_rows(_lib.dtype_code(cd), B, T, U1, V) if config.FUSED_DB2 else 0
        db2_parts = torch.empty(cs_rows, V, dtype=F32, device=dl.device) if cs_rows > 0 else None
        rows = (plan.row_off, plan.row_tu, plan.cells)
        with ops.timed("rnnt_grad"):
            if db2_parts is not None:
                _lib.call("rnnt_loss_backward_band_colsum", logits, _lib.dtype_code(cd), dl, labels, al_d, ll_d, *rows,
                          B, T, U1, V, blank, ws, 1.0 / B, gscale, 0, db2_parts, ctx.fastemit_lambda)
            else:
                _lib.call("rnnt_loss_backward_band", logits, _lib.dtype_code(cd), dl, labels, al_d, ll_d, *rows,
                          B, T, U1, V, blank, ws, 1.0 / B, gscale, 0, ctx.fastemit_lambda)
        del logits
        with ops.timed("joint_dhid_gemm"):
            dhid = ops.gemm(dl, w2t)
        with ops.timed("joint_hidden_bwd"):
            _lib.call("joint_hidden_bwd_band", _lib.dtype_code(cd), dhid, hid, dE1, dD1, plan.band, plan.row_off,
                      ops._ll(M), B, T, U1, J)
        del dhid
        dE1c = ops.cast(dE1, cd).view(B * T, J)
        dD1c = ops.cast(dD1, cd).view(B * U1, J)
        denc = ops.gemm(dE1c, w1c[:, :P].t()).view(B, T, P)
        ddec = ops.gemm(dD1c, w1c[:, P:].t()).view(B, U1, P2)
        with side.WeightGrads(ctx, 2, (w1, ctx.b1, w2, ctx.b2), dl, hid, dE1c, dD1c, dD1, enc2, dec2, db2_parts) as wg:
            wg.gemm(2, dl.t(), hid.t(), split_k=ops.pick_split_k(V, J, M), aux=dict(split_k=8, max_wg_per_cu=2))
            wg.colsum(3, dl if db2_parts is None else db2_parts)
            wg.gemm(0, dE1c.t(), enc2.t(), cols=slice(None, P), split_k=ops.pick_split_k(J, P, B * T))
            wg.gemm(0, dD1c.t(), dec2.t(), cols=slice(P, None), split_k=ops.pick_split_k(J, P2, B * U1))
            wg.colsum(1, dD1.view(B * U1, J))
        ops.mark("joint_bwd:exit")
        return (denc, ddec, *wg.grads, *tail)

    @staticmethod
    def backward(ctx, gout):
        ops.mark("joint_bwd:enter")
        if ctx.plan is not None:
            return _JointLossFn._backward_band(ctx, gout)
        enc2, dec2, w1, w2, hid, logits, labels, al_d, ll_d, off_d, ws = ctx.saved_tensors
        cd, B, T, U1, P, P2, J, V, M, blank = ctx.cfg
        dl = torch.empty_like(logits)
        gscale = gout.contiguous().float()
        # the mean: one scale for the batch, times 1 / B on the host; per-row costs: a scale per utterance, as it came
        gs_host, gs_stride = (1.0, 1) if ctx.row_costs else (1.0 / B, 0)
        w1c = WEIGHTS.get(w1, cd)
        w2t = WEIGHTS.get(w2, cd, transposed=True)
        dE1 = torch.empty(B, T, J, dtype=F32, device=dl.device)
        dD1 = torch.empty(B, U1, J, dtype=F32, device=dl.device)
        # (pipelining the loss gradient against the dhid product by utterance groups on two streams was measured:
        # 21.70 ms per step in one pass, 21.74 / 22.26 / 23.18 with 2 / 4 / 8 groups - both sit on the L2/HBM path)
        # the output bias's gradient is the column sum of dl: the loss-gradient kernel leaves it as per-workgroup
        # partial rows (a few MB) instead of a second pass over dl beside the encoder's BPTT (0.4 ms per step)
        cs_rows = _lib.load().edgedict_rnnt_grad_colsum_rows(_lib.dtype_code(cd), B, T, U1, V) if config.FUSED_DB2 else 0
        db2_parts = torch.empty(cs_rows, V, dtype=F32, device=dl.device) if cs_rows > 0 else None
        lam = ctx.fastemit_lambda
        with ops.timed("rnnt_grad"):
            if ctx.restricted:
                # gradient kernels with the dead-cell test (the windows are in the workspace)
                if db2_parts is not None:
                    _lib.call("rnnt_loss_backward_packed_colsum_ar", logits, _lib.dtype_code(cd), dl, labels, al_d,
                              ll_d, off_d, B, T, U1, V, blank, ws, gs_host, gscale, gs_stride, db2_parts, lam)
                else:
                    _lib.call("rnnt_loss_backward_packed_ar", logits, _lib.dtype_code(cd), dl, labels, al_d, ll_d,
                              off_d, B, T, U1, V, blank, ws, gs_host, gscale, gs_stride, lam)
            elif lam != 0.0:
                if db2_parts is not None:
                    _lib.call("rnnt_loss_backward_packed_colsum_fe", logits, _lib.dtype_code(cd), dl, labels, al_d,
                              ll_d, off_d, B, T, U1, V, blank, ws, gs_host, gscale, gs_stride, db2_parts, lam)
                else:
                    _lib.call("rnnt_loss_backward_packed_fe", logits, _lib.dtype_code(cd), dl, labels, al_d, ll_d,
                              off_d, B, T, U1, V, blank, ws, gs_host, gscale, gs_stride, lam)
            elif db2_parts is not None:
                _lib.call("rnnt_loss_backward_packed_colsum", logits, _lib.dtype_code(cd), dl, labels, al_d, ll_d,
                          off_d, B, T, U1, V, blank, ws, gs_host, gscale, gs_stride, db2_parts)
            else:
                _lib.call("rnnt_loss_backward_packed", logits, _lib.dtype_code(cd), dl, labels, al_d, ll_d,
                          off_d, B, T, U1, V, blank, ws, gs_host, gscale, gs_stride)
        del logits
        with ops.timed("joint_dhid_gemm"):
            dhid = ops.gemm(dl, w2t)
        with ops.timed("joint_hidden_bwd"):
            _lib.call("joint_hidden_bwd_packed", _lib.dtype_code(cd), dhid, hid, dE1, dD1, al_d, ll_d,
                      off_d, B, T, U1, J)
        del dhid
        dE1c = ops.cast(dE1, cd).view(B * T, J)
        dD1c = ops.cast(dD1, cd).view(B * U1, J)
        denc = ops.gemm(dE1c, w1c[:, :P].t()).view(B, T, P)
        ddec = ops.gemm(dD1c, w1c[:, P:].t()).view(B, U1, P2)
        with side.WeightGrads(ctx, 2, (w1, ctx.b1, w2, ctx.b2), dl, hid, dE1c, dD1c, dD1, enc2, dec2, db2_parts) as wg:
            wg.gemm(2, dl.t(), hid.t(), split_k=ops.pick_split_k(V, J, M), aux=dict(split_k=8, max_wg_per_cu=2))
            wg.colsum(3, dl if db2_parts is None else db2_parts)
            wg.gemm(0, dE1c.t(), enc2.t(), cols=slice(None, P), split_k=ops.pick_split_k(J, P, B * T))
            wg.gemm(0, dD1c.t(), dec2.t(), cols=slice(P, None), split_k=ops.pick_split_k(J, P2, B * U1))
            wg.colsum(1, dD1.view(B * U1, J))
        ops.mark("joint_bwd:exit")
        return (denc, ddec, *wg.grads, None, None, None, None, None, None, None, None, None, None)


# ----------------------------------------------------------------------------------------
# parameter containers with the reference's names, shapes and default initialisation
class TimeReduction(nn.Module):
    """Marker for the 2x time reduction of rnnt/models.py:16-29; the arithmetic (zero-pad to an
    even length after the LayerNorm, mean of frame pairs) is fused into the LayerNorm kernel."""

    def __init__(self, reduction_factor=2):
        super().__init__()
        self.reduction_factor = reduction_factor


class _LayerNormParams(nn.Module):
    def __init__(self, size, eps=1e-5):
        super().__init__()
        self.normalized_shape = (size,)
        self.eps = eps
        self.weight = nn.Parameter(torch.ones(size))
        self.bias = nn.Parameter(torch.zeros(size))


class _LinearParams(nn.Module):
    def __init__(self, in_features, out_features):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.weight = nn.Parameter(torch.empty(out_features, in_features))
        self.bias = nn.Parameter(torch.empty(out_features))
        # nn.Linear default init
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        bound = 1.0 / math.sqrt(in_features)
        nn.init.uniform_(self.bias, -bound, bound)


class _LSTMParams(nn.Module):
    """nn.LSTM-compatible parameter set: weight_ih_l{k} [4H,I], weight_hh_l{k} [4H,H],
    bias_ih_l{k}, bias_hh_l{k} [4H]; gate order i,f,g,o; uniform(-1/sqrt(H), 1/sqrt(H))."""

    def __init__(self, input_size, hidden_size, num_layers=1, dropout=0.0):
        super().__init__()
        self.input_size, self.hidden_size = input_size, hidden_size
        self.num_layers, self.dropout = num_layers, dropout
        k = 1.0 / math.sqrt(hidden_size)
        for layer in range(num_layers):
            i = input_size if layer == 0 else hidden_size
            for name, shape in (("weight_ih", (4 * hidden_size, i)),
                                ("weight_hh", (4 * hidden_size, hidden_size)),
                                ("bias_ih", (4 * hidden_size,)),
                                ("bias_hh", (4 * hidden_size,))):
                p = nn.Parameter(torch.empty(*shape).uniform_(-k, k))
                setattr(self, "%s_l%d" % (name, layer), p)

    def layer(self, k):
        return tuple(getattr(self, "%s_l%d" % (n, k))
                     for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))

    def flatten_parameters(self):  # API compatibility (cuDNN concept; nothing to do here)
        pass


class ResLayerNormLSTM(nn.Module):
    """Stack of 1-layer LSTMs with residual connections, LayerNorm and optional time reduction
    (reference rnnt/models.py:32-75).  Padded frames are NOT masked, as in the reference."""

    def __init__(self, input_size, hidden_size, num_layers, dropout=0,
                 time_reductions=[1], reduction_factor=2):
        super().__init__()
        if reduction_factor != 2:
            raise ValueError("only reduction_factor=2 is implemented (the reference default)")
        self.dropout = dropout      # nn.Dropout after LayerNorm(+TimeReduction), rnnt/models.py:47-53
        self.hidden_size = hidden_size
        self.lstms = nn.ModuleList()
        self.projs = nn.ModuleList()
        self.reductions = []
        for i in range(num_layers):
            self.lstms.append(_LSTMParams(input_size, hidden_size, 1))
            proj = [_LayerNormParams(hidden_size)]
            if i in time_reductions:
                proj.append(TimeReduction(reduction_factor))
            self.reductions.append(2 if i in time_reductions else 1)
            input_size = hidden_size
            self.projs.append(nn.Sequential(*proj))

    def forward(self, xs, hiddens=None, cd=None):
        cd = cd or config.get_compute_dtype()
        xs = _to_cd(xs, cd) if xs.dtype != cd else xs
        new_hs, new_cs = [], []
        for i, (lstm, proj) in enumerate(zip(self.lstms, self.projs)):
            h0 = c0 = None
            if hiddens is not None:
                h0, c0 = _state(hiddens[0][i]), _state(hiddens[1][i])
            w_ih, w_hh, b_ih, b_hh = lstm.layer(0)
            xs, h, c = _LSTMBlockFn.apply(xs.contiguous(), w_ih, w_hh, b_ih, b_hh,
                                          proj[0].weight, proj[0].bias, h0, c0, i != 0,
                                          self.reductions[i], cd)
            if self.dropout > 0 and self.training:
                xs = _dropout(xs, self.dropout)
            new_hs.append(h)
            new_cs.append(c)
        return xs, (torch.stack(new_hs, 0), torch.stack(new_cs, 0))


class _GRUParams(nn.Module):
    """nn.GRU-compatible 1-layer parameter set: weight_ih_l0 [3H,I], weight_hh_l0 [3H,H],
    bias_ih_l0, bias_hh_l0 [3H]; gate order r,z,n; uniform(-1/sqrt(H), 1/sqrt(H))."""

    def __init__(self, input_size, hidden_size):
        super().__init__()
        self.input_size, self.hidden_size, self.num_layers = input_size, hidden_size, 1
        k = 1.0 / math.sqrt(hidden_size)
        for name, shape in (("weight_ih", (3 * hidden_size, input_size)),
                            ("weight_hh", (3 * hidden_size, hidden_size)),
                            ("bias_ih", (3 * hidden_size,)), ("bias_hh", (3 * hidden_size,))):
            setattr(self, name + "_l0", nn.Parameter(torch.empty(*shape).uniform_(-k, k)))

    def layer(self, k=0):
        return tuple(getattr(self, n + "_l0") for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))

    def flatten_parameters(self):
        pass


class ResLayerNormGRU(nn.Module):
    """Stack of 1-layer GRUs with residual connections, LayerNorm and optional time reduction
    (reference rnnt/models.py:77-116; the module list is called ``lstms`` there too, so the
    state-dict keys are those of the LSTM variant with 3H rows).  ``hiddens`` is ONE tensor
    [L,B,H].  Per-layer kernels only (csrc/gru.hip): this variant is a compatibility module."""

    def __init__(self, input_size, hidden_size, num_layers, dropout=0,
                 time_reductions=[1], reduction_factor=2):
        super().__init__()
        if reduction_factor != 2:
            raise ValueError("only reduction_factor=2 is implemented (the reference default)")
        self.dropout = dropout
        self.hidden_size = hidden_size
        self.lstms = nn.ModuleList()
        self.projs = nn.ModuleList()
        self.reductions = []
        for i in range(num_layers):
            self.lstms.append(_GRUParams(input_size, hidden_size))
            proj = [_LayerNormParams(hidden_size)]
            if i in time_reductions:
                proj.append(TimeReduction(reduction_factor))
            self.reductions.append(2 if i in time_reductions else 1)
            input_size = hidden_size
            self.projs.append(nn.Sequential(*proj))

    def forward(self, xs, hiddens=None, cd=None):
        cd = cd or config.get_compute_dtype()
        xs = _to_cd(xs, cd) if xs.dtype != cd else xs
        new_hs = []
        for i, (gru, proj) in enumerate(zip(self.lstms, self.projs)):
            h0 = _state(hiddens[i]) if hiddens is not None else None
            w_ih, w_hh, b_ih, b_hh = gru.layer(0)
            xs, h = _GRUBlockFn.apply(xs.contiguous(), w_ih, w_hh, b_ih, b_hh, proj[0].weight,
                                      proj[0].bias, h0, i != 0, self.reductions[i], cd)
            if self.dropout > 0 and self.training:
                xs = _dropout(xs, self.dropout)
            new_hs.append(h)
        return xs, torch.stack(new_hs, 0)


class Encoder(nn.Module):
    """LayerNorm -> ResLayerNormLSTM -> Linear (reference rnnt/models.py:119-136)."""

    def __init__(self, input_size, hidden_size, num_layers, dropout, proj_size,
                 module=ResLayerNormLSTM, time_reductions=[1], has_proj=True):
        super().__init__()
        self.norm = _LayerNormParams(input_size)
        self.lstm = module(input_size, hidden_size, num_layers, dropout=dropout,
                           time_reductions=time_reductions)
        self.has_proj = has_proj
        if has_proj:
            self.proj = _LinearParams(hidden_size, proj_size)

    def output_frames(self, T):
        """Frames the encoder returns for ``T`` input frames (every time reduction rounds up)."""
        for r in self.lstm.reductions:
            T = (T + r - 1) // r
        return T

    def forward(self, xs, hiddens=None):
        require_cuda(xs)
        cd = getattr(self, "compute_dtype", None) or config.get_compute_dtype()
        lstm = self.lstm
        drop = getattr(lstm, "dropout", 0) > 0 and self.training    # applied inside the stack / by the per-layer path
        # short inputs (streaming chunks of a few frames) stay on the per-layer kernels: the
        # wavefront needs ~5 lags of launches to fill, more than 6 x T per-layer steps for small T
        if (isinstance(lstm, ResLayerNormLSTM) and xs.dim() == 3
                and xs.shape[1] >= config.STACK_MIN_FRAMES
                and encoder_stack.supported(cd, lstm.hidden_size, xs.shape[2], len(lstm.lstms),
                                            lstm.reductions)):
            # bf16: input LayerNorm + all layers as one layer-pipelined native call per direction
            h0 = c0 = None
            if hiddens is not None:
                h0 = _state(hiddens[0]).contiguous()
                c0 = _state(hiddens[1]).contiguous()
            params = []
            for m, proj in zip(lstm.lstms, lstm.projs):
                params += list(m.layer(0)) + [proj[0].weight, proj[0].bias]
            # nn.Dropout behind every layer's LayerNorm (+ TimeReduction), rnnt/models.py:47-53,70: inside the stack's
            # norm role, one seed per layer drawn in the order the per-layer path draws them
            dcfg = (float(lstm.dropout), tuple(_next_dropout_seed() for _ in lstm.lstms)) if drop else None
            xs, h, c = encoder_stack.EncoderStackFn.apply(
                xs, self.norm.weight, self.norm.bias, h0, c0, tuple(lstm.reductions), None, dcfg, *params)
            hiddens = (h, c)
        elif (isinstance(lstm, ResLayerNormLSTM) and xs.dim() == 3 and cd == torch.bfloat16 and not drop
              and not torch.is_grad_enabled() and 0 < xs.shape[1] < config.STACK_MIN_FRAMES
              and xs.shape[0] <= (config.STREAM_STEP_MAX_ROWS_SHORT if xs.shape[1] <= 2 else config.STREAM_STEP_MAX_ROWS)
              and lstm.hidden_size % 32 == 0 and xs.shape[2] % 8 == 0 and config.STREAM_ENCODER_STEP):
            # streaming chunks of a FEW streams (rnnt/stream.py:93-100: a frame or two per call): ONE native call, a
            # fused launch per layer-frame (csrc/decode_fused.hip, edgedict_stream_encoder_step) - 0.39 instead of
            # 0.67 ms per chunk for one stream, 0.33 instead of 0.61 for 256; longer chunks of many streams stay on the
            # per-layer kernels, which batch the input product over the frames (config.STREAM_STEP_MAX_ROWS*)
            xs, hiddens = _stream_encoder_step(self, xs, hiddens)
        else:
            xs = _InputNormFn.apply(xs, self.norm.weight, self.norm.bias, cd)
            xs, hiddens = self.lstm(xs, hiddens, cd)
        if self.has_proj:
            xs = _LinearFn.apply(xs, self.proj.weight, self.proj.bias, cd)
        return xs, hiddens


def _stream_encoder_step(enc, xs, hiddens):
    """Input LayerNorm + the ResLayerNormLSTM loop (rnnt/models.py:55-75,124,131-134) for a chunk of a few frames in
    bf16, inference only: ``edgedict_stream_encoder_step``.  Returns (out [B, T', H] bf16, (h, c) [L, B, H] fp32)."""
    import ctypes
    lstm = enc.lstm
    B, T, I0 = xs.shape
    H, L = lstm.hidden_size, len(lstm.lstms)
    dev = xs.device
    x = xs.contiguous()
    if x.dtype not in (F32, torch.bfloat16):
        x = x.float()
    if hiddens is None:
        h = torch.zeros(L, B, H, dtype=F32, device=dev)
        c = torch.zeros(L, B, H, dtype=F32, device=dev)
    else:                                                  # new tensors: the caller's state is not modified in place
        h = _state(hiddens[0]).clone()
        c = _state(hiddens[1]).clone()
    cd = torch.bfloat16
    w_ih = [WEIGHTS.get(m.layer(0)[0], cd) for m in lstm.lstms]
    w_hh = [WEIGHTS.get(m.layer(0)[1], cd) for m in lstm.lstms]
    b_ih = [m.layer(0)[2].detach() for m in lstm.lstms]
    b_hh = [m.layer(0)[3].detach() for m in lstm.lstms]
    g = [p[0].weight.detach() for p in lstm.projs]
    bt = [p[0].bias.detach() for p in lstm.projs]
    T_out = enc.output_frames(T)
    out = torch.empty(B, T_out, H, dtype=cd, device=dev)
    lib = _lib.load()
    ws = torch.empty(lib.edgedict_stream_encoder_workspace_bytes(B, T, I0, H, L), dtype=torch.uint8, device=dev)

    def arr(ts):
        return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    red = (ctypes.c_int * L)(*[int(r) for r in lstm.reductions])
    t_out = ctypes.c_int(0)
    rc = lib.edgedict_stream_encoder_step(
        _lib.ptr(x), _lib.dtype_code(x.dtype), B, T, I0, H, L, _lib.ptr(enc.norm.weight.detach()),
        _lib.ptr(enc.norm.bias.detach()), arr(w_ih), arr(w_hh), arr(b_ih), arr(b_hh), arr(g), arr(bt), red,
        _lib.ptr(h), _lib.ptr(c), _lib.ptr(out), ctypes.byref(t_out), _lib.ptr(ws), _lib.stream_ptr())
    _lib.check(rc, "stream_encoder_step")
    assert t_out.value == T_out
    return out, (h, c)


class Decoder(nn.Module):
    """Prediction network: Embedding -> multi-layer LSTM -> Linear (rnnt/models.py:139-157)."""

    def __init__(self, vocab_embed_size, vocab_size, hidden_size, num_layers,
                 dropout=0, proj_size=None):
        super().__init__()
        self.embed = nn.Embedding(vocab_size, vocab_embed_size, padding_idx=PAD)  # container
        self.lstm = _LSTMParams(vocab_embed_size, hidden_size, num_layers, dropout)
        self.proj = _LinearParams(hidden_size, proj_size)
        self.dropout = dropout

    def forward(self, ys, hidden=None):
        require_cuda(self.embed.weight)
        cd = getattr(self, "compute_dtype", None) or config.get_compute_dtype()
        prepend = hidden is None
        tokens = ys.to(device=self.embed.weight.device, dtype=torch.int32)
        if tokens.dim() != 2:
            raise ValueError("decoder expects token ids of shape [B, U]")
        if not tokens.is_contiguous():
            tokens = tokens.contiguous()
        x = _EmbeddingFn.apply(tokens, self.embed.weight, prepend, cd)
        hs, cs = [], []
        for k in range(self.lstm.num_layers):
            h0 = c0 = None
            if hidden is not None:
                h0, c0 = _state(hidden[0][k]), _state(hidden[1][k])
            w_ih, w_hh, b_ih, b_hh = self.lstm.layer(k)
            x, h, c = _LSTMBlockFn.apply(x, w_ih, w_hh, b_ih, b_hh, None, None, h0, c0,
                                         False, 1, cd)
            # nn.LSTM(dropout=p): on the outputs of every layer except the last, training only
            if self.dropout > 0 and self.training and k + 1 < self.lstm.num_layers:
                x = _dropout(x, self.dropout)
            hs.append(h)
            cs.append(c)
        y = _LinearFn.apply(x, self.proj.weight, self.proj.bias, cd)
        return y, (torch.stack(hs, 0), torch.stack(cs, 0))


class Joint(nn.Module):
    """Linear(P_enc+P_dec, J) -> Tanh -> Linear(J, V) on every (t, u) pair
    (rnnt/models.py:160-179).  Returns raw logits."""

    def __init__(self, input_size, hidden_size, vocab_size):
        super().__init__()
        self.joint = nn.Sequential(_LinearParams(input_size, hidden_size), nn.Tanh(),
                                   _LinearParams(hidden_size, vocab_size))

    def forward(self, h_enc, h_dec):
        require_cuda(h_enc, h_dec)
        cd = getattr(self, "compute_dtype", None) or config.get_compute_dtype()
        l1, l2 = self.joint[0], self.joint[2]
        if h_enc.dim() == 3 and h_dec.dim() == 3:
            e, d = _to_cd(h_enc, cd), _to_cd(h_dec, cd)
            return _JointFn.apply(e, d, l1.weight, l1.bias, l2.weight, l2.bias, cd)
        if h_enc.dim() != h_dec.dim() or h_enc.dim() != 2:
            raise ValueError("joint expects two 3-D or two 2-D inputs")
        e, d = _to_cd(h_enc, cd)[:, None], _to_cd(h_dec, cd)[:, None]
        out = _JointFn.apply(e, d, l1.weight, l1.bias, l2.weight, l2.bias, cd)
        return out[:, 0, 0]


class Transducer(nn.Module):
    """RNN-Transducer with the reference's constructor and methods (rnnt/models.py:182-269)."""

    def __init__(self,
                 vocab_embed_size, vocab_size, input_size,
                 enc_hidden_size, enc_layers, enc_dropout, enc_proj_size,
                 dec_hidden_size, dec_layers, dec_dropout, dec_proj_size,
                 joint_size, enc_time_reductions=[1],
                 blank=NUL, module_type='LSTM', output_loss=True, *, fastemit_lambda=0.0, ctc_weight=0.0):
        super().__init__()
        self.blank = blank
        # CTC auxiliary head (loss.CTCLoss): forward() returns rnnt + ctc_weight * ctc.  A plain attribute that may be
        # changed later; the head's parameters exist iff it is > 0 HERE (registered last, below), and at 0 forward()
        # skips the branch entirely - the launches, parameters and state-dict keys of a model without it.
        self.ctc_weight = self._check_ctc_weight(ctc_weight)
        self.loss_parts = None
        # FastEmit (loss.py): a plain attribute - no parameter, no buffer, the state dict's keys do not change.  Scales
        # the gradient through the label emissions by 1 + lambda; the loss forward() returns stays the plain one.
        from .loss import check_fastemit_lambda
        self.fastemit_lambda = check_fastemit_lambda(fastemit_lambda)
        if module_type not in ['GRU', 'LSTM']:
            raise ValueError('Unsupported module type')
        self.encoder = Encoder(input_size=input_size, hidden_size=enc_hidden_size,
                               num_layers=enc_layers, dropout=enc_dropout,
                               proj_size=enc_proj_size, time_reductions=enc_time_reductions,
                               module=ResLayerNormGRU if module_type == 'GRU' else ResLayerNormLSTM)
        self.decoder = Decoder(vocab_embed_size=vocab_embed_size, vocab_size=vocab_size,
                               hidden_size=dec_hidden_size, num_layers=dec_layers,
                               dropout=dec_dropout, proj_size=dec_proj_size)
        self.joint = Joint(input_size=enc_proj_size + dec_proj_size, hidden_size=joint_size,
                           vocab_size=vocab_size)
        self.output_loss = output_loss
        if self.ctc_weight > 0:
            self.ctc_head = _LinearParams(enc_proj_size, vocab_size)

    @staticmethod
    def _check_ctc_weight(value):
        w = float(value)
        if not (w >= 0.0 and math.isfinite(w)):
            raise ValueError("ctc_weight must be finite and >= 0, got %r" % (value,))
        return w

    # compute dtype shared with the sub-modules -----------------------------------------
    @property
    def compute_dtype(self):
        return getattr(self.encoder, "compute_dtype", None) or config.get_compute_dtype()

    @compute_dtype.setter
    def compute_dtype(self, value):
        value = config._parse(value)
        for m in (self.encoder, self.decoder, self.joint):
            m.compute_dtype = value

    def scale_length(self, logits, xlen):
        # rnnt/models.py:223-226 (host-side integer logic on a [B] tensor)
        return self._scale_to(logits.shape[1], xlen)

    @staticmethod
    def _scale_to(T, xlen):
        """scale_length's arithmetic for an encoder output of ``T`` frames."""
        scale = (xlen.max().float() / T).ceil()
        xlen = (xlen / scale).ceil().int()
        return xlen

    def _band_plan(self, xs, xlen, ylen, lo, hi):
        """Start the band plan of forward() (config.BAND_LATTICE): it depends on the windows and the lengths only, so
        its device work and the copy of its row total are enqueued BEFORE the encoder - forward() picks the total up
        (``plan.finish()``: one event, recorded in front of the encoder) once the encoder and the prediction network
        are enqueued."""
        from ._staging import to_device
        from .loss import rnnt_band_plan
        T = self.encoder.output_frames(xs.shape[1])
        al_d = to_device(self._scale_to(T, xlen).to(torch.int32), xs.device)
        ll_d = to_device(ylen.to(torch.int32), xs.device)
        return rnnt_band_plan(lo, hi, al_d, ll_d, T, finish=False)

    def _windows(self, windows, B, U, device):
        """``windows=(lo, hi)`` of forward() / align(): int32 [B, >= U] device tensors, cut to the label columns in use
        (as ``ys`` is) and validated as the loss validates them."""
        from .loss import check_windows
        if not isinstance(windows, (tuple, list)) or len(windows) != 2:
            raise TypeError("windows must be a pair (lo, hi) of int32 [B, U] tensors")
        lo, hi = windows
        if torch.is_tensor(lo) and torch.is_tensor(hi) and lo.dim() == 2 and hi.dim() == 2:
            lo, hi = lo[:, :U].contiguous(), hi[:, :U].contiguous()
        return check_windows((lo, hi), B, U, device)

    def _ctc_logits(self, h_enc):
        """Head logits [B, T', V] of the encoder output (the GEMM front door, in the compute dtype)."""
        head = getattr(self, "ctc_head", None)
        if head is None:
            raise RuntimeError("this model has no CTC head: construct it with Transducer(..., ctc_weight > 0)")
        cd = self.compute_dtype
        return _LinearFn.apply(_to_cd(h_enc, cd), head.weight, head.bias, cd)

    def _ctc_loss(self, h_enc, ys, act, ylen):
        """The auxiliary term of forward(): CTC 'mean' loss of the head on ``h_enc`` with the frame counts ``act`` of
        ``scale_length``.  zero_infinity: time reduction can leave a short utterance fewer frames than its labels plus
        repeats, and an auxiliary term must not turn the logged loss into +inf.  No host sync."""
        from ._staging import to_device
        from .loss import _CTCLossFn
        dev = h_enc.device
        logits = self._ctc_logits(h_enc).contiguous()

        def lens(t):
            if t.is_cuda:
                return t.to(device=dev, dtype=torch.int32).contiguous()
            return to_device(t.to(torch.int32), dev)

        labels = ys.to(device=dev, dtype=torch.int32).contiguous()
        return _CTCLossFn.apply(logits, labels, lens(act), lens(ylen), self.blank, "mean", True)

    def _with_ctc(self, rnnt, ctc):
        self.loss_parts = (rnnt.detach(), ctc.detach())
        return rnnt + self.ctc_weight * ctc

    @torch.no_grad()
    def ctc_greedy_decode(self, xs, xlen):
        """First-pass decode from the encoder alone: encoder, CTC head, ``loss.ctc_greedy`` - neither the prediction
        network nor the joint runs.  Returns (list of int64 numpy token arrays WITHOUT blanks, repeats collapsed;
        -sum log p of the kept frames as a [B] tensor): the return shape of ``greedy_decode``.  Raises RuntimeError on
        a model built without ``ctc_weight > 0``."""
        from .loss import ctc_greedy
        if getattr(self, "ctc_head", None) is None:
            raise RuntimeError("this model has no CTC head: construct it with Transducer(..., ctc_weight > 0)")
        xs = xs[:, :xlen.max()].contiguous()
        h_enc, _ = self.encoder(xs)
        act = self.scale_length(h_enc, xlen).to(device=h_enc.device, dtype=torch.int32).contiguous()
        tokens, counts, _, neglogp = ctc_greedy(self._ctc_logits(h_enc).contiguous(), act, self.blank)
        tokens, counts = tokens.cpu().numpy(), counts.cpu().numpy()
        return [tokens[b, :counts[b]].astype("int64") for b in range(tokens.shape[0])], neglogp

    def _ctc_align(self, xs, ys, xlen, ylen):
        """encoder, head, ``loss.ctc_align``: (frames, ends, scores, act_lens, label_lens), the lengths int32 on the
        device as the aligner read them."""
        from ._staging import to_device
        from .loss import ctc_align
        if getattr(self, "ctc_head", None) is None:
            raise RuntimeError("this model has no CTC head: construct it with Transducer(..., ctc_weight > 0)")
        xs = xs[:, :xlen.max()].contiguous()
        ys = ys[:, :ylen.max()].contiguous()
        h_enc, _ = self.encoder(xs)
        dev = h_enc.device

        def lens(t):
            if t.is_cuda:
                return t.to(device=dev, dtype=torch.int32).contiguous()
            return to_device(t.to(torch.int32), dev)

        act, lab = lens(self.scale_length(h_enc, xlen)), lens(ylen)
        labels = ys.to(device=dev, dtype=torch.int32).contiguous()
        frames, ends, scores = ctc_align(self._ctc_logits(h_enc).contiguous(), labels, act, lab, self.blank,
                                         check_lengths=False)
        return frames, ends, scores, act, lab

    @torch.no_grad()
    def ctc_align(self, xs, ys, xlen, ylen):
        """Forced alignment of the transcripts ``ys`` by the CTC head (encoder, head, ``loss.ctc_align`` - neither the
        prediction network nor the joint runs, no ``T x U x V`` lattice is formed): returns ``(frames, ends, scores)``,
        ``frames`` / ``ends`` int32 ``[B, U]`` with the first and the last ENCODER frame (after the time reductions, as
        ``scale_length`` counts them) the best CTC path spends in each label, -1 behind ``ylen[b]``; ``scores`` float32
        ``[B]``, that path's log-probability.  A row without a CTC path (fewer encoder frames than labels plus adjacent
        repeats) has score -inf and frames / ends of all -1.  ``decode.emission_times`` turns either into seconds.
        Arguments as ``forward``; no host sync.  Leaves no state behind: run it in ``eval()`` mode, or dropout takes
        part.  Raises RuntimeError on a model built without ``ctc_weight > 0``."""
        return self._ctc_align(xs, ys, xlen, ylen)[:3]

    @torch.no_grad()
    def ctc_windows(self, xs, ys, xlen, ylen, left, right):
        """Emission windows from the CTC head alone: ``ctc_align`` followed by ``loss.alignment_windows(frames, act,
        ylen, left, right)``.  Returns ``(lo, hi)`` int32 ``[B, U]`` on the device, ready for ``forward(...,
        windows=)``, ``align(..., windows=)`` and ``TrainEngine.train_step(..., windows=)``.  A CTC alignment's frames
        are strictly increasing and at most ``T_b - 1``, so windows that contain them always admit an RNN-T alignment
        (which needs them non-decreasing only).  A row without a CTC path (frames of -1) gets ``lo = 0, hi = T - 1`` in
        every column - the padding rule of ``alignment_windows``, ``T = max(act_lens)`` - so it stays unrestricted
        rather than dead.  Remarks of ``ctc_align`` (``eval()``, the missing head) apply."""
        from .loss import alignment_windows
        frames, _, scores, act, lab = self._ctc_align(xs, ys, xlen, ylen)
        # a row without a path counts as having no labels: alignment_windows then pads every column of it
        lab = torch.where(scores == float("-inf"), torch.zeros_like(lab), lab)
        return alignment_windows(frames, act, lab, left, right)

    def ctc_beam_search(self, xs, xlen, W=10, cand=None, bias=None, *, lm=None, lm_weight=None, length_bonus=0.0):
        """First-pass N-best from the encoder alone: encoder, CTC head, the CTC prefix beam search
        (``loss.ctc_prefix_beam``), one read to the host.  Returns a list of ``decode.NBestResult``, one per utterance,
        ranked (``logp`` descending, entry 0 the answer); ``bias`` (an ``edgedict_amd.bias.ContextGraph``) boosts a
        phrase list, ``lm`` (an ``edgedict_amd.ngram.NGramLM``, with ``lm_weight`` and ``length_bonus``) fuses a
        back-off n-gram into the search.  See ``decode.ctc_beam_search``.  Raises RuntimeError on a model built without ``ctc_weight > 0``."""
        from .decode import ctc_beam_search
        return ctc_beam_search(self, xs, xlen, W, cand, bias, lm=lm, lm_weight=lm_weight, length_bonus=length_bonus)

    def _ctc_encode(self, xs, xlen):
        """The encoder as the N-best searches run it: (enc_out contiguous, host int32 frame counts or None)."""
        if getattr(self, "ctc_head", None) is None:
            raise RuntimeError("this model has no CTC head: construct it with Transducer(..., ctc_weight > 0)")
        from . import _lib
        _lib.require_cuda(xs)
        enc_out, _ = self.encoder(xs)
        enc_out = enc_out.contiguous()
        if xlen is None:
            return enc_out, None
        xl = xlen.detach().cpu() if torch.is_tensor(xlen) else torch.as_tensor(xlen)
        return enc_out, self.scale_length(enc_out, xl).numpy().astype("int32")

    @torch.no_grad()
    def ctc_score(self, xs, xlen, hyps):
        """The CTC head's log-likelihood of given token sequences: ``hyps[b]`` is a list of sequences (ints, no blanks;
        at most 32 per utterance) to score on utterance ``b``.  Encoder, head, ``loss.ctc_score_nbest`` on all of them
        at once, one read to the host - neither the prediction network nor the joint runs.  Returns a list of float64
        numpy arrays, one value per sequence: minus the CTC cost of that transcript over the utterance's encoder
        frames, -inf where the head has no path for it (fewer frames than tokens plus adjacent repeats).  ``xlen`` as
        the beam searches take it (None: all frames).  Raises RuntimeError on a model built without
        ``ctc_weight > 0``."""
        from .decode import ctc_score_lists
        enc_out, lens = self._ctc_encode(xs, xlen)
        return ctc_score_lists(self, enc_out, lens, hyps)

    @torch.no_grad()
    def rescore_nbest(self, xs, xlen, results, weight):
        """Joint CTC / transducer rescoring of N-best lists obtained elsewhere (``ctc_beam_search``, a streaming
        search's ``nbest()``, a list read from disk): the encoder, then ``decode.ctc_rescore`` - ``ctc_logp`` filled,
        ``logp`` replaced by ``logp + weight * ctc_logp``, every list sorted by it.  What ``beam_search_nbest(...,
        ctc_rescore=weight)`` does to its own lists.  ``weight`` finite and ``>= 0``, else ``ValueError``.  Raises
        RuntimeError on a model built without ``ctc_weight > 0``."""
        from .decode import _check_rescore, ctc_rescore
        _check_rescore(self, weight)
        enc_out, lens = self._ctc_encode(xs, xlen)
        return ctc_rescore(self, enc_out, lens, results, weight)

    def forward(self, xs, ys, xlen, ylen, *, windows=None):
        """The reference's forward (rnnt/models.py:209-241).  ``windows=(lo, hi)`` (keyword only): the
        alignment-restricted loss of ``loss.RNNTLoss`` on either loss path, in ENCODER frames as ``align`` counts them;
        a batch with an utterance whose windows admit no alignment returns ``+inf`` (zero gradient for that utterance)."""
        xs = xs[:, :xlen.max()].contiguous()
        ys = ys[:, :ylen.max()].contiguous()
        if windows is not None and not self.output_loss:
            raise ValueError("windows need output_loss=True")
        if xs.is_cuda and not ys.is_cuda:
            # a host-side label batch (seq_collate output with only xs uploaded): one upload here,
            # the prediction network and the loss kernels both read the device copy
            ys = ys.to(xs.device, non_blocking=True)
        plan = checked = None
        if (windows is not None and config.BAND_LATTICE and config.PACKED_LATTICE and not xlen.is_cuda
                and not ylen.is_cuda and xs.dim() == 3 and xs.is_cuda):
            checked = self._windows(windows, ys.shape[0], ys.shape[1], xs.device)
            plan = self._band_plan(xs, xlen, ylen, *checked)
        if config.DECODER_ON_AUX_STREAM and xs.is_cuda:
            # the prediction network does not depend on the encoder: it runs on the auxiliary
            # stream under the encoder's recurrences.  Autograd replays each node on its forward
            # stream, so its backward overlaps the encoder's backward the same way.
            main = torch.cuda.current_stream(xs.device)
            aux = side.stream(xs.device)
            ready = main.record_event()          # ys (and the parameters) are ready here
            if config.DECODER_ENQUEUE_FIRST:
                aux.wait_event(ready)
                ys.record_stream(aux)
                with torch.cuda.stream(aux):
                    h_dec, _ = self.decoder(ys)
                h_enc, _ = self.encoder(xs)
            else:
                h_enc, _ = self.encoder(xs)          # enqueued first: it is the long pole
                aux.wait_event(ready)
                ys.record_stream(aux)
                with torch.cuda.stream(aux):
                    h_dec, _ = self.decoder(ys)
            main.wait_stream(aux)
            h_dec.record_stream(main)
        else:
            h_enc, _ = self.encoder(xs)
            h_dec, _ = self.decoder(ys)
        # CTC auxiliary term: on the main stream, between the encoder and the joint; at weight 0 nothing is launched
        use_ctc = self.output_loss and self.ctc_weight > 0
        ctc = self._ctc_loss(h_enc, ys, self.scale_length(h_enc, xlen), ylen) if use_ctc else None
        ops.mark("joint:enter")
        if (self.output_loss and config.PACKED_LATTICE and not xlen.is_cuda and not ylen.is_cuda
                and h_enc.dim() == 3 and h_enc.is_cuda):
            # lengths on the host: joint + loss on the packed lattice (no padding rows anywhere)
            cd = self.compute_dtype
            l1, l2 = self.joint.joint[0], self.joint.joint[2]
            act = self.scale_length(h_enc, xlen)
            # the loss kernels take a raw device pointer: a host-side label batch (seq_collate
            # output with only xs uploaded) is moved, as Decoder.forward does for its own copy
            labels = ys.to(device=h_enc.device, dtype=torch.int32).contiguous()
            if windows is None:
                loss = _JointLossFn.apply(_to_cd(h_enc, cd), _to_cd(h_dec, cd), l1.weight, l1.bias,
                                          l2.weight, l2.bias, labels, act, ylen, self.blank, cd, self.fastemit_lambda)
            else:
                lo, hi = checked or self._windows(windows, labels.shape[0], labels.shape[1], h_enc.device)
                if plan is not None:
                    if plan.band.shape[1] != h_enc.shape[1]:
                        raise RuntimeError("band plan built for %d encoder frames, the encoder returned %d"
                                           % (plan.band.shape[1], h_enc.shape[1]))
                    plan.finish()                # the one host read: an event in front of the encoder's work
                loss = _JointLossFn.apply(_to_cd(h_enc, cd), _to_cd(h_dec, cd), l1.weight, l1.bias, l2.weight, l2.bias,
                                          labels, act, ylen, self.blank, cd, self.fastemit_lambda, lo, hi, plan)
            ops.mark("joint:exit")
            return self._with_ctc(loss, ctc) if use_ctc else loss
        logits = self.joint(h_enc, h_dec)
        ops.mark("joint:exit")
        if self.output_loss:
            xlen = self.scale_length(logits, xlen)
            dev = logits.device   # lengths may live on the host (no sync for the slicing above)
            labels = ys.to(device=dev, dtype=torch.int32).contiguous()
            tail = () if windows is None else self._windows(windows, labels.shape[0], labels.shape[1], dev)
            loss = _RNNTLossFn.apply(
                logits, labels,
                xlen.to(device=dev, dtype=torch.int32, non_blocking=True).contiguous(),
                ylen.to(device=dev, dtype=torch.int32, non_blocking=True).contiguous(),
                self.blank, "mean", self.fastemit_lambda, *tail)
            return self._with_ctc(loss, ctc) if use_ctc else loss
        return logits

    @torch.no_grad()
    def align(self, xs, ys, xlen, ylen, *, windows=None):
        """Forced alignment of the transcripts ``ys`` (``loss.rnnt_align`` on this model's joint logits): returns
        ``(frames, scores)``, ``frames`` int32 ``[B, U]`` with the ENCODER frame (after the time reductions, as
        ``scale_length`` counts them) on which each label is emitted, -1 behind ``ylen[b]``; ``scores`` float32 ``[B]``, the
        log-probability of the best alignment.  ``decode.emission_times`` turns the frames into seconds.  Arguments as
        ``forward``; with host-side lengths the joint runs on the packed lattice as the training path does (the dense
        logits are never formed).  Leaves no state behind: run it in ``eval()`` mode, or dropout takes part.
        ``windows=(lo, hi)`` (keyword only, as ``forward``): the best alignment among those that respect the windows; a
        row whose windows admit none has score -inf and frames of all -1."""
        from ._staging import to_device
        xs = xs[:, :xlen.max()].contiguous()
        ys = ys[:, :ylen.max()].contiguous()
        if xs.is_cuda and not ys.is_cuda:
            ys = ys.to(xs.device)
        h_enc, _ = self.encoder(xs)
        h_dec, _ = self.decoder(ys)
        act = self.scale_length(h_enc, xlen)
        dev = h_enc.device
        labels = ys.to(device=dev, dtype=torch.int32).contiguous()
        if windows is not None:
            windows = self._windows(windows, labels.shape[0], labels.shape[1], dev)
        if not (config.PACKED_LATTICE and not xlen.is_cuda and not ylen.is_cuda and h_enc.is_cuda):
            from .loss import rnnt_align
            return rnnt_align(self.joint(h_enc, h_dec).contiguous(), labels,
                              act.to(device=dev, dtype=torch.int32).contiguous(),
                              ylen.to(device=dev, dtype=torch.int32).contiguous(), self.blank, windows=windows)
        cd = self.compute_dtype
        l1, l2 = self.joint.joint[0], self.joint.joint[2]
        enc, dec = _to_cd(h_enc, cd), _to_cd(h_dec, cd)
        B, T, P = enc.shape
        U1, P2 = dec.shape[1], dec.shape[2]
        J, V = l1.weight.shape[0], l2.weight.shape[0]
        al = act.to(torch.int64).cpu()
        ll = ylen.to(torch.int64).cpu()
        if int(al.max()) != T or int(ll.max()) != U1 - 1 or int(al.min()) < 1 or int(ll.min()) < 0:
            raise ValueError("Input length mismatch")
        rows = al * (ll + 1)
        off = torch.zeros(B, dtype=torch.int64)
        off[1:] = torch.cumsum(rows, 0)[:-1]
        M = int(rows.sum())
        off_d = to_device(off, dev)
        al_d = to_device(al.to(torch.int32), dev)
        ll_d = to_device(ll.to(torch.int32), dev)
        w1c = WEIGHTS.get(l1.weight, cd)
        w2c = WEIGHTS.get(l2.weight, cd)
        E1 = ops.gemm(enc.reshape(B * T, P), w1c[:, :P])
        D1 = ops.gemm(dec.reshape(B * U1, P2), w1c[:, P:], bias=l1.bias.detach())
        hid = torch.empty(M, J, dtype=cd, device=dev)
        _lib.call("joint_hidden_fwd_packed", _lib.dtype_code(cd), E1, D1, hid, al_d, ll_d, off_d, B, T, U1, J)
        ws = torch.empty(_lib.load().edgedict_rnnt_workspace_bytes(B, T, U1), dtype=torch.uint8, device=dev)
        frames = torch.empty(B, U1 - 1, dtype=torch.int32, device=dev)
        scores = torch.empty(B, dtype=F32, device=dev)
        if config.FUSED_LSE and cd == torch.bfloat16 and J >= 128 and J % 64 == 0 and V % 8 == 0 and M >= 256:
            slots = (V + 63) // 64
            parts = torch.empty(M, slots, 2, dtype=F32, device=dev)
            logits = torch.empty(M, V, dtype=cd, device=dev)
            _lib.call("gemm_nt_lse", hid, ops._ll(J), w2c, ops._ll(J), logits, ops._ll(V), M, V, J,
                      l2.bias.detach(), parts)
            with ops.timed("rnnt_align"):
                if windows is not None:
                    _lib.call("rnnt_align_packed_parts_ar", logits, labels, al_d, ll_d, windows[0], windows[1], off_d,
                              B, T, U1, V, int(self.blank), frames, scores, ws, parts, slots)
                else:
                    _lib.call("rnnt_align_packed_parts", logits, labels, al_d, ll_d, off_d, B, T, U1, V,
                              int(self.blank), frames, scores, ws, parts, slots)
        else:
            logits = ops.gemm(hid, w2c, bias=l2.bias.detach())
            with ops.timed("rnnt_align"):
                if windows is not None:
                    _lib.call("rnnt_align_packed_ar", logits, _lib.dtype_code(cd), labels, al_d, ll_d, windows[0],
                              windows[1], off_d, B, T, U1, V, int(self.blank), frames, scores, ws)
                else:
                    _lib.call("rnnt_align_packed", logits, _lib.dtype_code(cd), labels, al_d, ll_d, off_d, B, T, U1, V,
                              int(self.blank), frames, scores, ws)
        return frames, scores

    @torch.no_grad()
    def greedy_decode(self, xs, xlen):
        """Batched one-symbol-per-frame greedy search (rnnt/models.py:243-269): returns
        (list of int64 numpy arrays INCLUDING blanks, truncated to the un-scaled xlen,
        -sum_t max log p as a [B] tensor)."""
        from .decode import greedy_decode_batch
        return greedy_decode_batch(self, xs, xlen)

    def beam_search(self, xs, xlen=None, W=10, prefix=False, max_expansions=None, *, lm=None, lm_weight=None,
                    length_bonus=0.0, lm_bos=1, bias=None, skip_blank=None, ilm_weight=None):
        """Beam search of the reference's legacy model (models.py:121-202), batched; see
        ``decode.beam_search_batch``.  ``prefix=True`` is its prefix-sum variant (:145-161).  ``lm`` (an
        ``edgedict_amd.lm.LMModel``) with ``lm_weight`` adds LM shallow fusion, ``bias`` (an
        ``edgedict_amd.bias.ContextGraph``) contextual biasing towards a phrase list (``decode`` module docstring).
        ``skip_blank`` (a threshold in (0, 1]; needs the CTC head, not with ``prefix=True``) searches only the frames
        whose CTC blank posterior is at most the threshold (``decode.skip_blank_frames``).  ``ilm_weight`` raises
        ``ValueError``: internal-LM estimation is the frame-synchronous search's (``sync_beam_search``)."""
        from .decode import _no_ilm, beam_search_batch
        _no_ilm(ilm_weight, "beam_search")
        return beam_search_batch(self, xs, xlen, W, max_expansions, prefix=prefix, lm=lm, lm_weight=lm_weight,
                                 length_bonus=length_bonus, lm_bos=lm_bos, bias=bias, skip_blank=skip_blank)

    def beam_search_nbest(self, xs, xlen=None, W=10, max_expansions=None, *, lm=None, lm_weight=None, length_bonus=0.0,
                          lm_bos=1, bias=None, skip_blank=None, ctc_rescore=None, ilm_weight=None):
        """``beam_search`` (``prefix=False``) returning per utterance a ``decode.NBestResult``: the whole list B of the
        last frame in B's order, every hypothesis with its tokens, the encoder frame each token was emitted on, each
        token's score increment, and its log p; entry 0 is what ``beam_search`` returns.  ``skip_blank``: as in
        ``beam_search``, the frames reported in the original numbering.  ``ctc_rescore`` (a weight ``>= 0``; needs the
        CTC head): the list is rescored by the head - ``ctc_logp`` filled, ``logp = logp + weight * ctc_logp``, sorted
        by it (``decode.ctc_rescore``).  ``ilm_weight`` raises, as in ``beam_search``.  See
        ``decode.beam_search_nbest``."""
        from .decode import _no_ilm, beam_search_nbest
        _no_ilm(ilm_weight, "beam_search_nbest")
        return beam_search_nbest(self, xs, xlen, W, max_expansions, lm=lm, lm_weight=lm_weight,
                                 length_bonus=length_bonus, lm_bos=lm_bos, bias=bias, skip_blank=skip_blank,
                                 ctc_rescore=ctc_rescore)

    @torch.no_grad()
    def sync_beam_search(self, xs, xlen=None, W=10, *, lm=None, lm_weight=None, length_bonus=0.0, lm_bos=1, bias=None,
                         skip_blank=None, ilm_weight=None):
        """Frame-synchronous beam search (one symbol per frame at most, all B x W hypotheses in one step per frame,
        equal sequences merged by log-add; ``1 <= W <= 32``): a different algorithm from ``beam_search``, several times
        fewer launches.  ``lm`` / ``lm_weight`` / ``length_bonus`` / ``lm_bos`` / ``bias``: LM shallow fusion and
        contextual biasing, as ``beam_search`` takes them; ``skip_blank``: blank-frame skipping, as there.  Here ``lm``
        may also be an ``edgedict_amd.ngram.NGramLM`` (a back-off n-gram read inside the top-W kernel: no LM step per
        frame, ``lm_bos`` not read).  ``ilm_weight`` (a finite number ``>= 0``): internal-LM estimation - the model's own prior over the non-blank
        symbols (``ilm_score``) is subtracted with this weight.  Returns ``(seqs, scores)`` in ``beam_search``'s types.
        See ``decode.sync_beam_search_fusion``."""
        from .decode import sync_beam_search_fusion
        return sync_beam_search_fusion(self, xs, xlen, W, lm=lm, lm_weight=lm_weight, length_bonus=length_bonus,
                                       lm_bos=lm_bos, bias=bias, skip_blank=skip_blank, ilm_weight=ilm_weight)

    @torch.no_grad()
    def sync_beam_search_nbest(self, xs, xlen=None, W=10, *, lm=None, lm_weight=None, length_bonus=0.0, lm_bos=1,
                               bias=None, skip_blank=None, ctc_rescore=None, ilm_weight=None):
        """``sync_beam_search`` returning per utterance the final beam as a ranked ``decode.NBestResult``; entry 0 is
        what ``sync_beam_search`` returns.  ``ctc_rescore`` (a weight ``>= 0``; needs the CTC head): the list is
        rescored by the head and ranked by ``logp + weight * ctc_logp`` (``decode.ctc_rescore``).  ``ilm_weight``: as in
        ``sync_beam_search``.  See ``decode.sync_beam_search_nbest``."""
        from .decode import sync_beam_search_nbest
        return sync_beam_search_nbest(self, xs, xlen, W, lm=lm, lm_weight=lm_weight, length_bonus=length_bonus,
                                      lm_bos=lm_bos, bias=bias, skip_blank=skip_blank, ctc_rescore=ctc_rescore,
                                      ilm_weight=ilm_weight)

    @torch.no_grad()
    def ilm_logprobs(self, ys, ylen):
        """The internal LM's per-token log-probabilities of label sequences: fp32 [B, U] on the device,
        ``out[b, u] = log P_ILM(ys[b, u] | ys[b, :u])`` for ``u < ylen[b]`` and exactly 0 behind it.  The prediction
        network is teacher-forced from BOS; the internal LM of a position is the joint on an all-zero encoder row,
        normalised over the NON-BLANK symbols (what ``sync_beam_search(ilm_weight=)`` subtracts).  A blank label gives
        ``-inf``, one outside the vocabulary NaN.  Nothing is read back to the host."""
        from .decode import ilm_logprobs
        return ilm_logprobs(self, ys, ylen)

    @torch.no_grad()
    def ilm_score(self, ys, ylen):
        """Per utterance ``sum_u log P_ILM(y_u | y_<u)``: fp32 [B] on the device, no host sync.  The internal LM's
        perplexity of a text is ``exp(-ilm_score.sum() / ylen.sum())``: the number to choose ``ilm_weight`` by."""
        return self.ilm_logprobs(ys, ylen).sum(dim=1)

    @torch.no_grad()
    def confidence(self, xs, xlen, results, head="rnnt", **kw):
        """Token, word and utterance confidences of N-best lists (one ``decode.NBestResult`` per utterance, from any
        search on this input, or read from disk): the encoder as the N-best searches run it, then
        ``decode.hypothesis_confidence`` (``head="rnnt"``: the joint re-evaluated at every token's frame and prefix) or
        ``decode.ctc_hypothesis_confidence`` (``head="ctc"``: the CTC head's logits on every token's frame, for
        ``ctc_beam_search`` lists; RuntimeError on a model built without ``ctc_weight > 0``).  Keywords ``method``
        (``"tsallis"``, ``"entropy"``, ``"max_prob"``, ``"prob"``), ``alpha``, ``aggregate``, ``words`` as there.
        Returns one ``decode.Confidence`` per utterance.  It is the acoustic model's distribution: LM and bias terms of
        the search that made the lists take no part.  Run it in ``eval()`` mode, or dropout takes part."""
        from . import _lib, decode
        if head not in ("rnnt", "ctc"):
            raise ValueError("confidence: head must be 'rnnt' or 'ctc', got %r" % (head,))
        if head == "ctc":
            enc_out, lens = self._ctc_encode(xs, xlen)
            return decode.ctc_hypothesis_confidence(self, enc_out, lens, results, **kw)
        _lib.require_cuda(xs)
        enc_out, _ = self.encoder(xs)
        enc_out = enc_out.contiguous()
        lens = None
        if xlen is not None:
            xl = xlen.detach().cpu() if torch.is_tensor(xlen) else torch.as_tensor(xlen)
            lens = self.scale_length(enc_out, xl).numpy().astype("int32")
        return decode.hypothesis_confidence(self, enc_out, lens, results, **kw)

    EVALUATE_SEARCHES = ("greedy", "ctc_greedy", "beam", "sync_beam")
    last_error_rate = None       # the metrics.ErrorRateResult of the last evaluate_step

    @torch.no_grad()
    def evaluate_step(self, xs, ys, xlen, ylen, *, search="greedy", tokenizer=None, **search_kwargs):
        """One validation batch, as the reference's ``evaluate_step`` runs it behind its front-end (cli/train.py:
        294-319): the loss (``forward``), a decode, and the batch's error rate - under ``torch.no_grad()`` in the
        model's CURRENT mode (call ``eval()`` first, or dropout takes part; ``TrainEngine.evaluate_step`` does).
        ``search``: ``"greedy"`` (``greedy_decode``, the reference's choice, blanks removed), ``"ctc_greedy"``
        (``ctc_greedy_decode``), ``"beam"`` (``beam_search``) or ``"sync_beam"`` (``sync_beam_search``, its top
        hypothesis); ``search_kwargs`` go to the two beam searches (``W=``, ``lm=``, ``skip_blank=``, ...).  ``ys`` is cut
        at ``ylen`` row by row.  Returns the reference's tuple ``(loss_float, rate, pred, true)``: without a tokenizer
        ``rate`` is the batch's token error rate and ``pred`` / ``true`` are lists of int64 token arrays; with a
        tokenizer (anything with the reference's ``decode_plus``) ``rate`` is the batch's word error rate
        (``metrics.word_error_rate``: summed errors over summed reference words) and ``pred`` / ``true`` are the
        strings ``decode_plus`` returns.  The full ``metrics.ErrorRateResult`` of the call stays in
        ``self.last_error_rate``.  Needs ``output_loss=True``."""
        import numpy as np
        from . import metrics
        if search not in self.EVALUATE_SEARCHES:
            raise ValueError("search must be one of %s, got %r" % (", ".join(self.EVALUATE_SEARCHES), search))
        if search_kwargs and search in ("greedy", "ctc_greedy"):
            raise ValueError("search=%r takes no search arguments (got %s)" % (search, ", ".join(sorted(search_kwargs))))
        if not self.output_loss:
            raise ValueError("evaluate_step needs output_loss=True")
        loss = float(self.forward(xs, ys, xlen, ylen))
        if search == "greedy":
            seqs, _ = self.greedy_decode(xs, xlen)
            pred = [s[s != self.blank] for s in seqs]
        elif search == "ctc_greedy":
            pred, _ = self.ctc_greedy_decode(xs, xlen)
        elif search == "beam":
            pred, _ = self.beam_search(xs, xlen, **search_kwargs)
        else:
            pred, _ = self.sync_beam_search(xs, xlen, **search_kwargs)
        pred = [np.asarray(s, dtype=np.int64) for s in pred]
        ys_h, ylen_h = ys.detach().cpu().numpy(), ylen.detach().cpu().numpy()
        true = [ys_h[b, :int(ylen_h[b])].astype(np.int64) for b in range(ys_h.shape[0])]
        if tokenizer is None:
            record = metrics.token_error_rate(pred, true, xs.device)
        else:
            pred, true = tokenizer.decode_plus(pred), tokenizer.decode_plus(true)
            record = metrics.word_error_rate(pred, true, xs.device)
        self.last_error_rate = record
        return loss, record.rate, pred, true

    MWER_SEARCHES = ("sync_beam", "beam")
    last_mwer = None             # what the last mwer_loss call worked on (see there)

    def mwer_loss(self, xs, ys, xlen, ylen, *, W=4, search="sync_beam", nbest=None, nll_weight=0.0, **search_kwargs):
        """Minimum word error rate loss of a batch (Prabhavalkar et al. 2018; Guo et al. 2020): the expected number of
        token errors of every utterance's N-best list under the list's renormalised posterior, ``mean_b risk_b +
        nll_weight * mean_b nll_ref_b`` as a ``(1,)`` tensor, differentiable in every parameter (``loss.MWERLoss``).

        The encoder runs once, with gradient, in the model's current mode.  The lists: ``nbest`` (one entry per
        utterance: a ``decode.NBestResult`` or a list of token arrays), else a search on the detached encoder output
        under ``torch.no_grad()`` - ``search="sync_beam"``: ``decode.sync_beam_search_nbest_enc``, ``"beam"``:
        ``decode.beam_search_nbest_enc`` with ``.ranked(merge=True)`` - of width ``W``; ``search_kwargs`` (``lm=``,
        ``bias=``, ...) go to the search.  Equal sequences count once, an empty list is the empty hypothesis, more than
        32 distinct sequences per utterance raise.  Every hypothesis (and, with ``nll_weight > 0``, every reference) is a
        row of ONE packed joint + loss call whose per-row costs are the hypotheses' negative log-likelihoods; the
        encoder rows are gathered with ``index_select`` (torch adds the gradients back), the errors come from
        ``metrics.edit_distance`` on the same upload.

        No CTC term, and ``fastemit_lambda`` is NOT applied: the hypotheses' costs are plain negative log-likelihoods.
        Needs a device model and host-side ``xlen`` / ``ylen`` (they size the lattice), else ``ValueError``.  Apart from
        the search's own read nothing waits for the device as long as ``ys`` is a host tensor (a device ``ys`` is read
        back once, behind the search).  Leaves ``self.last_mwer``: ``lists`` (the distinct sequences used), and the
        device tensors ``errors`` ``[B, N, 4]``, ``costs`` ``[B, N]`` (+inf on empty slots), ``posterior`` ``[B, N]``,
        ``risk`` ``[B]`` and ``n_hyp`` ``[B]``."""
        import numpy as np
        from . import decode, metrics
        from ._staging import to_device
        from .loss import MWERLoss, check_nll_weight, mwer_rows
        if search not in self.MWER_SEARCHES:
            raise ValueError("search must be one of %s, got %r" % (", ".join(self.MWER_SEARCHES), search))
        nll_weight = check_nll_weight(nll_weight)
        if not (torch.is_tensor(xs) and xs.is_cuda and xs.dim() == 3):
            raise ValueError("mwer_loss needs a device batch xs [B, T, F]")
        if xlen.is_cuda or ylen.is_cuda:
            raise ValueError("mwer_loss needs xlen and ylen on the host: they size the packed lattice")
        B = xs.shape[0]
        if nbest is not None and len(nbest) != B:
            raise ValueError("nbest must hold one list per utterance (got %d for a batch of %d)" % (len(nbest), B))
        xs = xs[:, :xlen.max()].contiguous()
        cd = self.compute_dtype
        h_enc, _ = self.encoder(xs)
        h_enc = _to_cd(h_enc, cd)
        act = self.scale_length(h_enc, xlen)                 # host int32 [B]
        if nbest is None:
            with torch.no_grad():
                lens = act.numpy().astype(np.int32)
                if search == "sync_beam":
                    found = decode.sync_beam_search_nbest_enc(self, h_enc.detach(), lens, W, **search_kwargs)
                else:
                    found = [r.ranked(merge=True)
                             for r in decode.beam_search_nbest_enc(self, h_enc.detach(), lens, W, **search_kwargs)]
            lists = [r.tokens for r in found]
        else:
            lists = [r.tokens if isinstance(r, decode.NBestResult) else list(r) for r in nbest]
        rows = mwer_rows(lists, ys, ylen, nll_weight > 0)
        dev = h_enc.device
        v = rows.views(to_device(torch.from_numpy(rows.host), dev))
        host = rows.views()
        l1, l2 = self.joint.joint[0], self.joint.joint[2]
        ops.mark("joint:enter")
        enc_rows = h_enc.index_select(0, v["row_utt"])
        h_dec, _ = self.decoder(v["labels"])
        act_rows = act[torch.from_numpy(host["row_utt"].astype(np.int64))]
        row_costs = _JointLossFn.apply(enc_rows, _to_cd(h_dec, cd), l1.weight, l1.bias, l2.weight, l2.bias, v["labels"],
                                       act_rows, torch.from_numpy(host["label_lens"]), self.blank, cd, 0.0, None, None,
                                       None, True)
        ops.mark("joint:exit")
        errors = metrics.edit_distance(v["hyps"], v["hyp_lens"], v["refs"], v["ref_lens"], v["n_hyp"])
        N, Rh = rows.N, rows.Rh
        dense = torch.full((B * N,), float("inf"), dtype=F32, device=dev)
        dense = dense.index_copy(0, v["row_dense"][:Rh].long(), row_costs[:Rh]).view(B, N)
        crit = MWERLoss(nll_weight)
        loss = crit(dense, errors, v["n_hyp"], row_costs[Rh:] if nll_weight > 0 else None)
        self.last_mwer = dict(lists=rows.lists, errors=errors, costs=dense.detach(), posterior=crit.last_posterior,
                              risk=crit.last_risk, n_hyp=v["n_hyp"])
        return loss


class _CausalConvFn(torch.autograd.Function):
    """Conv1d(C_in, C_out, k, stride s, padding k-1) followed by dropping the last k-1 frames
    (CausalConv1d / DilatedConvBlock of rnnt/models.py:314-339), channels-last: im2col gather +
    one MFMA GEMM; backward = dW GEMM, bias column sum, dcols GEMM + col2im gather."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, cd):
        B, Tin, C = x.shape
        Cout, Cin, k = weight.shape
        assert Cin == C
        cols = ops.conv_im2col(x.contiguous(), k, stride, cd)
        Tout = cols.shape[1]
        w2 = WEIGHTS.get(weight, cd).view(Cout, Cin * k)
        y = ops.gemm(cols.view(B * Tout, C * k), w2, bias=None if bias is None else bias.detach())
        ctx.save_for_backward(cols, weight)
        ctx.cfg = (B, Tin, C, k, stride, cd, bias is not None, x.dtype)
        return y.view(B, Tout, Cout)

    @staticmethod
    def backward(ctx, dy):
        cols, weight = ctx.saved_tensors
        B, Tin, C, k, stride, cd, has_bias, in_dtype = ctx.cfg
        Cout = weight.shape[0]
        Tout = cols.shape[1]
        M = B * Tout
        dy2 = dy.contiguous().view(M, Cout)
        if dy2.dtype != cd:
            dy2 = ops.cast(dy2, cd)
        dw = ops.gemm(dy2.t(), cols.view(M, C * k).t(), out_dtype=F32,
                      split_k=ops.pick_split_k(Cout, C * k, M)).view(Cout, C, k)
        db = ops.colsum(dy2) if has_bias else None
        dx = None
        if ctx.needs_input_grad[0]:
            w2 = WEIGHTS.get(weight, cd).view(Cout, C * k)
            dcols = ops.gemm(dy2, w2.t()).view(B, Tout, C * k)
            dx = ops.conv_col2im(dcols, Tin, C, k, stride)
            if dx.dtype != in_dtype:
                dx = ops.cast(dx, in_dtype)
        return dx, dw, db, None, None


class _GeluGroupNormFn(torch.autograd.Function):
    """GroupNorm(1, C)(GELU(y)) on channels-last [B,T,C] (DilatedConvBlock.forward,
    rnnt/models.py:333-335): statistics over all (t, c) of a sample, affine per channel."""

    @staticmethod
    def forward(ctx, y, gamma, beta):
        out, mean, rstd = ops.gelu_groupnorm_fwd(y.contiguous(), gamma.detach(), beta.detach())
        ctx.save_for_backward(y, gamma, mean, rstd)
        return out

    @staticmethod
    def backward(ctx, dout):
        y, gamma, mean, rstd = ctx.saved_tensors
        if dout.dtype != y.dtype:
            dout = ops.cast(dout.contiguous(), y.dtype)
        dy, dgamma, dbeta = ops.gelu_groupnorm_bwd(y, dout, gamma.detach(), mean, rstd)
        return dy, dgamma, dbeta


class _ConvParams(nn.Module):
    """nn.Conv1d-compatible parameters: weight [C_out, C_in, k] (kaiming-normal as the reference
    re-initialises it, rnnt/models.py:317,329), bias [C_out] (nn.Conv1d default init)."""

    def __init__(self, in_channels, out_channels, kernel_size, stride, bias=True):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride = (kernel_size,), (stride,)
        self.padding = (kernel_size - 1,)
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, kernel_size))
        nn.init.kaiming_normal_(self.weight)
        if bias:
            bound = 1.0 / math.sqrt(in_channels * kernel_size)
            self.bias = nn.Parameter(torch.empty(out_channels).uniform_(-bound, bound))
        else:
            self.register_parameter("bias", None)


class DilatedConvBlock(nn.Module):
    """GELU -> GroupNorm(group_norm_size=1, C_in) -> causal strided Conv1d (rnnt/models.py:323-339);
    channels-last in and out.  Only dilation 1 and one group (what FrontEnd builds)."""

    def __init__(self, in_channels, out_channels, kernel_size, dilation=1, group_norm_size=1,
                 stride=1, bias=True):
        super().__init__()
        if dilation != 1 or group_norm_size != 1:
            raise NotImplementedError("DilatedConvBlock: only dilation=1, group_norm_size=1 (FrontEnd's use)")
        self.conv = _ConvParams(in_channels, out_channels, kernel_size, stride, bias)
        self.gn = _LayerNormParams(in_channels)      # weight / bias [C_in], the GroupNorm affine

    def forward(self, x, cd):
        x = _GeluGroupNormFn.apply(x, self.gn.weight, self.gn.bias)
        return _CausalConvFn.apply(x, self.conv.weight, self.conv.bias, self.conv.stride[0], cd)


class FrontEnd(nn.Module):
    """Convolutional waveform feature extractor of the reference's cli/train.py
    (rnnt/models.py:341-365): f32 [B, N] (or [B,1,N]) -> [B, T, C_last], LayerNorm over channels.
    State-dict keys as the reference: conv1.{weight,bias}, encode.{i}.conv.{weight,bias},
    encode.{i}.gn.{weight,bias}, layer_norm.{weight,bias}."""

    def __init__(self, frontend_params=[(10, 5, 16)] + [(8, 4, 32)] + [(4, 2, 128)] * 3, bias=True):
        super().__init__()
        ks = [p[0] for p in frontend_params]
        st = [p[1] for p in frontend_params]
        ch = [p[2] for p in frontend_params]
        self.conv1 = _ConvParams(1, ch[0], ks[0], st[0], bias)
        self.encode = nn.Sequential(*[
            DilatedConvBlock(ch[i - 1], ch[i], ks[i], dilation=1, stride=st[i], group_norm_size=1, bias=bias)
            for i in range(1, len(st))])
        self.layer_norm = _LayerNormParams(ch[-1])

    def out_frames(self, n_samples):
        t = ops.conv_out_frames(n_samples, self.conv1.kernel_size[0], self.conv1.stride[0])
        for blk in self.encode:
            t = ops.conv_out_frames(t, blk.conv.kernel_size[0], blk.conv.stride[0])
        return t

    def forward(self, x):
        require_cuda(x)
        cd = getattr(self, "compute_dtype", None) or config.get_compute_dtype()
        if not isinstance(cd, torch.dtype):
            cd = config._parse(cd)
        if x.dim() == 3:                      # B x 1 x T -> B x T (rnnt/models.py:352-353 the other way)
            x = x[:, 0]
        x = x.float().contiguous().unsqueeze(-1)          # channels-last [B, N, 1]
        x = _CausalConvFn.apply(x, self.conv1.weight, self.conv1.bias, self.conv1.stride[0], cd)
        for blk in self.encode:
            x = blk(x, cd)
        return _InputNormFn.apply(x, self.layer_norm.weight, self.layer_norm.bias, cd)


class _OutsideHotPath(nn.Module):
    """Names the reference's scripts import next to ``Transducer`` (cli/train.py:18,
    rnnt/wav2vec.py:12) but whose arithmetic is not on the MI355X hot path (SURVEY.md 8f rank 4,
    DESIGN.md section 8).  They stay importable so that those scripts load; constructing one fails
    loudly - there is no eager-PyTorch fallback in this engine."""

    _what = ""

    def __init__(self, *args, **kwargs):
        super().__init__()
        raise NotImplementedError(
            "%s is not implemented by the MI355X engine (%s); use the log-mel front-end and the LSTM "
            "encoder (cli/baseline.py path)" % (type(self).__name__, self._what))


class CTCEncoder(_OutsideHotPath):
    _what = "the CTC encoder of rnnt/models.py:272-311"


def convert_lightning2normal(checkpoint):
    """Lightning checkpoint -> ``{'model': state_dict}`` (same contract as the reference's
    rnnt/models.py:366-380): when the file has a ``state_dict`` whose keys carry the Lightning
    ``model.`` prefix, the prefix is removed everywhere and the result is wrapped under
    ``'model'``; a ``state_dict`` without the prefix is returned bare; anything else is
    passed through untouched."""
    if 'state_dict' not in checkpoint:
        return checkpoint
    inner = checkpoint['state_dict']
    names = list(inner.keys())
    if names and 'model.' in names[0]:
        return {'model': {name.replace('model.', ''): t for name, t in inner.items()}}
    return inner
