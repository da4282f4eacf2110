"""External LSTM language model: shallow fusion in the beam searches, and its training.

``LMModel`` is the reference's ``LMModel`` (models.py:224-261: ``nn.Embedding`` -> ``nn.LSTM`` stack -> ``nn.Linear``
-> ``log_softmax``), the model ``cli/train_lm.py`` trains on the transducer's BPE vocabulary (``LMModel(1024, 64, 1024,
2)``) and saves as a ``state_dict``.  The parameter names are the reference's (``encoder.weight``,
``rnn.weight_ih_l{k}`` ..., ``decoder.weight`` / ``decoder.bias``), so that checkpoint loads with ``strict=True`` - and
one written here (``LMTrainer.save``) loads into the reference's model.

Everything runs on the engine's kernels (embedding gather, one LSTM block per layer, the dense product, then a row
log-softmax or the fused loss); parameters must be on the device, there is no CPU path.

* ``forward`` is the reference's: fp32 log-probs ``[B * T, ntoken]``.  It is differentiable (the row log-softmax has a
  backward kernel), so the reference's loop - ``forward`` + ``torch.nn.NLLLoss(ignore_index=0)`` - trains as written.
* ``loss`` is the same network ending in the fused softmax-NLL (``loss.SoftmaxNLLLoss``, csrc/lm_loss.hip): the loss
  kernel reads the logits, the gradient kernel overwrites them; no fp32 ``[B * T, ntoken]`` tensor exists.
* ``score`` gives sentence log-probabilities (the forward-only mode of the loss kernel), what N-best rescoring needs.
* ``LMTrainer`` is the reference script's step (Adam, ``clip_grad_norm_(…, 1.0)``) on ``optim.FusedAdam``.

The beam searches (``decode.beam_search_batch(..., lm=...)``, ``decode.StreamingBeamSearch(..., lm=...)``) do not call
``forward``: they step the LM inside the native search loop (csrc/decode.hip) from the same parameters.
"""
import ctypes
import math

import torch
import torch.nn as nn

from . import _lib, config, ops, side
from ._lib import require_cuda
from .loss import SoftmaxNLLLoss, softmax_nll_rows
from .models import WEIGHTS, _LinearFn, _LinearParams, _LSTMBlockFn, _LSTMParams, _dropout, _state
from .optim import FlatParams, FusedAdam

NO_PAD = -1    # ops.embedding_bwd's `pad`: a value no token has (the reference LM's nn.Embedding has no padding_idx)


class _LMEmbeddingFn(torch.autograd.Function):
    """nn.Embedding WITHOUT padding_idx (models.py:230): token 0's row receives its gradient like any other.

    ``tied``: the weight is the decoder's too (``tie_weights=True``).  The decoder's product may have accumulated its
    share into the same ``.grad`` buffer on the auxiliary stream (side.WeightGrads); autograd adds this function's share
    on the current stream, so that stream first waits for the auxiliary one - two read-modify-writes of one buffer must
    not overlap.  This is the last node of the backward pass: nothing is left to hide the wait behind."""

    @staticmethod
    def forward(ctx, tokens, weight, cd, tied):
        out = ops.embedding_fwd(tokens, weight.detach(), cd, False, 0)
        ctx.save_for_backward(tokens)
        ctx.cfg = (weight.shape[0], tied)
        return out

    @staticmethod
    def backward(ctx, dout):
        (tokens,) = ctx.saved_tensors
        V, tied = ctx.cfg
        demb = ops.embedding_bwd(tokens, dout, V, False, 0, NO_PAD)
        if tied:
            aux = side.peek(dout.device)
            if aux is not None:
                torch.cuda.current_stream(dout.device).wait_stream(aux)
        return None, demb, None, None


class LMModel(nn.Module):
    """The reference's LSTM language model (models.py:224-261) with its constructor and parameter names."""

    def __init__(self, ntoken, ninp, nhid, nlayers, dropout=0.5, tie_weights=False):
        super().__init__()
        self.ntoken = ntoken
        self.dropout = dropout
        self.encoder = nn.Embedding(ntoken, ninp)      # container: the lookup runs on the engine's kernel
        self.rnn = _LSTMParams(ninp, nhid, nlayers, dropout)
        self.decoder = _LinearParams(nhid, ntoken)
        if tie_weights:
            if nhid != ninp:
                raise ValueError("When using the tied flag, nhid must be equal to emsize")
            self.decoder.weight = self.encoder.weight
        self.init_weights()
        self.nhid = nhid
        self.rnn_type = "LSTM"
        self.nlayers = nlayers

    def init_weights(self):
        initrange = 0.1
        nn.init.uniform_(self.encoder.weight, -initrange, initrange)
        nn.init.uniform_(self.decoder.weight, -initrange, initrange)

    @property
    def compute_dtype(self):
        return getattr(self, "_compute_dtype", None) or config.get_compute_dtype()

    @compute_dtype.setter
    def compute_dtype(self, value):
        self._compute_dtype = config._parse(value)

    def init_hidden(self, bsz):
        """Zero (h, c), each [nlayers, bsz, nhid] (models.py:255-261)."""
        weight = next(self.parameters())
        return (weight.new_zeros(self.nlayers, bsz, self.nhid), weight.new_zeros(self.nlayers, bsz, self.nhid))

    def _logits(self, input, hidden):
        """input int [B, T] -> (raw logits [B * T, ntoken] in the compute dtype, (h, c) fp32 [nlayers, B, nhid])."""
        require_cuda(self.encoder.weight)
        cd = self.compute_dtype
        tokens = input.to(device=self.encoder.weight.device, dtype=torch.int32)
        if tokens.dim() != 2:
            raise ValueError("LMModel expects token ids of shape [B, T]")
        tokens = tokens.contiguous()
        B, T = tokens.shape
        x = _LMEmbeddingFn.apply(tokens, self.encoder.weight, cd, self.decoder.weight is self.encoder.weight)
        if self.dropout > 0 and self.training:
            x = _dropout(x, self.dropout)
        hs, cs = [], []
        for k in range(self.nlayers):
            w_ih, w_hh, b_ih, b_hh = self.rnn.layer(k)
            h0 = c0 = None
            if hidden is not None:
                h0, c0 = _state(hidden[0][k]), _state(hidden[1][k])
            x, h, c = _LSTMBlockFn.apply(x, w_ih, w_hh, b_ih, b_hh, None, None, h0, c0, False, 1, cd)
            if self.dropout > 0 and self.training:
                x = _dropout(x, self.dropout)      # nn.LSTM(dropout) between layers, then self.drop on the output
            hs.append(h)
            cs.append(c)
        decoded = _LinearFn.apply(x, self.decoder.weight, self.decoder.bias, cd).reshape(B * T, self.ntoken)
        return decoded, (torch.stack(hs, 0), torch.stack(cs, 0))

    def forward(self, input, hidden):
        """input int [B, T] token ids, hidden (h, c) [nlayers, B, nhid] -> (log-probs fp32 [B * T, ntoken], (h, c)).

        Differentiable with respect to the parameters (they must be on the device: there is no CPU path, and asking
        for a gradient with parameters on the CPU raises ``NotImplementedError``); ``(h, c)`` carry no gradient."""
        if (torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
                and not self.encoder.weight.is_cuda):
            raise NotImplementedError("LMModel.forward has no CPU path: move the model to the device to train it, or "
                                      "run it under torch.no_grad()")
        decoded, state = self._logits(input, hidden)
        if torch.is_grad_enabled() and decoded.requires_grad:
            return _LogSoftmaxRowsFn.apply(decoded), state
        return log_softmax_rows(decoded), state

    def loss(self, input, targets, hidden=None, ignore_index=0, reduction="mean"):
        """The training loss of cli/train_lm.py:87-89 - ``NLLLoss(ignore_index)(forward(input)[0], targets.flatten())``
        - with the log-softmax and the loss fused (``loss.SoftmaxNLLLoss``): returns ``(loss, (h, c))``, ``(h, c)``
        detached (the reference's ``repackage_hidden``); ``hidden=None`` starts from zeros.  ``targets`` int ``[B, T]``;
        ``'none'`` returns ``[B, T]``."""
        decoded, state = self._logits(input, hidden)
        targets = targets.to(device=decoded.device)
        if tuple(targets.shape) != tuple(input.shape):
            raise ValueError("targets %s must have input's shape %s" % (tuple(targets.shape), tuple(input.shape)))
        out = SoftmaxNLLLoss(ignore_index=ignore_index, reduction=reduction)(decoded, targets.reshape(-1))
        return (out.view(targets.shape) if reduction == "none" else out), state

    @torch.no_grad()
    def score(self, tokens, lengths, bos=1, check_tokens=False):
        """Sentence log-probabilities, fp32 ``[B]``: ``sum_{u < lengths[b]} log P(tokens[b, u] | bos, tokens[b, :u])``.
        ``tokens`` int ``[B, U]`` (anything behind ``lengths[b]`` is ignored), ``lengths`` int ``[B]``.  The input is the
        BOS-shifted token matrix, as ``seq_collate`` builds it; the loss kernel runs forward-only (per-row NLL, no
        reduction, no gradient buffer).  Call it in ``eval()`` mode: in training mode dropout applies, as in ``forward``.

        A token outside ``[0, ntoken)`` INSIDE a sentence is not reported by default: as a target it is an ignored row
        (it adds an exact 0, which RAISES the sentence's score), as an input the embedding clamps it.
        ``check_tokens=True`` reads the tokens once on the host and raises ``ValueError`` for one."""
        dev = self.encoder.weight.device
        require_cuda(self.encoder.weight)
        tokens = tokens.to(device=dev, dtype=torch.int32)
        if tokens.dim() != 2:
            raise ValueError("score expects token ids of shape [B, U]")
        B, U = tokens.shape
        lengths = torch.as_tensor(lengths).to(device=dev, dtype=torch.int32)
        if lengths.shape != (B,):
            raise ValueError("score expects one length per sentence")
        if not 0 <= int(bos) < self.ntoken:
            raise ValueError("bos = %d outside the vocabulary" % bos)
        if U == 0:
            return torch.zeros(B, dtype=torch.float32, device=dev)
        keep = torch.arange(U, device=dev, dtype=torch.int32)[None, :] < lengths[:, None]
        if check_tokens and bool((keep & ((tokens < 0) | (tokens >= self.ntoken))).any()):
            raise ValueError("score: a token inside a sentence lies outside [0, %d)" % self.ntoken)
        inputs = torch.cat([torch.full((B, 1), int(bos), dtype=torch.int32, device=dev), tokens[:, :-1]], 1)
        # a position behind the sentence's end gets a target no vocabulary has: the kernel writes an exact 0 there
        targets = torch.where(keep, tokens, torch.full_like(tokens, -1)).reshape(-1).contiguous()
        decoded, _ = self._logits(inputs, None)
        return -softmax_nll_rows(decoded, targets, ignore_index=-1).view(B, U).sum(1)


class _LogSoftmaxRowsFn(torch.autograd.Function):
    """``log_softmax_rows`` with its backward kernel: dx = dy - exp(y) * rowsum(dy), in the logits' dtype."""

    @staticmethod
    def forward(ctx, x):
        y = log_softmax_rows(x)
        ctx.save_for_backward(y)
        ctx.x_dtype = x.dtype
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        M, N = y.shape
        if dy.dtype != torch.float32 or dy.stride(1) != 1 or (M > 1 and dy.stride(0) < N):
            dy = dy.float().contiguous()
        dx = torch.empty(M, N, dtype=ctx.x_dtype, device=y.device)
        _lib.call("log_softmax_rows_bwd", y, dy, ops._ll(dy.stride(0)) if M > 1 else ops._ll(N),
                  _lib.dtype_code(ctx.x_dtype), dx, M, N)
        return dx


def log_softmax_rows(x):
    """fp32 log_softmax over the last dimension of a 2-D fp32 / bf16 tensor (csrc/elementwise.hip)."""
    require_cuda(x)
    if x.dim() != 2 or x.stride(1) != 1:
        x = x.reshape(-1, x.shape[-1]).contiguous()
    M, N = x.shape
    y = torch.empty(M, N, dtype=torch.float32, device=x.device)
    _lib.call("log_softmax_rows", _lib.dtype_code(x.dtype), x, ops._ll(x.stride(0)) if M > 0 else ops._ll(N), y, M, N)
    return y


class BeamLM(ctypes.Structure):
    """ctypes mirror of ``edgedict_beam_lm_t`` (include/edgedict_hip.h)."""
    _fields_ = [("L", ctypes.c_int), ("E", ctypes.c_int), ("H", ctypes.c_int), ("V", ctypes.c_int),
                ("emb", ctypes.c_void_p), ("emb_dtype", ctypes.c_int),
                ("w_ih", ctypes.c_void_p), ("w_hh", ctypes.c_void_p), ("b_ih", ctypes.c_void_p),
                ("b_hh", ctypes.c_void_p), ("Wo", ctypes.c_void_p), ("bo", ctypes.c_void_p),
                ("bos", ctypes.c_int), ("weight", ctypes.c_double), ("length_bonus", ctypes.c_double)]


def check_fusion_args(lm, lm_weight, V=None, prefix=False):
    """The argument rules of every beam search that takes an LM (raised before anything is launched)."""
    if lm is None:
        return
    if not isinstance(lm, LMModel):
        raise ValueError("lm must be an edgedict_amd.lm.LMModel (got %s)" % type(lm).__name__)
    if lm_weight is None:
        raise ValueError("an LM needs lm_weight (the shallow-fusion weight lambda)")
    if prefix:
        raise ValueError("prefix=True (the prefix-sum merge) is not supported with an LM")
    if V is not None and lm.ntoken != V:
        raise ValueError("the LM's vocabulary (ntoken = %d) differs from the transducer's (V = %d)" % (lm.ntoken, V))


class FusionLM:
    """The LM's weights in the search's compute dtype ``cd`` (converted once through ``WEIGHTS``, as the prediction
    network's are) and the ``edgedict_beam_lm_t`` the native searches take."""

    def __init__(self, lm, cd, lm_weight, length_bonus=0.0, lm_bos=1):
        from .decode import _ptr_array
        rnn = lm.rnn
        self.L, self.H = lm.nlayers, lm.nhid
        self.E = lm.encoder.weight.shape[1]
        self.V = lm.ntoken
        self.emb = lm.encoder.weight.detach()
        self.w_ih = [WEIGHTS.get(rnn.layer(k)[0], cd) for k in range(self.L)]
        self.w_hh = [WEIGHTS.get(rnn.layer(k)[1], cd) for k in range(self.L)]
        self.b_ih = [rnn.layer(k)[2].detach() for k in range(self.L)]
        self.b_hh = [rnn.layer(k)[3].detach() for k in range(self.L)]
        self.wo = WEIGHTS.get(lm.decoder.weight, cd)
        self.bo = lm.decoder.bias.detach()
        for t in [self.emb, self.wo, self.bo] + self.w_ih + self.w_hh + self.b_ih + self.b_hh:
            require_cuda(t)
        if not 0 <= int(lm_bos) < self.V:
            raise ValueError("lm_bos = %d outside the vocabulary" % lm_bos)
        # the pointer arrays must outlive every call that reads the struct
        self._arrays = (_ptr_array(self.w_ih), _ptr_array(self.w_hh), _ptr_array(self.b_ih), _ptr_array(self.b_hh))
        s = BeamLM()
        s.L, s.E, s.H, s.V = self.L, self.E, self.H, self.V
        s.emb, s.emb_dtype = self.emb.data_ptr(), _lib.dtype_code(self.emb.dtype)
        s.w_ih, s.w_hh, s.b_ih, s.b_hh = [ctypes.cast(a, ctypes.c_void_p).value for a in self._arrays]
        s.Wo, s.bo = self.wo.data_ptr(), self.bo.data_ptr()
        s.bos, s.weight, s.length_bonus = int(lm_bos), float(lm_weight), float(length_bonus)
        self.struct = s

    def ref(self):
        return ctypes.byref(self.struct)


# ------------------------------------------------------------------------------------------------ training
def seq_collate(batches, bos=1, pad=0):
    """The reference's collate (cli/train_lm.py:37-43): a list of 1-D token tensors -> ``(inputs, targets)``, both long
    ``[B, max_len]``; ``targets`` are the sentences padded with ``pad`` = 0 (the loss's ``ignore_index``), ``inputs`` the
    same matrix shifted right by one with ``bos`` = 1 in front."""
    targets = torch.nn.utils.rnn.pad_sequence([torch.as_tensor(b).long() for b in batches], batch_first=True,
                                              padding_value=pad)
    inputs = torch.cat([torch.full((targets.shape[0], 1), bos, dtype=torch.long), targets], dim=1)
    return inputs[:, :-1], targets


class LMTrainer:
    """The training step of cli/train_lm.py:79-93 on the engine: ``Adam(lr)`` with ``clip_grad_norm_(parameters,
    max_grad_norm)`` as one ``optim.FusedAdam`` over ``FlatParams`` (weight gradients accumulate in place, deferred to
    the auxiliary stream), the loss through ``LMModel.loss`` (``ignore_index`` = 0, the collate's padding).

    ``dtype``: the model's compute dtype (``'bf16'`` / ``'fp32'`` / a torch dtype; ``None`` leaves it as it is)."""

    def __init__(self, model, lr=1e-4, max_grad_norm=1.0, dtype=None):
        if not isinstance(model, LMModel):
            raise ValueError("LMTrainer trains an edgedict_amd.lm.LMModel (got %s)" % type(model).__name__)
        self.model = model
        if dtype is not None:
            model.compute_dtype = dtype
        self.optimizer = FusedAdam(FlatParams(model), lr=lr, max_grad_norm=max_grad_norm)

    def train_step(self, inputs, targets, hidden=None):
        """One step on ``(inputs, targets)`` int ``[B, T]`` (``seq_collate``'s pair); returns the mean NLL over the
        non-padding targets as a 0-dim device tensor - nothing here waits for the device."""
        self.model.train()
        self.optimizer.zero_grad()
        loss, _ = self.model.loss(inputs, targets, hidden, ignore_index=0, reduction="mean")
        loss.backward()
        self.optimizer.step()
        return loss.detach()

    @torch.no_grad()
    def evaluate(self, batches):
        """``(mean NLL per non-padding token, perplexity)`` over an iterable of ``(inputs, targets)``, in eval mode (the
        host reads sum and count once, at the end).  Token-weighted, not the reference's mean of batch means (cli/train_lm.py:95-104)."""
        was_training = self.model.training
        self.model.eval()
        total = count = None
        try:
            for inputs, targets in batches:
                nll, _ = self.model.loss(inputs, targets, None, ignore_index=0, reduction="sum")
                n = (targets != 0).sum().to(nll.device)
                total = nll.double() if total is None else total + nll.double()
                count = n if count is None else count + n
        finally:
            self.model.train(was_training)
        if total is None or int(count) == 0:
            return 0.0, 1.0
        mean = float(total) / int(count)
        return mean, math.exp(mean)

    def save(self, path):
        """Write the bare ``state_dict`` cli/train_lm.py:109 writes (CPU tensors, the reference's keys): it loads into
        the reference's ``LMModel`` and into ``LMModel.load_state_dict(strict=True)`` here with nothing converted."""
        torch.save({k: v.detach().cpu().clone() for k, v in self.model.state_dict().items()}, path)

    def load(self, path):
        self.model.load_state_dict(torch.load(path, map_location="cpu"), strict=True)
        config.bump_param_epoch()
