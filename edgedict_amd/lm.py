"""External LSTM language model for shallow fusion in the beam searches.

``LMModel`` is the reference's ``LMModel`` (models.py:224-261: ``nn.Embedding`` -> ``nn.LSTM`` stack -> ``nn.Linear``
-> ``log_softmax``), the model ``cli/train_lm.py`` trains on the transducer's BPE vocabulary (``LMModel(1024, 64, 1024,
2)``) and saves as a ``state_dict``.  The parameter names are the reference's (``encoder.weight``,
``rnn.weight_ih_l{k}`` ..., ``decoder.weight`` / ``decoder.bias``), so that checkpoint loads with ``strict=True``.

``forward`` runs on the engine's kernels (embedding gather, one LSTM block per layer, the dense product, a row
log-softmax) and is inference only: training the LM is not supported, so ``forward`` raises ``NotImplementedError``
when autograd would need a gradient.  Run it under ``torch.no_grad()`` (or with frozen parameters).  The beam searches
(``decode.beam_search_batch(..., lm=...)``, ``decode.StreamingBeamSearch(..., lm=...)``) do not call ``forward``: they
step the LM inside the native search loop (csrc/decode.hip) from the same parameters.
"""
import ctypes

import torch
import torch.nn as nn

from . import _lib, config, ops
from ._lib import require_cuda
from .models import WEIGHTS, _EmbeddingFn, _LinearFn, _LinearParams, _LSTMBlockFn, _LSTMParams, _dropout, _state


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

    def forward(self, input, hidden):
        """input int [B, T] token ids, hidden (h, c) [nlayers, B, nhid] -> (log-probs fp32 [B * T, ntoken], (h, c))."""
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise NotImplementedError("LMModel.forward is inference only (training the LM is not supported): run it "
                                      "under torch.no_grad()")
        require_cuda(self.encoder.weight)
        cd = self.compute_dtype
        tokens = input.to(device=self.encoder.weight.device, dtype=torch.int32)
        if tokens.dim() != 2:
            raise ValueError("LMModel expects token ids of shape [B, T]")
        tokens = tokens.contiguous()
        B, T = tokens.shape
        x = _EmbeddingFn.apply(tokens, self.encoder.weight, False, cd)
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
        return log_softmax_rows(decoded), (torch.stack(hs, 0), torch.stack(cs, 0))


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
