"""Greedy search over a batch, driven by csrc/decode.hip (one C call for the whole time loop).

``greedy_decode_batch`` reproduces ``Transducer.greedy_decode`` (rnnt/models.py:243-269):
encoder over the whole batch, prediction network primed with BOS, then for each encoder frame
joint -> log-softmax max -> decoder step for every row -> state committed only where the
symbol is not blank; blanks stay in the returned sequences, which are truncated to the
(un-scaled) ``xlen``; the score is ``-sum_t max log p``.

``beam_search_batch`` is the reference's legacy ``Transducer.beam_search`` (models.py:121-202,
``prefix=False``) for a batch of utterances in lockstep (csrc/decode.hip, second half);
``beam_search_enc`` is the same search over a given encoder output, and ``StreamingBeamSearch`` runs it over
encoder output that arrives chunk by chunk, carrying the beams from chunk to chunk.

Every beam search here takes an optional external language model for shallow fusion (``lm=``, an
``edgedict_amd.lm.LMModel``: the reference's ``LMModel``, models.py:224-261).  A popped hypothesis y* with fp64 score
``base`` feeds its last token to the LM from y*'s stored LM state; with ``lp_lm = log_softmax(LM logits)`` (fp32) a
non-blank child k scores ``base + (double)lp_rnnt[k] + (lm_weight * (double)lp_lm[k] + length_bonus)`` (fp64, in this
order), the blank child ``base + (double)lp_rnnt[blank]`` (the LM sees no blank).  There is no end-of-sentence term.
The stop test and the B[:W] / B[0] rules are unchanged and apply to the fused scores; the returned score is -(fused
log p).  The LM's root token is ``lm_bos`` (default 1, the start token ``cli/train_lm.py`` prepends) from a zero state,
or, when streaming, the last committed token once a stream has committed one.  ``lm_weight = length_bonus = 0`` gives
tokens, scores and expansion counts bit-equal to the search without an LM.  A positive ``length_bonus`` can raise the
pops per frame; hitting ``max_expansions`` stays an error.

``beam_search_nbest`` (``_enc``, ``_rows``; ``StreamingBeamSearch(..., detail=True).nbest()``) runs the same search and
returns the WHOLE list B of the last frame as ``NBestResult`` objects: every hypothesis with the encoder frame on which
each of its tokens was emitted and the token's score increment (csrc/decode.hip keeps both per token-tree node).

Every beam search also takes a contextual-biasing list (``bias=``, an ``edgedict_amd.bias.ContextGraph``: phrases to
prefer, given at run time), alone or together with ``lm=``.  Every hypothesis then carries a state of the phrase
automaton beside its prediction-network state, and a non-blank child k scores ``(base + lp_rnnt[k]) + D(s, k)``, with an
LM ``((base + lp_rnnt[k]) + (lm_weight * lp_lm[k] + length_bonus)) + D(s, k)`` (fp64, in this order), where
``D(s, k) = held[goto(s, k)] - pend[s]`` is the automaton's increment; the blank child is unchanged.  A partial match
that breaks gives its bonus back, a completed phrase keeps it.  ``NBestResult.token_logp`` and ``logp`` include the
bias increments.  Not in scope: output links (a phrase that occurs only inside a longer partial match that then breaks
is not credited), an end-of-utterance retraction of a still-pending bonus, and the greedy search (not biased);
``prefix=True`` with a bias list raises ``ValueError``, as with an LM.  ``bias=None``, an empty list and a list whose
boosts are all 0 give tokens, scores and expansion counts bit-equal to the search without one (the first two run the
plain kernels).  See ``edgedict_amd.bias``.

``ctc_beam_search`` is the first pass from the encoder alone: a CTC prefix beam search on the CTC head's logits
(``Transducer(ctc_weight > 0)``; csrc/ctc_decode.hip), all frames inside one launch, returning ranked ``NBestResult``
lists; it takes ``bias=`` too, and ``lm=`` - there an ``edgedict_amd.ngram.NGramLM``, a back-off n-gram in device
tables read inside the walk (``lm_weight``, ``length_bonus``), not an ``LMModel``.  The frame-synchronous search
(``sync_beam_search*``) takes either kind as ``lm=``; the best-first ``beam_search*`` take an ``LMModel`` only.  ``lm_rescore`` re-ranks any
search's ``NBestResult`` lists with such an n-gram (``NBestResult.lm_logp``; csrc/ngram.hip).

``sync_beam_search`` (``_nbest``, ``_enc``, ``_rows``) is a SECOND RNN-T beam search, frame-synchronous (at most one
symbol per frame and hypothesis, all B x W hypotheses in one step per frame, equal sequences merged by log-add;
csrc/decode_sync.hip).  A different algorithm from ``beam_search_batch``: it does not return the same hypotheses, and
takes neither ``lm=`` nor ``bias=`` nor ``prefix=``.  ``StreamingSyncBeamSearch`` runs it over encoder output that
arrives chunk by chunk, carrying every stream's beam in a persistent device state, with the offline search's bits.

``skip_blank=threshold`` (keyword only, on ``beam_search_batch``, ``beam_search_nbest``, ``sync_beam_search_fusion`` and
``sync_beam_search_nbest``; needs ``Transducer(ctc_weight > 0)``): the search runs only on the encoder frames whose CTC
blank posterior is at most ``threshold`` (``skip_blank_frames``: the head's logits, ``loss.ctc_blank_skip``, one read
to the host, ``gather_frames``; csrc/frame_skip.hip), through the ``_enc`` form on the compacted output, and the N-best
forms report ``frames`` in the original numbering.  Everything else passes through; ``prefix=True`` raises
``ValueError``.  Not for the greedy search, the streaming searches or ``ctc_beam_search``.  None launches nothing new.

``ctc_rescore=weight`` (keyword only, on ``beam_search_nbest``, ``sync_beam_search_nbest`` and their ``_enc`` forms;
needs ``Transducer(ctc_weight > 0)``): joint CTC / transducer rescoring, the cheap second pass.  The list the search
returns is scored by the CTC head (``ctc_rescore``: the head's logits, ``loss.ctc_score_nbest`` on all hypotheses of
the batch at once, one read to the host; csrc/ctc_score.hip), ``logp`` becomes ``logp + weight * ctc_logp`` and the list
is sorted by it; the CTC score itself is kept in ``NBestResult.ctc_logp``.  With ``skip_blank=`` the head scores the
UNSKIPPED encoder output.  ``Transducer.rescore_nbest`` does the same to lists obtained elsewhere (``ctc_beam_search``,
a streaming search's ``nbest()``).  No length normalisation, no LM term, no CTC prefix score inside the frame loop.
None launches nothing new.

``ilm_weight=weight`` (keyword only, on ``sync_beam_search_fusion``, ``sync_beam_search_nbest``, the ``_enc`` / ``_rows``
forms and ``StreamingSyncFusionBeamSearch``): internal-LM estimation.  The log-probabilities of the transducer's own
prior - the log-softmax over the non-blank symbols of the joint on an all-zero encoder row - are subtracted from every
non-blank candidate's score inside the frame loop (csrc/decode_sync.hip, csrc/decode_fused.hip), with or without
``lm=`` / ``bias=``.  ``ilm_logits`` is the raw kernel call, ``Transducer.ilm_logprobs`` / ``ilm_score`` score a text
with the internal LM (csrc/ilm_score.hip).  Not for the best-first searches.  None launches nothing new.

``hypothesis_confidence`` / ``ctc_hypothesis_confidence`` (``Transducer.confidence``) are a post-pass over the
``NBestResult`` lists of any of these searches: token, word and utterance confidences from the acoustic model's whole
output distribution on each token's frame (normalised Tsallis or Shannon entropy, ``confidence_measure``), by
re-evaluating the joint at every token's (frame, prefix) - or reading the CTC head's logits there - and reducing each
row of logits to five statistics (csrc/confidence.hip).  LM, ILME and bias terms take no part; no search changes.
"""
import ctypes

import numpy as np
import torch

from . import _lib, ops
from ._lib import dtype_code


def _ptr_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


class SearchState:
    """Prediction-network state of a batch of hypotheses (one per row)."""

    def __init__(self, dec_out, h, c):
        self.dec_out = dec_out      # [B, P_dec] compute dtype
        self.h = h                  # [L, B, H] fp32
        self.c = c


def init_search_state(model, batch):
    """decoder(BOS) for every row — rnnt/models.py:247, rnnt/stream.py:84-91."""
    dev = model.decoder.embed.weight.device
    empty = torch.empty(batch, 0, dtype=torch.int32, device=dev)
    dec, (h, c) = model.decoder(empty)
    return SearchState(dec[:, 0].contiguous(), h.contiguous(), c.contiguous())


def run_search(model, enc_out, state, unk=-1, want_score=True):
    """Advance ``state`` over all frames of ``enc_out`` [B, T, P_enc] (compute dtype).
    Returns (tokens int32 [B, T] on device, score fp32 [B] or None)."""
    cd = enc_out.dtype
    B, T, P = enc_out.shape
    net = _SearchNet(model, cd)
    E1 = net.e1(enc_out)
    lib = _lib.load()
    dev = enc_out.device
    nbytes = lib.edgedict_greedy_workspace_bytes(dtype_code(cd), B, net.J, net.V, net.E, net.L, net.H, net.P2)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    tokens = torch.empty(B, max(T, 1), dtype=torch.int32, device=dev)
    score = torch.zeros(B, dtype=torch.float32, device=dev) if want_score else None
    keep = (E1, net, ws)   # alive until the stream is done
    rc = lib.edgedict_greedy_decode(
        dtype_code(cd), _lib.ptr(E1), ctypes.c_longlong(T * net.J), ctypes.c_longlong(net.J), B, T, *net.args(P),
        _lib.ptr(state.h), _lib.ptr(state.c), _lib.ptr(state.dec_out), int(model.blank), int(unk),
        _lib.ptr(tokens), tokens.stride(0), _lib.ptr(score), _lib.ptr(ws), _lib.stream_ptr())
    _lib.check(rc, "greedy_decode")
    del keep
    return tokens[:, :T], score


def greedy_decode_batch(model, xs, xlen):
    _lib.require_cuda(xs)
    enc_out, _ = model.encoder(xs)
    state = init_search_state(model, xs.shape[0])
    tokens, score = run_search(model, enc_out.contiguous(), state, unk=-1, want_score=True)
    toks = tokens.cpu().numpy().astype(np.int64)
    # the copy above synchronised: a bounded in-kernel wait of the encoder stack that gave up during THIS call
    # has written its code by now (an inference call has no later step that would notice it)
    from . import encoder_stack
    encoder_stack.check_wsr_error()
    lens = xlen.cpu().numpy() if torch.is_tensor(xlen) else np.asarray(xlen)
    return [seq[:int(n)] for seq, n in zip(toks, lens)], score


def _vocab(model):
    return model.joint.joint[2].weight.shape[0]


class SkippedFrames:
    """What ``skip_blank_frames`` returns: ``enc_out`` [B, Tc, P] (the kept frames of every utterance compacted to the
    front, zero rows behind ``lens[b]``), ``lens`` int32 numpy [B] (kept frames per utterance, ``Tc = lens.max()``) and
    ``frame_map`` int32 numpy [B, T] (the original index of the j-th kept frame, -1 behind ``lens[b]``)."""

    def __init__(self, enc_out, lens, frame_map):
        self.enc_out = enc_out
        self.lens = lens
        self.frame_map = frame_map

    def restore(self, results):
        """Rewrite ``frames`` of the ``NBestResult`` list of a search over ``enc_out`` into the original frame numbers
        (in place; returns the list)."""
        for b, r in enumerate(results):
            r.frames = [self.frame_map[b, np.asarray(f, dtype=np.int64)].astype(np.int32) for f in r.frames]
        return results


def _check_skip(model, skip_blank, prefix=False):
    """The argument rules of ``skip_blank=`` (raised before anything touches the device): the threshold as a float."""
    from .loss import check_skip_threshold
    thr = check_skip_threshold(skip_blank)
    if prefix:
        raise ValueError("skip_blank with prefix=True is not supported: the prefix variant's sums are defined over all "
                         "frames of an utterance")
    if getattr(model, "ctc_head", None) is None:
        raise RuntimeError("this model has no CTC head: construct it with Transducer(..., ctc_weight > 0)")
    return thr


def gather_frames(enc_out, frame_map, kept, Tc, out=None):
    """``out[b, j] = enc_out[b, frame_map[b, j]]`` for ``j < kept[b]``, zero rows for ``kept[b] <= j < Tc``
    (csrc/frame_skip.hip): ``enc_out`` [B, T, P] float32 / bfloat16, contiguous; ``frame_map`` int32 [B, T] and ``kept``
    int32 [B] on the device, as ``loss.ctc_blank_skip`` returns them; ``1 <= Tc <= T`` a host int.  ``out``: a contiguous
    [B, Tc, P] tensor of ``enc_out``'s dtype to write into (default: a new one).  No host sync."""
    if enc_out.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("enc_out must be float32 or bfloat16, got %s" % enc_out.dtype)
    if enc_out.dim() != 3 or not enc_out.is_contiguous():
        raise ValueError("enc_out must be contiguous [B, T, P]")
    B, T, P = enc_out.shape
    Tc = int(Tc)
    if frame_map.dtype != torch.int32 or kept.dtype != torch.int32:
        raise TypeError("frame_map and kept must be int32")
    if tuple(frame_map.shape) != (B, T) or tuple(kept.shape) != (B,) or not frame_map.is_contiguous() \
            or not kept.is_contiguous():
        raise ValueError("frame_map must be contiguous [B, T] = [%d, %d] and kept [B]" % (B, T))
    if B < 1 or P < 1 or not 1 <= Tc <= T:
        raise ValueError("need B, P >= 1 and 1 <= Tc <= T (B = %d, P = %d, Tc = %d, T = %d)" % (B, P, Tc, T))
    if out is None:
        out = torch.empty(B, Tc, P, dtype=enc_out.dtype, device=enc_out.device)
    elif out.dtype != enc_out.dtype or tuple(out.shape) != (B, Tc, P) or not out.is_contiguous():
        raise ValueError("out must be contiguous [B, Tc, P] of enc_out's dtype")
    _lib.require_cuda(enc_out, frame_map, kept, out)
    _lib.call("frame_skip_gather", enc_out.detach(), dtype_code(enc_out.dtype), frame_map, kept, B, T, P, Tc, out)
    return out


@torch.no_grad()
def skip_blank_frames(model, enc_out, lens, threshold):
    """Drop the encoder frames on which the model's CTC head is sure nothing is emitted: frame ``t < lens[b]`` of
    ``enc_out`` [B, T, P] (compute dtype, device; ``lens`` host ints or None for all T) is kept iff the head's blank
    posterior on it is at most ``threshold`` (in (0, 1]; ``loss.ctc_blank_skip``).  The head's logits, the decision and
    the compaction run on the device; ONE read brings the kept counts and the frame map to the host, which sizes the
    gather.  Returns a ``SkippedFrames``: run an ``_enc`` search on its ``enc_out`` with its ``lens`` and pass an N-best
    result through its ``restore``.  ``Tc = 0`` (every frame of every utterance dropped) is legal.  Raises
    ``RuntimeError`` on a model built without ``ctc_weight > 0``."""
    from .loss import ctc_blank_skip
    thr = _check_skip(model, threshold)
    _lib.require_cuda(enc_out)
    enc_out = enc_out.contiguous()
    B, T, P = enc_out.shape
    if T < 1:
        return SkippedFrames(enc_out, np.zeros(B, dtype=np.int32), np.zeros((B, 0), dtype=np.int32))
    lens = np.full(B, T, dtype=np.int32) if lens is None else np.ascontiguousarray(lens, dtype=np.int32)
    if lens.shape != (B,) or (lens < 0).any() or (lens > T).any():
        raise ValueError("skip_blank_frames: lens must be [B] ints in [0, %d]" % T)
    act = torch.from_numpy(lens).to(enc_out.device)
    frame_map, kept, _ = ctc_blank_skip(model._ctc_logits(enc_out).contiguous(), act, thr, model.blank)
    host = torch.cat([kept[:, None], frame_map], dim=1).cpu().numpy()
    kept_h, map_h = np.ascontiguousarray(host[:, 0]), np.ascontiguousarray(host[:, 1:])
    Tc = int(kept_h.max())
    out = gather_frames(enc_out, frame_map, kept, Tc) if Tc > 0 else enc_out.new_zeros(B, 0, P)
    return SkippedFrames(out, kept_h, map_h)


def _empty_nbest(B):
    return [NBestResult([np.zeros(0, np.int64)], [np.zeros(0, np.int32)], [np.zeros(0)], [0.0]) for _ in range(B)]


def beam_search_batch(model, xs, xlen=None, W=10, max_expansions=None, prefix=False, *, lm=None, lm_weight=None,
                      length_bonus=0.0, lm_bos=1, bias=None, skip_blank=None):
    """Graves (2012) beam search as the reference's legacy ``Transducer.beam_search`` runs it
    (models.py:121-202), batched: every utterance keeps its own A / B sets and all open utterances
    advance one expansion per lockstep iteration on the device.  ``prefix=True`` is the reference's
    prefix-sum variant (:145-161): see ``edgedict_beam_search`` in include/edgedict_hip.h.

    xs [B, T0, I]; xlen (host or device int tensor, stacked frames) or None for "all frames".
    Returns ``(list of int64 arrays (tokens, no blanks), fp64 tensor [B] = -log p)``: per
    utterance the FIRST hypothesis of the last frame's B list, which is what the reference returns
    (its ``sorted`` calls are no-ops).  ``max_expansions`` bounds the pops per utterance and frame
    (default 8 W, at least 16); hitting it raises instead of truncating the search.

    ``lm`` / ``lm_weight`` / ``length_bonus`` / ``lm_bos``: LM shallow fusion, see the module docstring (``lm`` needs
    ``lm_weight``; ``prefix=True`` with an LM and an LM of another vocabulary raise ``ValueError``).

    ``bias``: a contextual-biasing list (``edgedict_amd.bias.ContextGraph``), see the module docstring; the same two
    cases raise ``ValueError``.

    ``skip_blank``: a threshold in (0, 1] - the search then runs only on the encoder frames whose CTC blank posterior
    is at most the threshold (``skip_blank_frames``; the model needs a CTC head, ``prefix=True`` raises ``ValueError``).
    None: nothing of this runs."""
    from .bias import check_bias_args
    from .lm import check_fusion_args
    check_fusion_args(lm, lm_weight, _vocab(model), prefix)
    check_bias_args(bias, _vocab(model), prefix)
    if skip_blank is not None:
        _check_skip(model, skip_blank, prefix)
    _lib.require_cuda(xs)
    if W < 1:
        raise ValueError("beam width must be >= 1")
    enc_out, _ = model.encoder(xs)
    enc_out = enc_out.contiguous()
    B, T, P = enc_out.shape
    if xlen is None:
        lens = None
    else:
        xl = xlen.detach().cpu() if torch.is_tensor(xlen) else torch.as_tensor(xlen)
        lens = model.scale_length(enc_out, xl).numpy().astype(np.int32)
    if skip_blank is not None:
        sk = skip_blank_frames(model, enc_out, lens, skip_blank)
        if sk.enc_out.shape[1] == 0:        # every frame dropped: the empty hypothesis, nothing to launch
            beam_search_batch.last_expansions = 0
            return [np.zeros(0, np.int64) for _ in range(B)], torch.zeros(B, dtype=torch.float64)
        enc_out, lens = sk.enc_out, sk.lens
    return beam_search_enc(model, enc_out, lens, W, max_expansions, prefix, lm=lm, lm_weight=lm_weight,
                           length_bonus=length_bonus, lm_bos=lm_bos, bias=bias)


class SearchNetStruct(ctypes.Structure):
    """ctypes mirror of ``edgedict_search_net_t`` (include/edgedict_hip.h)."""
    _fields_ = [("dtype", ctypes.c_int), ("J", ctypes.c_int), ("W1d", ctypes.c_void_p), ("ldw1", ctypes.c_longlong),
                ("b1", ctypes.c_void_p), ("P2", ctypes.c_int), ("W2", ctypes.c_void_p), ("b2", ctypes.c_void_p),
                ("V", ctypes.c_int), ("emb", ctypes.c_void_p), ("emb_dtype", ctypes.c_int), ("E", ctypes.c_int),
                ("L", ctypes.c_int), ("w_ih", ctypes.c_void_p), ("w_hh", ctypes.c_void_p), ("b_ih", ctypes.c_void_p),
                ("b_hh", ctypes.c_void_p), ("H", ctypes.c_int), ("Wp", ctypes.c_void_p), ("bp", ctypes.c_void_p),
                ("blank", ctypes.c_int), ("bos", ctypes.c_int)]


class SearchOpts(ctypes.Structure):
    """ctypes mirror of ``edgedict_search_opts_t`` (include/edgedict_hip.h)."""
    _fields_ = [("lm", ctypes.c_void_p), ("bias", ctypes.c_void_p), ("ilm_weight", ctypes.c_void_p),
                ("ngram", ctypes.c_void_p)]


class _SearchNet:
    """The prediction network's and the joint's weights in the compute dtype ``cd`` (converted once through
    ``WEIGHTS``) with the shapes and ctypes arguments the native searches take."""

    def __init__(self, model, cd):
        self.blank = int(model.blank)
        self._refs = {}
        from .models import WEIGHTS
        dec = model.decoder
        l1, l2 = model.joint.joint[0], model.joint.joint[2]
        self.J, self.V = l1.weight.shape[0], l2.weight.shape[0]
        self.P2 = dec.proj.weight.shape[0]
        self.L, self.H = dec.lstm.num_layers, dec.lstm.hidden_size
        self.E = dec.embed.weight.shape[1]
        self.w1c = WEIGHTS.get(l1.weight, cd)
        self.w2c = WEIGHTS.get(l2.weight, cd)
        self.wpc = WEIGHTS.get(dec.proj.weight, cd)
        self.w_ih = [WEIGHTS.get(dec.lstm.layer(k)[0], cd) for k in range(self.L)]
        self.w_hh = [WEIGHTS.get(dec.lstm.layer(k)[1], cd) for k in range(self.L)]
        self.b_ih = [dec.lstm.layer(k)[2].detach() for k in range(self.L)]
        self.b_hh = [dec.lstm.layer(k)[3].detach() for k in range(self.L)]
        self.b1, self.b2 = l1.bias.detach(), l2.bias.detach()
        self.emb, self.bp = dec.embed.weight.detach(), dec.proj.bias.detach()
        self.cd = cd

    def e1(self, enc_out):
        """The encoder half of the joint's first Linear for all frames of ``enc_out`` [B, T, P] at once: [B * T, J]."""
        B, T, P = enc_out.shape
        return ops.gemm(enc_out.reshape(B * T, P), self.w1c[:, :P]) if T > 0 else enc_out.new_empty(0, self.J)

    def ref(self, P=0):
        """``const edgedict_search_net_t*`` of the beam searches' native calls, for an encoder output of width P (cached
        per P; the struct and the pointer arrays it names live as long as this object).  The size queries read the
        shapes alone: any P serves them."""
        if P not in self._refs:
            from .tokenizer import BOS
            arrays = [_ptr_array(t) for t in (self.w_ih, self.w_hh, self.b_ih, self.b_hh)]
            vp = lambda a: ctypes.cast(a, ctypes.c_void_p)
            s = SearchNetStruct(
                dtype=dtype_code(self.cd), J=self.J, W1d=_lib.ptr(self.w1c[:, P:]), ldw1=self.w1c.stride(0),
                b1=_lib.ptr(self.b1), P2=self.P2, W2=_lib.ptr(self.w2c), b2=_lib.ptr(self.b2), V=self.V,
                emb=_lib.ptr(self.emb), emb_dtype=dtype_code(self.emb.dtype), E=self.E, L=self.L, w_ih=vp(arrays[0]),
                w_hh=vp(arrays[1]), b_ih=vp(arrays[2]), b_hh=vp(arrays[3]), H=self.H, Wp=_lib.ptr(self.wpc),
                bp=_lib.ptr(self.bp), blank=self.blank, bos=int(BOS))
            self._refs[P] = (s, arrays)
        return ctypes.byref(self._refs[P][0])

    def args(self, P):
        """(W1d ... bp) of ``edgedict_greedy_decode``, for an encoder output of width P."""
        w1d = self.w1c[:, P:]
        return (self.J, _lib.ptr(w1d), ctypes.c_longlong(self.w1c.stride(0)), _lib.ptr(self.b1), self.P2,
                _lib.ptr(self.w2c), _lib.ptr(self.b2), self.V, _lib.ptr(self.emb), dtype_code(self.emb.dtype),
                self.E, self.L, _ptr_array(self.w_ih), _ptr_array(self.w_hh), _ptr_array(self.b_ih),
                _ptr_array(self.b_hh), self.H, _lib.ptr(self.wpc), _lib.ptr(self.bp))


def _opts(flm=None, bref=None, ilm=None, ng=None):
    """``const edgedict_search_opts_t*`` of a native call: the fusion LM ``flm`` (``FusionLM``), the bias list ``bref``
    (``ContextGraph.ref``), the ILME weight ``ilm`` (a ``c_double``), the n-gram ``ng`` (an ``NGramStruct``:
    ``NGramLM.struct(device, weight, bonus)``).  None - a null pointer, the plain search - when all four are absent.
    The pointer keeps what it names alive."""
    if flm is None and bref is None and ilm is None and ng is None:
        return None
    o = SearchOpts(lm=None if flm is None else ctypes.addressof(flm.struct),
                   bias=None if bref is None else ctypes.addressof(bref._obj),
                   ilm_weight=None if ilm is None else ctypes.addressof(ilm),
                   ngram=None if ng is None else ctypes.addressof(ng))
    o.keep = (flm, bref, ilm, ng)
    return ctypes.pointer(o)


def _sync_lm_opts(lm, cd, device, lm_weight, length_bonus, lm_bos):
    """``(flm, ng)`` of ``_opts`` for the ``lm=`` of a frame-synchronous search: an ``LMModel`` becomes a ``FusionLM``,
    an ``NGramLM`` its ``NGramStruct`` on ``device`` (``lm_bos`` is not read with an n-gram: the empty sequence stands
    on the table's ``start``)."""
    from .lm import FusionLM
    from .ngram import NGramLM
    if lm is None:
        return None, None
    if isinstance(lm, NGramLM):
        return None, lm.struct(device, lm_weight, length_bonus)
    return FusionLM(lm, cd, lm_weight, length_bonus, lm_bos), None


def joint_rows(model, enc_out):
    """E1 = enc_out [B, T, P] times the encoder half of the joint's first Linear, [B * T, J] in the compute dtype: the
    rows both beam searches read (``beam_search_rows``, ``StreamingBeamSearch.advance``)."""
    return _SearchNet(model, enc_out.dtype).e1(enc_out.contiguous())


def beam_search_enc(model, enc_out, lens=None, W=10, max_expansions=None, prefix=False, *, lm=None, lm_weight=None,
                    length_bonus=0.0, lm_bos=1, bias=None):
    """``beam_search_batch`` over a given encoder output ``enc_out`` [B, T, P] (compute dtype) with ``lens`` (host int,
    encoder frames per utterance; None: all T)."""
    from .bias import check_bias_args
    from .lm import check_fusion_args
    check_fusion_args(lm, lm_weight, _vocab(model), prefix)
    check_bias_args(bias, _vocab(model), prefix)
    enc_out = enc_out.contiguous()
    B, T, P = enc_out.shape
    return beam_search_rows(model, joint_rows(model, enc_out), B, T, P, lens, W, max_expansions, prefix, lm=lm,
                            lm_weight=lm_weight, length_bonus=length_bonus, lm_bos=lm_bos, bias=bias)


def beam_search_rows(model, E1, B, T, P, lens=None, W=10, max_expansions=None, prefix=False, *, lm=None,
                     lm_weight=None, length_bonus=0.0, lm_bos=1, bias=None):
    """``beam_search_enc`` from the joint's encoder rows ``E1`` [B * T, J] (``joint_rows``) of an encoder output of
    width P."""
    from .bias import active, check_bias_args
    from .lm import FusionLM, check_fusion_args
    check_fusion_args(lm, lm_weight, _vocab(model), prefix)
    check_bias_args(bias, _vocab(model), prefix)
    if W < 1:
        raise ValueError("beam width must be >= 1")
    cd = E1.dtype
    lens = np.full(B, T, dtype=np.int32) if lens is None else np.ascontiguousarray(lens, dtype=np.int32)
    EM = int(max_expansions) if max_expansions else max(16, 8 * W)
    net = _SearchNet(model, cd)
    flm = FusionLM(lm, cd, lm_weight, length_bonus, lm_bos) if lm is not None else None
    bref = None
    if active(bias) is not None:
        _lib.require_cuda(E1)
        bref = active(bias).ref(E1.device)
    lib, nref, opts = _lib.load(), net.ref(P), _opts(flm, bref)
    nbytes = lib.edgedict_beam_workspace_bytes(nref, B, T, int(W), EM, int(bool(prefix)), opts)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=E1.device)
    max_tokens = T * EM + 1
    tokens = np.zeros((B, max_tokens), dtype=np.int32)
    ntok = np.zeros(B, dtype=np.int32)
    score = np.zeros(B, dtype=np.float64)
    nexp = ctypes.c_longlong(0)
    rc = lib.edgedict_beam_search(
        nref, _lib.ptr(E1), ctypes.c_longlong(T * net.J), ctypes.c_longlong(net.J), B, T,
        lens.ctypes.data_as(ctypes.c_void_p), int(W), EM, int(bool(prefix)), tokens.ctypes.data_as(ctypes.c_void_p),
        max_tokens, ntok.ctypes.data_as(ctypes.c_void_p), score.ctypes.data_as(ctypes.c_void_p), ctypes.byref(nexp), opts,
        _lib.ptr(ws), _lib.stream_ptr())
    _lib.check(rc, "beam_search")
    beam_search_batch.last_expansions = int(nexp.value)
    seqs = [tokens[b, :ntok[b]].astype(np.int64) for b in range(B)]
    return seqs, torch.from_numpy(score)


class NBestResult:
    """The list B of one utterance's last frame: ``n <= W`` hypotheses **in B's own order, which is insertion order**
    (the order in which the hypotheses emitted blank on the last frame - the reference's ``sorted`` calls discard their
    result, so neither it nor the search here ever ranks B; entry 0 is what ``beam_search_batch`` returns).  Ranking is
    therefore a separate step: ``ranked()``.

    ``tokens[i]``      int64 array: the hypothesis' tokens, no blanks
    ``frames[i]``      int32 array, same length: the encoder frame on which each token was emitted (offline: index into
                       the utterance; streaming: counted since the stream's reset); ``emission_times`` turns them into
                       seconds
    ``token_logp[i]``  float64 array, same length: the increment each token added to the hypothesis' score (with an LM
                       the fused increment ``lp_rnnt + (lm_weight lp_lm + length_bonus)``, with a bias list plus the
                       automaton's increment ``D``); ``logp[i]`` minus their sum is what the hypothesis' blanks
                       contributed
    ``logp``           float64 [n]: log p per hypothesis (fused log p with an LM; plus the total bias with a list);
                       after ``ctc_rescore`` the combined score ``logp + weight * ctc_logp``
    ``ctc_logp``       None, or float64 [n]: the CTC head's log-likelihood of each hypothesis' tokens (``ctc_rescore``
                       fills it; -inf: the head has no path for them)
    ``lm_logp``        None, or float64 [n]: an n-gram LM's log-probability of each hypothesis' tokens (``lm_rescore``
                       fills it)
    """

    def __init__(self, tokens, frames, token_logp, logp, ctc_logp=None, lm_logp=None):
        self.tokens = list(tokens)
        self.frames = list(frames)
        self.token_logp = list(token_logp)
        self.logp = np.asarray(logp, dtype=np.float64)
        self.ctc_logp = None if ctc_logp is None else np.asarray(ctc_logp, dtype=np.float64)
        if not (len(self.tokens) == len(self.frames) == len(self.token_logp) == self.logp.shape[0]):
            raise ValueError("NBestResult: fields of different lengths")
        if self.ctc_logp is not None and self.ctc_logp.shape != self.logp.shape:
            raise ValueError("NBestResult: ctc_logp must have one value per hypothesis")
        self.lm_logp = None if lm_logp is None else np.asarray(lm_logp, dtype=np.float64)
        if self.lm_logp is not None and self.lm_logp.shape != self.logp.shape:
            raise ValueError("NBestResult: lm_logp must have one value per hypothesis")

    def __len__(self):
        return len(self.tokens)

    def ranked(self, merge=True):
        """A new ``NBestResult`` sorted by ``logp`` descending, stably (ties keep B's order).  ``merge=True`` first folds
        entries with identical token sequences into one with log-add (the legacy search keeps them apart: the same
        sequence can be in B twice, reached with different emission frames); the folded entry keeps the frames and
        increments of its most probable member (the first one on ties) and stands at that member's place in B.
        ``ctc_logp`` is carried along; a folded entry keeps its kept member's value (equal token sequences have equal
        CTC scores, so the log-add of combined scores is the combined score of the log-add); ``lm_logp`` likewise."""
        idx = list(range(len(self)))
        logp = self.logp.copy()
        if merge:
            groups = {}
            for i in idx:
                groups.setdefault(tuple(int(t) for t in self.tokens[i]), []).append(i)
            idx = []
            for members in groups.values():
                best = max(members, key=lambda i: (self.logp[i], -i))
                vals = self.logp[members]
                m = vals.max()
                logp[best] = m + np.log(np.exp(vals - m).sum()) if np.isfinite(m) else m
                idx.append(best)
            idx.sort()
        order = sorted(idx, key=lambda i: -logp[i])          # sorted() is stable
        return NBestResult([self.tokens[i] for i in order], [self.frames[i] for i in order],
                           [self.token_logp[i] for i in order], logp[order] if order else np.zeros(0),
                           None if self.ctc_logp is None else (self.ctc_logp[order] if order else np.zeros(0)),
                           None if self.lm_logp is None else (self.lm_logp[order] if order else np.zeros(0)))


def _nbest_results(tokens, frames, tlogp, ntok, nhyp, logp, prefix=None):
    """Host arrays of a native N-best read -> one ``NBestResult`` per row; ``prefix[b]`` = (tokens, frames, increments)
    lists prepended to every hypothesis of row b (the streams' committed log)."""
    out = []
    for b in range(len(nhyp)):
        ts, fs, ls = [], [], []
        for j in range(int(nhyp[b])):
            n = int(ntok[b, j])
            t, f, l = tokens[b, j, :n].astype(np.int64), frames[b, j, :n].astype(np.int32), tlogp[b, j, :n].copy()
            if prefix is not None:
                t = np.concatenate([np.asarray(prefix[b][0], dtype=np.int64), t])
                f = np.concatenate([np.asarray(prefix[b][1], dtype=np.int32), f])
                l = np.concatenate([np.asarray(prefix[b][2], dtype=np.float64), l])
            ts.append(t); fs.append(f); ls.append(l)
        out.append(NBestResult(ts, fs, ls, logp[b, :int(nhyp[b])].copy()))
    return out


CTC_RESCORE_MAX_N = 32


def _check_rescore(model, weight):
    """The argument rules of ``ctc_rescore=`` (raised before anything touches the device): the weight as a float."""
    try:
        w = float(weight)
    except (TypeError, ValueError):
        raise ValueError("the CTC rescoring weight must be a finite number >= 0, got %r" % (weight,)) from None
    if not (np.isfinite(w) and w >= 0.0):
        raise ValueError("the CTC rescoring weight must be finite and >= 0, got %r" % (weight,))
    if getattr(model, "ctc_head", None) is None:
        raise RuntimeError("this model has no CTC head: construct it with Transducer(..., ctc_weight > 0)")
    return w


def combine_ctc(logp, ctc_logp, weight):
    """The combine-and-sort rule of ``ctc_rescore`` on one list (host, float64): ``(combined, order)`` with
    ``combined = logp + weight * ctc_logp`` evaluated as exactly that expression - for ``weight == 0`` ``logp`` itself,
    so no ``0 * inf`` is formed - and ``order`` the stable sort of ``combined``, descending.  A ``ctc_logp`` of -inf
    with ``weight > 0`` gives -inf, which sorts last."""
    logp = np.asarray(logp, dtype=np.float64)
    ctc_logp = np.asarray(ctc_logp, dtype=np.float64)
    combined = logp + weight * ctc_logp if weight > 0 else logp.copy()
    return combined, np.argsort(-combined, kind="stable")


@torch.no_grad()
def ctc_score_lists(model, enc_out, lens, lists):
    """The CTC head's log-likelihood of token sequences: ``lists[b]`` holds the sequences (int arrays without blanks)
    to score on utterance ``b`` of ``enc_out`` [B, T, P] (compute dtype, device; ``lens`` host ints, encoder frames per
    utterance, or None for all T).  The head's logits (``model._ctc_logits``), ONE int32 upload holding all tokens as
    ``[B, N, U]`` (``N`` the longest list, at most 32; ``U`` the longest sequence) with the lengths behind them, ONE
    ``loss.ctc_score_nbest`` call and ONE read to the host.  Returns a list of float64 arrays, one value per sequence
    (-inf: no CTC path).  Raises ``RuntimeError`` on a model built without ``ctc_weight > 0``."""
    from .loss import ctc_score_nbest
    if getattr(model, "ctc_head", None) is None:
        raise RuntimeError("this model has no CTC head: construct it with Transducer(..., ctc_weight > 0)")
    _lib.require_cuda(enc_out)
    enc_out = enc_out.contiguous()
    B, T, _ = enc_out.shape
    lists = [[np.asarray(t, dtype=np.int64).reshape(-1) for t in seqs] for seqs in lists]
    if len(lists) != B:
        raise ValueError("ctc_score_lists: %d lists for a batch of %d utterances" % (len(lists), B))
    lens = np.full(B, T, dtype=np.int32) if lens is None else np.ascontiguousarray(lens, dtype=np.int32)
    if lens.shape != (B,) or (lens < 0).any() or (lens > T).any():
        raise ValueError("ctc_score_lists: lens must be [B] ints in [0, %d]" % T)
    N = max([len(seqs) for seqs in lists], default=0)
    U = max([t.size for seqs in lists for t in seqs], default=0)
    if N > CTC_RESCORE_MAX_N:
        raise ValueError("ctc_score_lists: a list of %d hypotheses exceeds the supported maximum of %d"
                         % (N, CTC_RESCORE_MAX_N))
    if N == 0 or T < 1:             # nothing to score / no frame: no sequence has a path
        return [np.full(len(seqs), -np.inf) for seqs in lists]
    # one upload: hyps [B, N, U], hyp_lens [B, N], n_hyp [B], act_lens [B], back to back
    nh, nl = B * N * U, B * N
    host = np.zeros(nh + nl + 2 * B, dtype=np.int32)
    hyps, hyp_lens = host[:nh].reshape(B, N, U), host[nh:nh + nl].reshape(B, N)
    for b, seqs in enumerate(lists):
        host[nh + nl + b] = len(seqs)
        for n, t in enumerate(seqs):
            hyps[b, n, :t.size] = t
            hyp_lens[b, n] = t.size
    host[nh + nl + B:] = lens
    dev = torch.from_numpy(host).to(enc_out.device)
    scores = ctc_score_nbest(model._ctc_logits(enc_out).contiguous(), dev[nh + nl + B:], dev[:nh].view(B, N, U),
                             dev[nh:nh + nl].view(B, N), dev[nh + nl:nh + nl + B], model.blank).cpu().numpy()
    return [scores[b, :len(seqs)].copy() for b, seqs in enumerate(lists)]


def ctc_rescore(model, enc_out, lens, results, weight):
    """Rescore N-best lists with the model's CTC head: ``results`` (one ``NBestResult`` per utterance of ``enc_out``
    [B, T, P], compute dtype, device; ``lens`` host ints, encoder frames per utterance, or None for all T) from any
    search over this encoder output.  All hypotheses of the batch are scored by ``ctc_score_lists``: one upload, one
    ``loss.ctc_score_nbest`` call, one read to the host.

    Returns new ``NBestResult`` objects: ``ctc_logp`` is the head's log-likelihood of each hypothesis' tokens, ``logp``
    the combined score ``logp + weight * ctc_logp`` (float64 on the host, exactly that expression), the entries sorted
    by it descending, stably, with ``tokens``, ``frames`` and ``token_logp`` permuted along.  ``weight`` must be finite
    and ``>= 0`` (``ValueError``); for ``weight == 0`` the combined score is ``logp`` itself and the order its stable
    sort.  A hypothesis without a CTC path (``ctc_logp`` -inf) gets -inf for ``weight > 0`` and sorts last.  An empty
    list stays empty.  Equal token sequences are NOT merged here: chain ``.ranked(merge=True)``.  No length
    normalisation, no LM term.  Raises ``RuntimeError`` on a model built without ``ctc_weight > 0``."""
    w = _check_rescore(model, weight)
    results = list(results)
    scores = ctc_score_lists(model, enc_out, lens, [r.tokens for r in results])
    out = []
    for r, ctc in zip(results, scores):
        combined, order = combine_ctc(r.logp, ctc, w)
        out.append(NBestResult([r.tokens[i] for i in order], [r.frames[i] for i in order],
                               [r.token_logp[i] for i in order], combined[order], ctc[order]))
    return out


def lm_rescore(results, lm, weight, length_bonus=0.0, eos=False):
    """Rescore N-best lists with an n-gram LM (``ngram.NGramLM``): all hypotheses of ``results`` (one ``NBestResult``
    per utterance, from any search) are scored by ``lm.score_lists`` - one upload, one ``ngram_score`` launch, one read.
    Returns new ``NBestResult`` objects: ``lm_logp`` is the LM's log-probability of each hypothesis' tokens (from
    ``<s>``, with the end-of-sentence step for ``eos=True``), ``logp`` the combined score
    ``logp + (weight * lm_logp + length_bonus * ntok)`` (float64 on the host, exactly that expression), the entries
    sorted by it descending, stably; ``ctc_logp`` is carried along.  For ``weight == 0`` the LM term is left out (no
    ``0 * -inf``) and ``lm_logp`` is still filled.  ``weight`` must be finite and ``>= 0``,
    ``length_bonus`` finite (``ValueError``)."""
    from .ngram import NGramLM
    if not isinstance(lm, NGramLM):
        raise TypeError("lm_rescore: lm must be an edgedict_amd.ngram.NGramLM (got %s)" % type(lm).__name__)
    w, lb = float(weight), float(length_bonus)
    if not (np.isfinite(w) and w >= 0.0) or not np.isfinite(lb):
        raise ValueError("lm_rescore: weight must be finite and >= 0, length_bonus finite (got %r, %r)"
                         % (weight, length_bonus))
    results = list(results)
    scores = lm.score_lists([r.tokens for r in results], bos=True, eos=eos) if results else []
    out = []
    for r, lp in zip(results, scores):
        ntok = np.array([len(t) for t in r.tokens], dtype=np.float64)
        combined = r.logp + (w * lp + lb * ntok) if w > 0 else r.logp + lb * ntok      # (no 0 * -inf)
        order = np.argsort(-combined, kind="stable")
        out.append(NBestResult([r.tokens[i] for i in order], [r.frames[i] for i in order],
                               [r.token_logp[i] for i in order], combined[order],
                               None if r.ctc_logp is None else r.ctc_logp[order], lp[order]))
    return out


def beam_search_nbest(model, xs, xlen=None, W=10, max_expansions=None, *, lm=None, lm_weight=None, length_bonus=0.0,
                      lm_bos=1, bias=None, skip_blank=None, ctc_rescore=None):
    """``beam_search_batch`` (``prefix=False``) returning, per utterance, an ``NBestResult``: all ``n <= W`` hypotheses
    of the last frame's list B in B's order, each with its tokens, the encoder frame every token was emitted on and the
    score increment every token added, and ``logp`` (log p, not negated).  Entry 0 is exactly what ``beam_search_batch``
    returns (same tokens, ``logp[0] == -score`` bit for bit), and ``beam_search_batch.last_expansions`` is set as there.
    An utterance of 0 frames yields one empty hypothesis with ``logp`` 0.  The prefix-sum variant is not available
    here: its merge changes a score at frame starts, so the increments would no longer add up.  With ``bias`` (module
    docstring) ``token_logp`` and ``logp`` include the bias increments.  ``skip_blank``: as in ``beam_search_batch``;
    ``frames`` stay in the original frame numbering.  ``ctc_rescore``: a weight ``>= 0`` - the list then goes through
    ``ctc_rescore`` (the module-level function; on the unskipped encoder output) before it is returned: ``ctc_logp``
    filled, ``logp`` the combined score, sorted by it.  None: nothing of this runs."""
    from .bias import check_bias_args
    from .lm import check_fusion_args
    check_fusion_args(lm, lm_weight, _vocab(model), False)
    check_bias_args(bias, _vocab(model), False)
    if skip_blank is not None:
        _check_skip(model, skip_blank)
    if ctc_rescore is not None:
        _check_rescore(model, ctc_rescore)
    _lib.require_cuda(xs)
    if W < 1:
        raise ValueError("beam width must be >= 1")
    enc_out, _ = model.encoder(xs)
    enc_out = enc_out.contiguous()
    if xlen is None:
        lens = None
    else:
        xl = xlen.detach().cpu() if torch.is_tensor(xlen) else torch.as_tensor(xlen)
        lens = model.scale_length(enc_out, xl).numpy().astype(np.int32)
    if skip_blank is not None:
        sk = skip_blank_frames(model, enc_out, lens, skip_blank)
        if sk.enc_out.shape[1] == 0:        # every frame dropped: the empty hypothesis, nothing to launch
            beam_search_batch.last_expansions = 0
            return _rescored(model, enc_out, lens, _empty_nbest(enc_out.shape[0]), ctc_rescore)
        return _rescored(model, enc_out, lens,
                         sk.restore(beam_search_nbest_enc(model, sk.enc_out, sk.lens, W, max_expansions, lm=lm,
                                                          lm_weight=lm_weight, length_bonus=length_bonus,
                                                          lm_bos=lm_bos, bias=bias)), ctc_rescore)
    return beam_search_nbest_enc(model, enc_out, lens, W, max_expansions, lm=lm, lm_weight=lm_weight,
                                 length_bonus=length_bonus, lm_bos=lm_bos, bias=bias, ctc_rescore=ctc_rescore)


def _rescored(model, enc_out, lens, results, weight):
    """``results`` as they are for ``weight`` None, else through ``ctc_rescore`` on ``enc_out``."""
    return results if weight is None else ctc_rescore(model, enc_out, lens, results, weight)


def beam_search_nbest_enc(model, enc_out, lens=None, W=10, max_expansions=None, *, lm=None, lm_weight=None,
                          length_bonus=0.0, lm_bos=1, prefix=False, bias=None, ctc_rescore=None):
    """``beam_search_nbest`` over a given encoder output ``enc_out`` [B, T, P] (compute dtype) with ``lens`` (host int,
    encoder frames per utterance; None: all T).  ``ctc_rescore``: as there, the head scoring this ``enc_out``."""
    from .bias import check_bias_args
    check_bias_args(bias, _vocab(model), prefix)
    if ctc_rescore is not None:
        _check_rescore(model, ctc_rescore)
    enc_out = enc_out.contiguous()
    B, T, P = enc_out.shape
    return _rescored(model, enc_out, lens,
                     beam_search_nbest_rows(model, joint_rows(model, enc_out), B, T, P, lens, W, max_expansions, lm=lm,
                                            lm_weight=lm_weight, length_bonus=length_bonus, lm_bos=lm_bos,
                                            prefix=prefix, bias=bias), ctc_rescore)


def beam_search_nbest_rows(model, E1, B, T, P, lens=None, W=10, max_expansions=None, *, lm=None, lm_weight=None,
                           length_bonus=0.0, lm_bos=1, prefix=False, max_tokens=None, bias=None):
    """``beam_search_nbest_enc`` from the joint's encoder rows ``E1`` [B * T, J] (``joint_rows``) of an encoder output
    of width P.  ``prefix=True`` raises ``ValueError`` (see ``beam_search_nbest``).  ``max_tokens`` bounds a hypothesis'
    length (default: what the token tree can hold, T x max_expansions + 1); a longer one raises, it is never cut."""
    from .bias import active, check_bias_args
    from .lm import FusionLM, check_fusion_args
    if prefix:
        raise ValueError("beam_search_nbest: prefix=True is not supported with token detail (the prefix merge changes a "
                         "hypothesis' score at frame starts, so the per-token increments would no longer add up)")
    check_fusion_args(lm, lm_weight, _vocab(model), False)
    check_bias_args(bias, _vocab(model), False)
    if W < 1:
        raise ValueError("beam width must be >= 1")
    cd = E1.dtype
    lens = np.full(B, T, dtype=np.int32) if lens is None else np.ascontiguousarray(lens, dtype=np.int32)
    EM = int(max_expansions) if max_expansions else max(16, 8 * W)
    net = _SearchNet(model, cd)
    flm = FusionLM(lm, cd, lm_weight, length_bonus, lm_bos) if lm is not None else None
    lib = _lib.load()
    bref = None
    if active(bias) is not None:
        _lib.require_cuda(E1)
        bref = active(bias).ref(E1.device)
    nref, opts = net.ref(P), _opts(flm, bref)
    nbytes = lib.edgedict_beam_workspace_bytes(nref, B, T, int(W), EM, 0, opts)
    MT = T * EM + 1 if max_tokens is None else int(max_tokens)
    dev = E1.device
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    detail = torch.empty(lib.edgedict_beam_detail_bytes(B, T, EM), dtype=torch.uint8, device=dev)
    result = torch.empty(lib.edgedict_beam_nbest_result_bytes(B, W, MT), dtype=torch.uint8, device=dev)
    tokens = np.empty((B, W, MT), dtype=np.int32)       # (only the used columns are written and read)
    frames = np.empty((B, W, MT), dtype=np.int32)
    tlogp = np.empty((B, W, MT), dtype=np.float64)
    ntok = np.zeros((B, W), dtype=np.int32)
    nhyp = np.zeros(B, dtype=np.int32)
    logp = np.zeros((B, W), dtype=np.float64)
    nexp = ctypes.c_longlong(0)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = lib.edgedict_beam_search_nbest(
        nref, _lib.ptr(E1), ctypes.c_longlong(T * net.J), ctypes.c_longlong(net.J), B, T, vp(lens), int(W), EM, 0,
        vp(tokens), vp(frames), vp(tlogp), MT, vp(ntok), vp(nhyp), vp(logp), ctypes.byref(nexp), opts, _lib.ptr(ws),
        _lib.ptr(detail), _lib.ptr(result), _lib.stream_ptr())
    _lib.check(rc, "beam_search_nbest")
    beam_search_batch.last_expansions = int(nexp.value)
    return _nbest_results(tokens, frames, tlogp, ntok, nhyp, logp)


SYNC_BEAM_MAX_W = 32


def _check_sync_width(W):
    if not 1 <= int(W) <= SYNC_BEAM_MAX_W:
        raise ValueError("sync_beam_search: beam width W = %r outside [1, %d]" % (W, SYNC_BEAM_MAX_W))


def _check_sync_fusion(model, lm, lm_weight, bias, length_bonus=0.0):
    """The fusion argument rules of the ``sync_beam_search*`` entry points (raised before anything is launched).  ``lm``
    is an ``LMModel`` (``check_fusion_args``) or an ``NGramLM`` (``ngram.check_ngram_args``: a finite ``lm_weight >= 0``,
    a finite ``length_bonus``, the transducer's vocabulary and blank, at most ``SYNC_NGRAM_MAX_V`` symbols)."""
    from .bias import check_bias_args
    from .lm import LMModel, check_fusion_args
    from .ngram import SYNC_NGRAM_MAX_V, NGramLM, check_ngram_args
    if isinstance(lm, NGramLM):
        check_ngram_args(lm, lm_weight, length_bonus, _vocab(model), int(model.blank), "the transducer's",
                         SYNC_NGRAM_MAX_V)
    elif lm is not None and not isinstance(lm, LMModel):
        raise ValueError("lm must be an edgedict_amd.lm.LMModel or an edgedict_amd.ngram.NGramLM (got %s)"
                         % type(lm).__name__)
    else:
        check_fusion_args(lm, lm_weight, _vocab(model), False)
    check_bias_args(bias, _vocab(model), False)


def _check_ilm_weight(ilm_weight):
    """``ilm_weight`` of the ``sync_beam_search*`` entry points: None (no internal-LM estimation) or a finite number
    ``>= 0``, else ``ValueError`` (raised before anything is launched).  Returns None or the weight as a ``c_double``."""
    if ilm_weight is None:
        return None
    ok = isinstance(ilm_weight, (int, float, np.integer, np.floating)) and not isinstance(ilm_weight, bool)
    if not ok or not np.isfinite(ilm_weight) or ilm_weight < 0:
        raise ValueError("sync_beam_search: ilm_weight = %r must be a finite number >= 0 (or None)" % (ilm_weight,))
    return ctypes.c_double(float(ilm_weight))


def _no_ilm(ilm_weight, what):
    """The best-first searches have another expand kernel: internal-LM estimation is the frame-synchronous search's."""
    if ilm_weight is not None:
        raise ValueError("%s: ilm_weight is not supported here (internal-LM estimation is in sync_beam_search*)" % what)


def ilm_logits(model, dec_rows):
    """The internal LM's logits, fp32 [R, V], of R rows of prediction-network output ``dec_rows`` [R, P2] (compute dtype,
    on the device): the joint evaluated on an all-zero encoder row, ``tanh(act(d W1d^T + b1)) W2^T + b2``, by the kernels
    the frame-synchronous search's step uses for this model (csrc/ilm_score.hip).  The raw kernel call behind
    ``Transducer.ilm_logprobs`` and what ``sync_beam_search*(ilm_weight=)`` subtracts (there as a log-softmax over the
    non-blank symbols)."""
    _lib.require_cuda(dec_rows)
    net = _SearchNet(model, dec_rows.dtype)
    if dec_rows.dim() != 2 or dec_rows.shape[1] != net.P2:
        raise ValueError("ilm_logits: dec_rows must be [R, P2=%d]" % net.P2)
    dec_rows = dec_rows.contiguous()
    R = dec_rows.shape[0]
    out = torch.empty(R, net.V, dtype=torch.float32, device=dec_rows.device)
    if R == 0:
        return out
    lib = _lib.load()
    cdc = dtype_code(dec_rows.dtype)
    ws = torch.empty(lib.edgedict_ilm_workspace_bytes(cdc, R, net.J), dtype=torch.uint8, device=dec_rows.device)
    w1d = net.w1c[:, net.w1c.shape[1] - net.P2:]
    rc = lib.edgedict_ilm_logits(cdc, _lib.ptr(dec_rows), R, net.P2, net.J, _lib.ptr(w1d),
                                 ctypes.c_longlong(net.w1c.stride(0)), _lib.ptr(net.b1), _lib.ptr(net.w2c),
                                 _lib.ptr(net.b2), net.V, dtype_code(net.emb.dtype), net.E, net.H, _lib.ptr(out),
                                 _lib.ptr(ws), _lib.stream_ptr())
    _lib.check(rc, "ilm_logits")
    return out


def ilm_logprobs(model, ys, ylen):
    """``Transducer.ilm_logprobs``: fp32 [B, U] on the device, nothing read back."""
    dev = model.decoder.embed.weight.device
    ys = torch.as_tensor(ys)
    if ys.dim() != 2:
        raise ValueError("ilm_logprobs: ys must be [B, U] token ids")
    B, U = ys.shape
    ylen = torch.as_tensor(ylen)
    if ylen.shape != (B,):
        raise ValueError("ilm_logprobs: ylen must be [B]")
    out = torch.zeros(B, U, dtype=torch.float32, device=dev)
    if B == 0 or U == 0:
        return out
    tgt = ys.to(device=dev, dtype=torch.int32).contiguous()
    yl = ylen.to(device=dev, dtype=torch.int32).contiguous()
    h_dec, _ = model.decoder(tgt)                       # BOS in front: row u is the network's output after y_<u
    logits = ilm_logits(model, h_dec[:, :U].reshape(B * U, -1))
    rc = _lib.load().edgedict_ilm_logprobs(_lib.ptr(logits), _lib.ptr(tgt), _lib.ptr(yl), B, U, logits.shape[1],
                                           int(model.blank), _lib.ptr(out), _lib.stream_ptr())
    _lib.check(rc, "ilm_logprobs")
    return out


def _sync_encode(model, xs, xlen, W):
    """The argument rules of the ``sync_beam_search*`` entry points, then the encoder: (enc_out, lens)."""
    _check_sync_width(W)
    _lib.require_cuda(xs)
    enc_out, _ = model.encoder(xs)
    enc_out = enc_out.contiguous()
    if xlen is None:
        return enc_out, None
    xl = xlen.detach().cpu() if torch.is_tensor(xlen) else torch.as_tensor(xlen)
    return enc_out, model.scale_length(enc_out, xl).numpy().astype(np.int32)


def _best_of(results):
    """(seqs, scores) in ``beam_search_batch``'s types from ranked ``NBestResult`` lists: entry 0 of each."""
    seqs = [r.tokens[0] for r in results]
    return seqs, torch.from_numpy(np.array([-r.logp[0] for r in results], dtype=np.float64))


def sync_beam_search(model, xs, xlen=None, W=10):
    """Frame-synchronous beam search ("modified beam search"; csrc/decode_sync.hip): every hypothesis emits at most one
    symbol per frame - the greedy search's rule - so all B x W hypotheses of the batch advance through ONE
    prediction-network step and ONE joint per frame, with a fixed number of launches per frame and no wait for the host
    inside the frame loop.  Hypotheses with the same token sequence are merged by log-add, so a hypothesis' log p sums
    over its alignments inside the beam.  ``1 <= W <= 32``; ``W = 1`` is the greedy search with the blanks removed.

    This is a different algorithm from ``beam_search_batch`` (the reference's best-first search, which may emit several
    symbols per frame and never merges): the two do not return the same hypotheses.  It takes no ``prefix=`` or
    ``max_expansions=``.  Its streaming form is ``StreamingSyncBeamSearch``.  This function is the plain search and keeps
    its signature (no ``lm=``, ``bias=``): LM fusion and biasing are ``sync_beam_search_fusion``, below, the ``_nbest`` /
    ``_enc`` / ``_rows`` forms and ``Transducer.sync_beam_search``, which take the keywords.

    Returns ``(list of int64 arrays (tokens, no blanks), fp64 tensor [B] = -log p)`` of the best hypothesis per
    utterance, in ``beam_search_batch``'s types."""
    return _best_of(sync_beam_search_nbest(model, xs, xlen, W))


def sync_beam_search_fusion(model, xs, xlen=None, W=10, *, lm=None, lm_weight=None, length_bonus=0.0, lm_bos=1,
                            bias=None, skip_blank=None, ilm_weight=None):
    """``sync_beam_search`` with LM shallow fusion and contextual biasing (without either: ``sync_beam_search`` itself,
    launch for launch).

    ``lm`` / ``lm_weight`` / ``length_bonus`` / ``lm_bos``: LM shallow fusion with ``beam_search_batch``'s arguments and
    rules (``lm`` needs ``lm_weight``; an LM of another vocabulary raises ``ValueError``).  Every row carries its LM state
    as it carries the prediction network's and all B x W rows step the LM once per frame (``lm.nlayers + 1`` more
    launches on the fused LM step); a non-blank candidate k of hypothesis i scores
    ``((logp_i + lp_i[k]) + (lm_weight * lp_lm_i[k] + length_bonus)) + D(s_i, k)`` in fp64, blank ``logp_i + lp_i[blank]``.
    ``bias``: a contextual-biasing list (``edgedict_amd.bias.ContextGraph``); ``D(s, k) = held[goto(s, k)] - pend[s]`` is
    its increment from the row's automaton state, so a partial match that breaks gives its bonus back, and nothing is
    settled at the end of an utterance (as in ``beam_search_batch`` and ``ContextGraph.score``).  Selection, merging and
    ranking act on the fused score, which is what the returned score is; ``lm_weight = 0, length_bonus = 0`` and an
    empty list are bit-equal to the plain search, and without ``lm`` / ``bias`` the plain kernels run.

    ``skip_blank``: a threshold in (0, 1] - the search then runs only on the encoder frames whose CTC blank posterior
    is at most the threshold (``skip_blank_frames``; the model needs a CTC head).  None: nothing of this runs.

    ``lm`` may also be an ``edgedict_amd.ngram.NGramLM``, a back-off n-gram in device tables (one LM at a time; the type
    dispatches).  A row then carries one integer n-gram state - the state AFTER its tokens, the table's ``start`` (the
    context ``(BOS)``) for the empty sequence; ``lm_bos`` is not read - and the LM term of a non-blank candidate is
    ``lm_weight * step(s_i, k) + length_bonus`` in fp64, bit-equal to ``NGramLM.step`` on the host.  No LM step runs: the
    per-row top-W kernel builds the row's n-gram image in LDS, so a frame keeps the plain search's launches.  Rules
    (``ngram.check_ngram_args``, ``ValueError`` before anything is launched): ``lm_weight`` required, finite and
    ``>= 0``; ``length_bonus`` finite; the n-gram's vocabulary and blank equal to the transducer's; at most
    ``ngram.SYNC_NGRAM_MAX_V`` = 5376 symbols (the image has to fit 64 KiB of LDS).  ``NBestResult.lm_logp`` is not
    filled by the search (``lm_rescore`` does that).

    ``ilm_weight``: internal-LM estimation (ILME; a finite number ``>= 0``, with or without ``lm`` / ``bias``).  The
    transducer's prediction network and joint hold a language model of the training transcripts; its log-probabilities
    ``lp_ilm_i`` - the log-softmax over the NON-BLANK symbols of the joint evaluated on an all-zero encoder row - are
    subtracted while an external LM is added: a non-blank candidate scores
    ``(((logp_i + lp_i[k]) + (lm_weight * lp_lm_i[k] + length_bonus)) - ilm_weight * lp_ilm_i[k]) + D(s_i, k)``.
    ``Transducer.ilm_score`` gives the internal LM's score of a text, to choose the weight by.  No launch more per frame
    on the fused step, two more on the composed one.  ``ilm_weight=0.0`` runs the ILME kernels and is bit-equal to the
    call without it; None (the default) launches exactly the kernels of the call without it.

    Returns ``(list of int64 arrays (tokens, no blanks), fp64 tensor [B] = -log p)`` of the best hypothesis per
    utterance, in ``beam_search_batch``'s types."""
    return _best_of(sync_beam_search_nbest(model, xs, xlen, W, lm=lm, lm_weight=lm_weight, length_bonus=length_bonus,
                                           lm_bos=lm_bos, bias=bias, skip_blank=skip_blank, ilm_weight=ilm_weight))


def sync_beam_search_nbest(model, xs, xlen=None, W=10, *, lm=None, lm_weight=None, length_bonus=0.0, lm_bos=1,
                           bias=None, skip_blank=None, ctc_rescore=None, ilm_weight=None):
    """``sync_beam_search`` returning, per utterance, the final beam as an ``NBestResult`` **already ranked**: ``logp``
    descending (ties keep beam order), at most W hypotheses with distinct token sequences, entry 0 what
    ``sync_beam_search`` returns.  ``frames[i]``: the encoder frame on which each token's tree node was created
    (``emission_times`` applies); ``token_logp[i]``: the token's log-softmax value on that frame - NOT an increment of
    ``logp``, which sums over alignments (as in ``ctc_beam_search``), and with an LM or a bias list still the RNN-T
    value alone while ``logp`` is the fused score.  An utterance of 0 frames yields one empty hypothesis with ``logp`` 0.
    ``skip_blank``: as in ``sync_beam_search_fusion``; ``frames`` stay in the original frame numbering, and an utterance
    whose frames are all dropped is an utterance of 0 frames.  ``ctc_rescore``: a weight ``>= 0`` - the ranked list
    then goes through ``ctc_rescore`` (the module-level function; on the unskipped encoder output) before it is
    returned: ``ctc_logp`` filled, ``logp`` the combined score, ranked by it.  None: nothing of this runs.
    ``ilm_weight``: internal-LM estimation, as in ``sync_beam_search_fusion``."""
    _check_sync_fusion(model, lm, lm_weight, bias, length_bonus)
    _check_ilm_weight(ilm_weight)
    if skip_blank is not None:
        _check_skip(model, skip_blank)
    if ctc_rescore is not None:
        _check_rescore(model, ctc_rescore)
    enc_out, lens = _sync_encode(model, xs, xlen, W)
    if skip_blank is not None:
        sk = skip_blank_frames(model, enc_out, lens, skip_blank)
        return _rescored(model, enc_out, lens,
                         sk.restore(sync_beam_search_nbest_enc(model, sk.enc_out, sk.lens, W, lm=lm,
                                                               lm_weight=lm_weight, length_bonus=length_bonus,
                                                               lm_bos=lm_bos, bias=bias, ilm_weight=ilm_weight)),
                         ctc_rescore)
    return sync_beam_search_nbest_enc(model, enc_out, lens, W, lm=lm, lm_weight=lm_weight, length_bonus=length_bonus,
                                      lm_bos=lm_bos, bias=bias, ctc_rescore=ctc_rescore, ilm_weight=ilm_weight)


def sync_beam_search_enc(model, enc_out, lens=None, W=10,
                         *, lm=None, lm_weight=None, length_bonus=0.0, lm_bos=1, bias=None, ilm_weight=None):
    """``sync_beam_search`` over a given encoder output ``enc_out`` [B, T, P] (compute dtype) with ``lens`` (host int,
    encoder frames per utterance; None: all T)."""
    return _best_of(sync_beam_search_nbest_enc(model, enc_out, lens, W, lm=lm, lm_weight=lm_weight,
                                               length_bonus=length_bonus, lm_bos=lm_bos, bias=bias,
                                               ilm_weight=ilm_weight))


def sync_beam_search_nbest_enc(model, enc_out, lens=None, W=10, *, lm=None, lm_weight=None, length_bonus=0.0, lm_bos=1,
                               bias=None, ctc_rescore=None, ilm_weight=None):
    """``sync_beam_search_nbest`` over a given encoder output, as ``sync_beam_search_enc``.  ``ctc_rescore``: as there,
    the head scoring this ``enc_out``."""
    _check_sync_fusion(model, lm, lm_weight, bias, length_bonus)
    _check_ilm_weight(ilm_weight)
    _check_sync_width(W)
    if ctc_rescore is not None:
        _check_rescore(model, ctc_rescore)
    _lib.require_cuda(enc_out)
    enc_out = enc_out.contiguous()
    B, T, P = enc_out.shape
    return _rescored(model, enc_out, lens,
                     sync_beam_search_nbest_rows(model, joint_rows(model, enc_out), B, T, P, lens, W, lm=lm,
                                                 lm_weight=lm_weight, length_bonus=length_bonus, lm_bos=lm_bos,
                                                 bias=bias, ilm_weight=ilm_weight), ctc_rescore)


def sync_beam_search_rows(model, E1, B, T, P, lens=None, W=10,
                          *, lm=None, lm_weight=None, length_bonus=0.0, lm_bos=1, bias=None, ilm_weight=None):
    """``sync_beam_search_enc`` from the joint's encoder rows ``E1`` [B * T, J] (``joint_rows``) of an encoder output of
    width P."""
    return _best_of(sync_beam_search_nbest_rows(model, E1, B, T, P, lens, W, lm=lm, lm_weight=lm_weight,
                                                length_bonus=length_bonus, lm_bos=lm_bos, bias=bias,
                                                ilm_weight=ilm_weight))


def sync_beam_search_nbest_rows(model, E1, B, T, P, lens=None, W=10, max_tokens=None,
                                *, lm=None, lm_weight=None, length_bonus=0.0, lm_bos=1, bias=None, ilm_weight=None):
    """``sync_beam_search_nbest_enc`` from the joint's encoder rows, as ``sync_beam_search_rows``.  ``max_tokens``
    bounds a hypothesis' length (default T: one token per frame at most); a longer one raises, it is never cut."""
    from .bias import active
    _check_sync_fusion(model, lm, lm_weight, bias, length_bonus)
    ilm = _check_ilm_weight(ilm_weight)
    _check_sync_width(W)
    _lib.require_cuda(E1)
    W = int(W)
    cd = E1.dtype
    lens = np.full(B, T, dtype=np.int32) if lens is None else np.ascontiguousarray(lens, dtype=np.int32)
    if lens.shape != (B,) or (lens < 0).any() or (lens > T).any():
        raise ValueError("sync_beam_search: lens must be [B] ints in [0, %d]" % T)
    if T < 1:       # nothing to search: the empty hypothesis (the native call refuses T <= 0)
        return [NBestResult([np.zeros(0, np.int64)], [np.zeros(0, np.int32)], [np.zeros(0)], [0.0]) for _ in range(B)]
    net = _SearchNet(model, cd)
    lib = _lib.load()
    MT = T if max_tokens is None else int(max_tokens)
    dev = E1.device
    flm, ng = _sync_lm_opts(lm, cd, dev, lm_weight, length_bonus, lm_bos)
    bref = active(bias).ref(dev) if active(bias) is not None else None
    nref, opts = net.ref(P), _opts(flm, bref, ilm, ng)      # (no feature: a null opts, the plain search)
    nbytes = lib.edgedict_sync_beam_workspace_bytes(nref, B, T, W, opts)
    if opts is not None and nbytes == 0:
        raise ValueError("sync_beam_search: shapes out of range (the LM's hidden width must be a multiple of 4)")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    result = torch.empty(lib.edgedict_sync_beam_result_bytes(B, W, MT), dtype=torch.uint8, device=dev)
    tokens = np.empty((B, W, MT), dtype=np.int32)       # (only the used columns are written and read)
    frames = np.empty((B, W, MT), dtype=np.int32)
    tlogp = np.empty((B, W, MT), dtype=np.float64)
    ntok = np.zeros((B, W), dtype=np.int32)
    nhyp = np.zeros(B, dtype=np.int32)
    logp = np.zeros((B, W), dtype=np.float64)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = lib.edgedict_sync_beam_search(
        nref, _lib.ptr(E1), ctypes.c_longlong(T * net.J), ctypes.c_longlong(net.J), B, T, vp(lens), W, vp(tokens),
        vp(frames), vp(tlogp), MT, vp(ntok), vp(nhyp), vp(logp), opts, _lib.ptr(ws), _lib.ptr(result), _lib.stream_ptr())
    _lib.check(rc, "sync_beam_search")
    return _nbest_results(tokens, frames, tlogp, ntok, nhyp, logp)


def ctc_beam_search(model, xs, xlen, W=10, cand=None, bias=None, *, lm=None, lm_weight=None, length_bonus=0.0):
    """First-pass N-best from the encoder alone: encoder, CTC head, ``loss.ctc_prefix_beam`` (the CTC prefix beam search
    of csrc/ctc_decode.hip), then ONE read to the host - neither the prediction network nor the joint runs.  Returns a
    list of ``NBestResult``, one per utterance, already ranked: ``logp`` is descending and entry 0 is the answer.

    ``tokens[i]`` / ``frames[i]``: the prefix and the encoder frame on which each token's node was created (the first
    frame the prefix could end on), so ``emission_times`` applies.  ``token_logp[i]``: the log-softmax value of each
    token on that frame.  Unlike in the RNN-T searches ``token_logp`` is NOT an increment of ``logp``: CTC sums over all
    paths of a prefix, so ``logp[i]`` is not the sum of per-token terms.  With ``bias`` (an
    ``edgedict_amd.bias.ContextGraph``) ``logp`` includes the prefix' bias total ``bias.score(tokens)``; a frame's
    candidate list (``cand``, default ``min(V - 1, 32)``) is cut before the bias is seen, so a boosted token outside it
    is not rescued.  ``lm`` / ``lm_weight`` / ``length_bonus``: an ``edgedict_amd.ngram.NGramLM`` fused into the search
    (``loss.ctc_prefix_beam``); ``logp`` then includes the prefix' LM total as well.  Raises ``RuntimeError`` on a model
    built without ``ctc_weight > 0``, as ``ctc_greedy_decode``."""
    from .loss import ctc_prefix_beam
    from .ngram import check_ngram_args
    check_ngram_args(lm, lm_weight, length_bonus)
    if getattr(model, "ctc_head", None) is None:
        raise RuntimeError("this model has no CTC head: construct it with Transducer(..., ctc_weight > 0)")
    _lib.require_cuda(xs)
    with torch.no_grad():
        xs = xs[:, :xlen.max()].contiguous()
        h_enc, _ = model.encoder(xs)
        act = model.scale_length(h_enc, xlen).to(device=h_enc.device, dtype=torch.int32).contiguous()
        out = ctc_prefix_beam(model._ctc_logits(h_enc).contiguous(), act, W, model.blank, cand, bias, lm=lm,
                              lm_weight=lm_weight, length_bonus=length_bonus)
        B, Wn, T = out[0].shape
        # one read: the int32 fields and token_lp as raw bits in one buffer, logp beside them
        packed = torch.cat([out[0].reshape(B, -1), out[1].reshape(B, -1), out[2].view(torch.int32).reshape(B, -1),
                            out[3], out[4].reshape(B, 1), out[5].view(torch.int32).reshape(B, -1)], dim=1).cpu().numpy()
    n = Wn * T
    tokens = packed[:, :n].reshape(B, Wn, T)
    frames = packed[:, n:2 * n].reshape(B, Wn, T)
    tlp = np.ascontiguousarray(packed[:, 2 * n:3 * n]).view(np.float32).reshape(B, Wn, T).astype(np.float64)
    ntok = packed[:, 3 * n:3 * n + Wn]
    nhyp = packed[:, 3 * n + Wn]
    logp = np.ascontiguousarray(packed[:, 3 * n + Wn + 1:]).view(np.float64).reshape(B, Wn)
    return _nbest_results(tokens, frames, tlp, ntok, nhyp, logp)


class StreamingBeamSearch:
    """The beam search of ``beam_search_batch`` for S streams whose encoder output arrives chunk by chunk.

    The reference's search is frame-synchronous: all it carries from frame to frame is the list B (at most W
    hypotheses with their log-probability, last token, prediction-network state and token sequence).  That list lives in
    a persistent device state (csrc/decode.hip, ``edgedict_beam_stream_*``), so ``advance`` over frames [0, t1) and
    then [t1, t2) gives exactly what ``beam_search_enc`` over [0, t2) gives, and ``best()`` after any chunk is what the
    offline search would return if the audio ended there.  After every advance each stream's token tree is compacted:
    the tokens down to the survivors' lowest common ancestor are committed (they can no longer change) and move to a
    host-side log, so the device tree stays bounded by ``node_capacity`` however long a stream runs.

    ``prefix=True`` (the reference's prefix-sum merge, models.py:145-161) is not supported: it would need the
    prediction stored per token-tree node to survive compaction; asking for it raises ``ValueError``.

    ``node_capacity`` bounds the token tree per stream: an advance whose streams could need more (live nodes +
    frames x max_expansions) raises ``RuntimeError`` before it runs; it never truncates.  The default leaves room for
    chunks of 32 frames on top of the live tree.

    ``lm`` / ``lm_weight`` / ``length_bonus`` / ``lm_bos``: LM shallow fusion as in ``beam_search_batch`` (module
    docstring).  The survivors' LM states are carried in the device state beside the prediction network's; the LM's
    root token is ``lm_bos`` until a stream has committed a token, then its last committed token.

    ``detail=True`` keeps, per token, the encoder frame it was emitted on (counted since the stream's reset) and its
    score increment, through compaction and in the committed log: ``nbest()`` then returns the whole list B as
    ``NBestResult`` objects and ``committed_detail()`` the committed log with frames and increments.  Without it both
    raise; ``best()``, ``committed()`` and ``expansions()`` are the same either way.

    ``bias``: a contextual-biasing list (``edgedict_amd.bias.ContextGraph``, module docstring) shared by all streams.
    The survivors' automaton states are carried in the device state; the automaton reads a stream's root token as the
    prediction network does, so commits change nothing.  ``set_bias`` swaps the list between utterances.  A search
    built without a list (or with an empty one) runs the plain kernels until ``set_bias`` gives it one.
    """

    def __init__(self, model, n_streams, W=10, max_expansions=None, node_capacity=None, prefix=False, *, lm=None,
                 lm_weight=None, length_bonus=0.0, lm_bos=1, detail=False, bias=None):
        from .bias import active, check_bias_args
        from .lm import check_fusion_args
        check_fusion_args(lm, lm_weight, _vocab(model), prefix)
        check_bias_args(bias, _vocab(model), prefix)
        if prefix:
            raise ValueError("StreamingBeamSearch: prefix=True (the prefix-sum merge) is not supported when streaming")
        if W < 1:
            raise ValueError("beam width must be >= 1")
        if n_streams < 1:
            raise ValueError("n_streams must be >= 1")
        self.model = model
        self.S = int(n_streams)
        self.W = int(W)
        self.EM = int(max_expansions) if max_expansions else max(16, 8 * self.W)
        self.NC = int(node_capacity) if node_capacity else 32 * self.EM + 1024
        from .stream import _compute_dtype
        self.cd = _compute_dtype(model)
        self.device = model.decoder.embed.weight.device
        self.lm = lm
        self._lm_args = (lm_weight, length_bonus, lm_bos)
        self.bias = active(bias)
        self._frames = np.zeros(self.S, dtype=np.int64)      # frames per stream since its reset
        self._alloc()
        self._commit_buf = np.zeros((self.S, self.NC), dtype=np.int32)
        self._ncommit = np.zeros(self.S, dtype=np.int32)
        self.detail = bool(detail)
        if self.detail:
            lib = _lib.load()
            self._dstate = torch.empty(lib.edgedict_beam_stream_detail_state_bytes(self.S, self.NC), dtype=torch.uint8,
                                       device=self.device)
            self._dws = torch.empty(lib.edgedict_beam_stream_detail_workspace_bytes(self.S, self.NC), dtype=torch.uint8,
                                    device=self.device)
            self._commit_frame_buf = np.zeros((self.S, self.NC), dtype=np.int32)
            self._commit_logp_buf = np.zeros((self.S, self.NC), dtype=np.float64)
            self._result = None
        self.last_expansions = 0
        self.reset()

    def _alloc(self):
        """The persistent state and the workspace, sized for the current forms (LM, bias list)."""
        net, lib, opts = self._weights(), _lib.load(), self._opts()
        sbytes = lib.edgedict_beam_stream_state_bytes(opts, self.S, net.L, net.H, self.W, self.NC)
        wbytes = lib.edgedict_beam_stream_workspace_bytes(net.ref(), self.S, self.W, self.EM, self.NC, opts)
        self._state = torch.empty(sbytes, dtype=torch.uint8, device=self.device)
        self._ws = torch.empty(wbytes, dtype=torch.uint8, device=self.device)

    def _bref(self):
        if self.bias is None:
            return None
        _lib.require_cuda(self.model.decoder.embed.weight)
        return self.bias.ref(self.device)

    def set_bias(self, graph, mask=None):
        """Swap the bias list (a ``ContextGraph``, or None / an empty one for "no bias").  The list is shared by all
        streams of the search and the survivors of a stream in mid-utterance hold states of the old automaton, so EVERY
        stream must be fresh - no frames since its reset - or ``ValueError`` is raised.  ``mask`` (None: all) only
        names the streams the caller swaps the list for: a stream in it that has frames is reported as such, one
        outside it as being in the middle of an utterance.  Nothing is launched; the next ``advance`` reads the new
        tables."""
        from .bias import active, check_bias_args
        check_bias_args(graph, _vocab(self.model), False)
        if mask is None:
            sel = np.ones(self.S, dtype=bool)
        else:
            m = mask.detach().cpu().numpy() if torch.is_tensor(mask) else np.asarray(mask)
            sel = m.astype(bool).reshape(self.S)
        busy = np.nonzero(self._frames > 0)[0]
        for s in busy:
            if sel[s]:
                raise ValueError("set_bias: stream %d has advanced over %d frames since its reset (reset it first)"
                                 % (s, self._frames[s]))
        if len(busy):
            raise ValueError("set_bias: the bias list is shared by all streams and stream %d, outside the mask, is in "
                             "the middle of an utterance" % busy[0])
        had = self.bias is not None
        self.bias = active(graph)
        if had != (self.bias is not None):
            # the state gains / loses the survivors' automaton states: every stream is fresh, so a new state, reset
            # (the committed logs are empty), is the old one
            self._alloc()
            self.reset()

    def _weights(self):
        # converted once per parameter version by WEIGHTS (as run_search does); only the pointer bundle is rebuilt
        return _SearchNet(self.model, self.cd)

    def _opts(self):
        from .lm import FusionLM
        return _opts(None if self.lm is None else FusionLM(self.lm, self.cd, *self._lm_args), self._bref())

    def reset(self, mask=None):
        """Every stream, or those where ``mask[s]`` is true, back to the empty hypothesis with an empty committed log."""
        from .tokenizer import BOS
        net = self._weights()
        if mask is None:
            sel = np.ones(self.S, dtype=bool)
            mh, on_host = None, 0
        else:
            m = mask.detach().cpu().numpy() if torch.is_tensor(mask) else np.asarray(mask)
            sel = m.astype(bool).reshape(self.S)
            mh, on_host = np.ascontiguousarray(sel, dtype=np.int32), 1
        mp = None if mh is None else mh.ctypes.data_as(ctypes.c_void_p)
        rc = _lib.load().edgedict_beam_stream_reset(
            self._opts(), self.S, net.L, net.H, self.W, self.NC, int(BOS), mp, on_host, _lib.ptr(self._state),
            _lib.ptr(self._dstate) if self.detail else None, _lib.stream_ptr())
        _lib.check(rc, "beam_stream_reset")
        if not hasattr(self, "_committed"):
            self._committed = [[] for _ in range(self.S)]
            self._committed_frames = [[] for _ in range(self.S)]
            self._committed_logp = [[] for _ in range(self.S)]
        self._frames[sel] = 0
        for s in np.nonzero(sel)[0]:
            self._committed[s] = []
            self._committed_frames[s] = []
            self._committed_logp[s] = []

    def joint_rows(self, enc_out):
        """The rows ``advance`` reads for ``enc_out`` [S, T, P]: see ``joint_rows``."""
        return self._weights().e1(enc_out)

    def advance(self, enc_out, n_frames=None):
        """Advance every stream over the first ``n_frames[s]`` frames (host ints, default all T; 0: the stream sits
        this chunk out) of ``enc_out`` [S, T, P] (compute dtype, on the device)."""
        _lib.require_cuda(enc_out)
        if enc_out.dim() != 3 or enc_out.shape[0] != self.S:
            raise ValueError("advance: enc_out must be [S=%d, T, P]" % self.S)
        if enc_out.dtype != self.cd:
            raise TypeError("advance: enc_out is %s, the model computes in %s" % (enc_out.dtype, self.cd))
        enc_out = enc_out.contiguous()
        S, T, P = enc_out.shape
        if n_frames is None:
            nf = np.full(S, T, dtype=np.int32)
        else:
            nf = np.ascontiguousarray(n_frames.cpu().numpy() if torch.is_tensor(n_frames) else n_frames, dtype=np.int32)
            if nf.shape != (S,) or (nf < 0).any() or (nf > T).any():
                raise ValueError("advance: n_frames must be [S] ints in [0, %d]" % T)
        net = self._weights()
        self._advance(net, net.e1(enc_out), T, P, nf)

    def advance_rows(self, E1, P, n_frames=None):
        """``advance`` from the joint's encoder rows ``E1`` [S * T, J] (``joint_rows``) of an encoder output of width
        P: what ``advance`` runs after its first product."""
        _lib.require_cuda(E1)
        net = self._weights()
        if E1.dim() != 2 or E1.shape[1] != net.J or E1.shape[0] % self.S or not E1.is_contiguous():
            raise ValueError("advance_rows: E1 must be contiguous [S * T, J=%d]" % net.J)
        if E1.dtype != self.cd:
            raise TypeError("advance_rows: E1 is %s, the model computes in %s" % (E1.dtype, self.cd))
        T = E1.shape[0] // self.S
        nf = np.full(self.S, T, dtype=np.int32) if n_frames is None else np.ascontiguousarray(n_frames, dtype=np.int32)
        if nf.shape != (self.S,) or (nf < 0).any() or (nf > T).any():
            raise ValueError("advance_rows: n_frames must be [S] ints in [0, %d]" % T)
        self._advance(net, E1, T, P, nf)

    def _advance(self, net, E1, T, P, nf):
        nexp = ctypes.c_longlong(0)
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        detail = ((_lib.ptr(self._dstate), _lib.ptr(self._dws), vp(self._commit_frame_buf), vp(self._commit_logp_buf))
                  if self.detail else (None,) * 4)
        rc = _lib.load().edgedict_beam_stream_advance(
            net.ref(P), _lib.ptr(E1), ctypes.c_longlong(T * net.J), ctypes.c_longlong(net.J), self.S, vp(nf), self.W,
            self.EM, self.NC, vp(self._commit_buf), vp(self._ncommit), ctypes.byref(nexp), self._opts(),
            _lib.ptr(self._state), _lib.ptr(self._ws), *detail, _lib.stream_ptr())
        _lib.check(rc, "beam_stream_advance")
        self._frames += nf
        self.last_expansions = int(nexp.value)
        for s in np.nonzero(self._ncommit)[0]:
            self._committed[s].extend(self._commit_buf[s, :self._ncommit[s]].tolist())
            if self.detail:
                self._committed_frames[s].extend(self._commit_frame_buf[s, :self._ncommit[s]].tolist())
                self._committed_logp[s].extend(self._commit_logp_buf[s, :self._ncommit[s]].tolist())

    def _read(self):
        net = self._weights()
        lib = _lib.load()
        max_tokens = self.NC
        tokens = np.zeros((self.S, max_tokens), dtype=np.int32)
        ntok = np.zeros(self.S, dtype=np.int32)
        score = np.zeros(self.S, dtype=np.float64)
        ncom = np.zeros(self.S, dtype=np.int64)
        nexp = np.zeros(self.S, dtype=np.int64)
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        rc = lib.edgedict_beam_stream_read(self.S, net.L, net.H, self.W, self.NC, _lib.ptr(self._state), vp(tokens),
                                           max_tokens, vp(ntok), vp(score), vp(ncom), vp(nexp), _lib.stream_ptr())
        _lib.check(rc, "beam_stream_read")
        for s in range(self.S):
            if ncom[s] != len(self._committed[s]):
                raise RuntimeError("beam_stream_read: stream %d has %d committed tokens on the device, %d in the log"
                                   % (s, ncom[s], len(self._committed[s])))
        return tokens, ntok, score, nexp

    def best(self):
        """Per stream the first hypothesis of the current list B, as ``beam_search_batch`` returns it:
        ``(list of int64 arrays (tokens, no blanks), fp64 tensor [S] = -log p)``."""
        tokens, ntok, score, _ = self._read()
        seqs = [np.concatenate([np.asarray(self._committed[s], dtype=np.int64),
                                tokens[s, :ntok[s]].astype(np.int64)]) for s in range(self.S)]
        return seqs, torch.from_numpy(score)

    def committed(self):
        """Per stream the committed tokens (int64 arrays): a prefix of ``best()`` that no later frame can change."""
        return [np.asarray(c, dtype=np.int64) for c in self._committed]

    def expansions(self):
        """int64 [S]: prediction-network steps (pops) of every stream since its reset."""
        return self._read()[3]

    def _need_detail(self, what):
        if not self.detail:
            raise RuntimeError("StreamingBeamSearch.%s() needs a search built with detail=True" % what)

    def nbest(self):
        """Per stream an ``NBestResult``: the current list B, as ``beam_search_nbest`` over the stream's frames since
        its reset returns it; every hypothesis is the committed log followed by its uncommitted tail, in tokens, frames
        and increments alike.  Needs ``detail=True``."""
        self._need_detail("nbest")
        net = self._weights()
        lib = _lib.load()
        S, W, MT = self.S, self.W, self.NC
        if self._result is None:
            self._result = torch.empty(lib.edgedict_beam_nbest_result_bytes(S, W, MT), dtype=torch.uint8,
                                       device=self.device)
        tokens = np.empty((S, W, MT), dtype=np.int32)
        frames = np.empty((S, W, MT), dtype=np.int32)
        tlogp = np.empty((S, W, MT), dtype=np.float64)
        ntok = np.zeros((S, W), dtype=np.int32)
        nhyp = np.zeros(S, dtype=np.int32)
        logp = np.zeros((S, W), dtype=np.float64)
        ncom = np.zeros(S, dtype=np.int64)
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        rc = lib.edgedict_beam_stream_read_nbest(S, net.L, net.H, W, self.NC, _lib.ptr(self._state),
                                                 _lib.ptr(self._dstate), _lib.ptr(self._result), vp(tokens), vp(frames),
                                                 vp(tlogp), MT, vp(ntok), vp(nhyp), vp(logp), vp(ncom), None, None,
                                                 _lib.stream_ptr())
        _lib.check(rc, "beam_stream_read_nbest")
        for s in range(S):
            if ncom[s] != len(self._committed[s]):
                raise RuntimeError("beam_stream_read_nbest: stream %d has %d committed tokens on the device, %d in the "
                                   "log" % (s, ncom[s], len(self._committed[s])))
        prefix = list(zip(self._committed, self._committed_frames, self._committed_logp))
        return _nbest_results(tokens, frames, tlogp, ntok, nhyp, logp, prefix)

    def committed_detail(self):
        """Per stream ``(tokens int64, frames int32, token_logp float64)`` of the committed log: a prefix of every
        hypothesis of ``nbest()`` that no later frame can change.  Needs ``detail=True``."""
        self._need_detail("committed_detail")
        return [(np.asarray(t, dtype=np.int64), np.asarray(f, dtype=np.int32), np.asarray(l, dtype=np.float64))
                for t, f, l in zip(self._committed, self._committed_frames, self._committed_logp)]


class StreamingSyncBeamSearch:
    """The frame-synchronous beam search of ``sync_beam_search`` for S streams whose encoder output arrives chunk by
    chunk (csrc/decode_sync.hip, ``edgedict_sync_stream_*``).

    Every stream's beam - W rows with their log p, token-tree node, sequence hash, last token and prediction-network
    state - lives in a persistent device state and stays in beam order between chunks, so ``advance`` over frames
    [0, t1) and then [t1, t2) leaves exactly the beam the offline search has after t2 frames: after any chunk ``nbest()``
    is bit for bit what ``sync_beam_search_nbest_rows`` over the stream's frames since its reset returns, and ``best()``
    is its entry 0.  A frame is the offline search's launches (6 + L); nothing inside the frame loop waits for the
    host.  A stream may take fewer frames of a chunk than the others, or none (``n_frames``).

    After the last frame of an advance ONE launch compacts every stream's token tree: the tokens from the root down to
    the lowest common ancestor of the live hypotheses' leaves are committed - no later frame can change them - and move
    to a host-side log with their frames and log-probs, that ancestor becomes the root, and the nodes a live leaf still
    reaches are renumbered densely.  The device tree therefore stays bounded by ``node_capacity`` however long a stream
    runs.  The committed prefix is the TREE's common ancestor, not the longest common token prefix of the beam: a
    sequence that was pruned and later created again has a second chain of nodes, so hypotheses that agree on their
    first tokens can still hold them in different nodes, and those tokens are committed later (or, at the latest, never
    lost: ``nbest()`` always returns whole hypotheses).  Per advance there is one device-to-host read (per stream the
    commit count, the live node count and the committed records) and one stream synchronisation, after the compaction.

    ``node_capacity`` (NC): token-tree nodes per stream.  An advance adds at most ``n_frames[s] * W`` nodes to stream s,
    so one with ``live[s] + n_frames[s] * W > NC`` (``live[s]``: the stream's nodes after the previous advance's
    compaction) raises ``RuntimeError`` before anything is launched and leaves the state as it was; nothing is ever
    truncated.  Default ``NC = 32 * W + 1024``: room for chunks of 32 frames on top of a live tree of 1024 nodes.

    ``1 <= W <= 32``.  The constructor keeps the plain search's signature: there is no ``lm=``, ``bias=``, ``prefix=``
    or ``max_expansions=`` here.  LM shallow fusion and contextual biasing are ``StreamingSyncFusionBeamSearch``, the
    same class with a wider constructor; ``set_bias`` gives a search built here a bias list between utterances.
    A stream with no frames since its reset holds one empty hypothesis with ``logp`` 0."""

    _EMPTY = (np.zeros(0, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float64))

    def __init__(self, model, n_streams, W=10, node_capacity=None):
        self._setup(model, n_streams, W, node_capacity)

    def _setup(self, model, n_streams, W, node_capacity, lm=None, lm_weight=None, length_bonus=0.0, lm_bos=1, bias=None,
               ilm_weight=None):
        from .bias import active
        _check_sync_fusion(model, lm, lm_weight, bias, length_bonus)
        self._ilm = _check_ilm_weight(ilm_weight)       # None, or the weight as the c_double the advance points at
        _check_sync_width(W)
        if n_streams < 1:
            raise ValueError("n_streams must be >= 1")
        self.model = model
        self.S = int(n_streams)
        self.W = int(W)
        self.NC = int(node_capacity) if node_capacity else 32 * self.W + 1024
        if self.NC < self.W:
            raise ValueError("node_capacity = %d is below W = %d: not even one frame fits" % (self.NC, self.W))
        _lib.require_cuda(model.decoder.embed.weight)
        from .stream import _compute_dtype
        self.cd = _compute_dtype(model)
        self.device = model.decoder.embed.weight.device
        self.lm = lm
        self._lm_args = (lm_weight, length_bonus, lm_bos)
        self.bias = active(bias)
        self._alloc()
        self._result, self._result_mt = None, -1
        self._live = np.zeros(self.S, dtype=np.int32)        # token-tree nodes per stream after the last compaction
        self._parity = ctypes.c_int32(0)                     # which state buffer the next frame reads
        self._frames = np.zeros(self.S, dtype=np.int64)      # frames per stream since its reset
        self._ncommitted = np.zeros(self.S, dtype=np.int64)  # tokens in its committed log
        # the advance's read: [S][1 + NC] records {int32, int32, float32, int32}; record 0 = (commits, live nodes)
        self._commit_buf = np.zeros((self.S, self.NC + 1, 4), dtype=np.int32)
        # the committed log per stream, as arrays: (tokens int64, frames int32, token_logp float64)
        self._committed = [self._EMPTY[0]] * self.S
        self._committed_frames = [self._EMPTY[1]] * self.S
        self._committed_logp = [self._EMPTY[2]] * self.S
        self.reset()

    def _weights(self):
        return _SearchNet(self.model, self.cd)

    def _opts(self):
        """The ``opts`` of this search's native calls (None: the plain search)."""
        flm, ng = _sync_lm_opts(self.lm, self.cd, self.device, *self._lm_args)
        return _opts(flm, None if self.bias is None else self.bias.ref(self.device), self._ilm, ng)

    def _alloc(self):
        """The persistent state and the workspace, sized for the current forms (LM, bias list)."""
        net, lib, opts = self._weights(), _lib.load(), self._opts()
        sbytes = lib.edgedict_sync_stream_state_bytes(opts, self.S, net.L, net.H, self.W, self.NC)  # (no ILME part)
        wbytes = lib.edgedict_sync_stream_workspace_bytes(net.ref(), self.S, self.W, self.NC, opts)
        if sbytes == 0 or wbytes == 0:
            raise ValueError("StreamingSyncBeamSearch: shapes out of range (H and the LM's hidden width must be "
                             "multiples of 4)")
        self._state = torch.empty(sbytes, dtype=torch.uint8, device=self.device)
        self._ws = torch.empty(wbytes, dtype=torch.uint8, device=self.device)

    def set_bias(self, graph, mask=None):
        """Swap the bias list (a ``ContextGraph``, or None / an empty one for "no bias"), with
        ``StreamingBeamSearch.set_bias``'s rules: the list is shared by all streams and the rows of a stream in
        mid-utterance hold states of the old automaton, so EVERY stream must be fresh - no frames since its reset - or
        ``ValueError`` is raised.  ``mask`` (None: all) only names the streams the caller swaps the list for: a stream in
        it that has frames is reported as such, one outside it as being in the middle of an utterance.  Nothing is
        launched when the state keeps its size (a fresh stream stands on state 0, the root of every automaton) and the
        next ``advance`` reads the new tables; where the gain or loss of a list changes the state's size, the state is
        allocated anew and reset."""
        from .bias import active, check_bias_args
        check_bias_args(graph, _vocab(self.model), False)
        if mask is None:
            sel = np.ones(self.S, dtype=bool)
        else:
            m = mask.detach().cpu().numpy() if torch.is_tensor(mask) else np.asarray(mask)
            sel = m.astype(bool).reshape(self.S)
        busy = np.nonzero(self._frames > 0)[0]
        for s in busy:
            if sel[s]:
                raise ValueError("set_bias: stream %d has advanced over %d frames since its reset (reset it first)"
                                 % (s, self._frames[s]))
        if len(busy):
            raise ValueError("set_bias: the bias list is shared by all streams and stream %d, outside the mask, is in "
                             "the middle of an utterance" % busy[0])
        had = self.bias is not None
        self.bias = active(graph)
        if had != (self.bias is not None):
            self._alloc()
            self._parity = ctypes.c_int32(0)
            self.reset()

    def reset(self, mask=None):
        """Every stream, or those where ``mask[s]`` is true, back to the empty hypothesis with an empty committed log;
        its frames count from 0 again."""
        from .tokenizer import BOS
        net = self._weights()
        if mask is None:
            sel = np.ones(self.S, dtype=bool)
            mp, on_host = None, 0
        else:
            m = mask.detach().cpu().numpy() if torch.is_tensor(mask) else np.asarray(mask)
            sel = m.astype(bool).reshape(self.S)
            mh, on_host = np.ascontiguousarray(sel, dtype=np.int32), 1
            mp = mh.ctypes.data_as(ctypes.c_void_p)
        rc = _lib.load().edgedict_sync_stream_reset(self._opts(), self.S, net.L, net.H, self.W, self.NC, int(BOS), mp,
                                                    on_host, _lib.ptr(self._state), _lib.stream_ptr())
        _lib.check(rc, "sync_stream_reset")
        self._frames[sel] = 0
        self._live[sel] = 0
        self._ncommitted[sel] = 0
        for s in np.nonzero(sel)[0]:
            self._committed[s], self._committed_frames[s], self._committed_logp[s] = self._EMPTY

    def joint_rows(self, enc_out):
        """The rows ``advance`` reads for ``enc_out`` [S, T, P]: see ``joint_rows``."""
        return self._weights().e1(enc_out)

    def _n_frames(self, what, n_frames, T):
        if n_frames is None:
            return np.full(self.S, T, dtype=np.int32)
        nf = np.ascontiguousarray(n_frames.cpu().numpy() if torch.is_tensor(n_frames) else n_frames, dtype=np.int32)
        if nf.shape != (self.S,) or (nf < 0).any() or (nf > T).any():
            raise ValueError("%s: n_frames must be [S] ints in [0, %d]" % (what, T))
        return nf

    def advance(self, enc_out, n_frames=None):
        """Advance every stream over the first ``n_frames[s]`` frames (host ints, default all T; 0: the stream sits
        this chunk out) of ``enc_out`` [S, T, P] (compute dtype, on the device)."""
        _lib.require_cuda(enc_out)
        if enc_out.dim() != 3 or enc_out.shape[0] != self.S:
            raise ValueError("advance: enc_out must be [S=%d, T, P]" % self.S)
        if enc_out.dtype != self.cd:
            raise TypeError("advance: enc_out is %s, the model computes in %s" % (enc_out.dtype, self.cd))
        enc_out = enc_out.contiguous()
        S, T, P = enc_out.shape
        nf = self._n_frames("advance", n_frames, T)
        net = self._weights()
        self._advance(net, net.e1(enc_out), T, P, nf)

    def advance_rows(self, E1, P, n_frames=None):
        """``advance`` from the joint's encoder rows ``E1`` [S * T, J] (``joint_rows``) of an encoder output of width
        P: what ``advance`` runs after its first product."""
        _lib.require_cuda(E1)
        net = self._weights()
        if E1.dim() != 2 or E1.shape[1] != net.J or E1.shape[0] % self.S or not E1.is_contiguous():
            raise ValueError("advance_rows: E1 must be contiguous [S * T, J=%d]" % net.J)
        if E1.dtype != self.cd:
            raise TypeError("advance_rows: E1 is %s, the model computes in %s" % (E1.dtype, self.cd))
        T = E1.shape[0] // self.S
        self._advance(net, E1, T, P, self._n_frames("advance_rows", n_frames, T))

    def _advance(self, net, E1, T, P, nf):
        need = self._live.astype(np.int64) + nf.astype(np.int64) * self.W
        if (need > self.NC).any():
            s = int(np.argmax(need > self.NC))
            raise RuntimeError("StreamingSyncBeamSearch: stream %d may need %d token-tree nodes (%d live + %d frames x "
                               "W = %d), node_capacity is %d" % (s, need[s], self._live[s], nf[s], self.W, self.NC))
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        rc = _lib.load().edgedict_sync_stream_advance(
            net.ref(P), _lib.ptr(E1), ctypes.c_longlong(T * net.J), ctypes.c_longlong(net.J), self.S, T, vp(nf), self.W,
            self.NC, vp(self._live), ctypes.byref(self._parity), vp(self._commit_buf), self.NC, self._opts(),
            _lib.ptr(self._state), _lib.ptr(self._ws), _lib.stream_ptr())
        _lib.check(rc, "sync_stream_advance")
        self._frames += nf
        ncommit = self._commit_buf[:, 0, 0]
        self._ncommitted += ncommit
        for s in np.nonzero(ncommit)[0]:
            rec = self._commit_buf[s, 1:1 + ncommit[s]]
            lp = np.ascontiguousarray(rec[:, 2]).view(np.float32).astype(np.float64)
            self._committed[s] = np.concatenate([self._committed[s], rec[:, 0].astype(np.int64)])
            self._committed_frames[s] = np.concatenate([self._committed_frames[s], rec[:, 1]])
            self._committed_logp[s] = np.concatenate([self._committed_logp[s], lp])

    def live_nodes(self):
        """int32 [S]: every stream's token-tree nodes after the last advance's compaction (what the capacity rule
        counts)."""
        return self._live.copy()

    def _read(self, detail=True):
        """The read-out: the ranked uncommitted tails of every stream as host arrays (``detail=False``: tokens only)."""
        net = self._weights()
        lib = _lib.load()
        S, W = self.S, self.W
        MT = max(1, int(self._live.max()))          # a tail holds at most the stream's live nodes
        if self._result_mt < MT:
            self._result = torch.empty(lib.edgedict_sync_stream_result_bytes(S, W, MT), dtype=torch.uint8,
                                       device=self.device)
            self._result_mt = MT
        MT = self._result_mt
        tokens = np.empty((S, W, MT), dtype=np.int32)       # (only the used columns are written and read)
        frames = np.empty((S, W, MT), dtype=np.int32) if detail else None
        tlogp = np.empty((S, W, MT), dtype=np.float64) if detail else None
        ntok = np.zeros((S, W), dtype=np.int32)
        nhyp = np.zeros(S, dtype=np.int32)
        logp = np.zeros((S, W), dtype=np.float64)
        ncom = np.zeros(S, dtype=np.int64)
        nfr = np.zeros(S, dtype=np.int64)
        vp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
        rc = lib.edgedict_sync_stream_read(S, net.L, net.H, W, self.NC, _lib.ptr(self._state), _lib.ptr(self._result),
                                           vp(tokens), vp(frames), vp(tlogp), MT, vp(ntok), vp(nhyp), vp(logp), vp(ncom),
                                           vp(nfr), _lib.stream_ptr())
        _lib.check(rc, "sync_stream_read")
        bad = (ncom != self._ncommitted) | (nfr != self._frames)
        if bad.any():
            s = int(np.argmax(bad))
            raise RuntimeError("sync_stream_read: stream %d has %d committed tokens and %d frames on the device, "
                               "%d and %d on the host" % (s, ncom[s], nfr[s], self._ncommitted[s], self._frames[s]))
        return tokens, frames, tlogp, ntok, nhyp, logp

    def nbest(self):
        """Per stream a ranked ``NBestResult`` (``logp`` descending, ties keep beam order): the beam as
        ``sync_beam_search_nbest`` over the stream's frames since its reset returns it, every hypothesis the committed log
        followed by its uncommitted tail, in tokens, frames and ``token_logp`` alike.  Does not modify the state."""
        prefix = list(zip(self._committed, self._committed_frames, self._committed_logp))
        return _nbest_results(*self._read(), prefix)

    def best(self):
        """Per stream the best hypothesis of the current beam - entry 0 of ``nbest()`` -, as ``sync_beam_search`` returns
        it: ``(list of int64 arrays (tokens, no blanks), fp64 tensor [S] = -log p)``."""
        tokens, _, _, ntok, _, logp = self._read(detail=False)
        tails, n = tokens[:, 0].astype(np.int64), ntok[:, 0].tolist()
        seqs = [np.concatenate([c, tails[s, :n[s]]]) if len(c) else tails[s, :n[s]].copy()
                for s, c in enumerate(self._committed)]
        return seqs, torch.from_numpy(-logp[:, 0])

    def committed(self):
        """Per stream the committed tokens (int64 arrays): a prefix of every hypothesis of ``nbest()`` that no later
        frame can change."""
        return [c.copy() for c in self._committed]

    def committed_detail(self):
        """Per stream ``(tokens int64, frames int32, token_logp float64)`` of the committed log."""
        return [(t.copy(), f.copy(), l.copy())
                for t, f, l in zip(self._committed, self._committed_frames, self._committed_logp)]


class StreamingSyncFusionBeamSearch(StreamingSyncBeamSearch):
    """``StreamingSyncBeamSearch`` with ``lm`` / ``lm_weight`` / ``length_bonus`` / ``lm_bos`` / ``bias``: LM shallow
    fusion and contextual biasing as in ``sync_beam_search_fusion``, every method the base class's.  After any chunk
    ``nbest()`` is bit for bit ``sync_beam_search_nbest_rows(..., lm=, bias=)`` over the stream's frames since its reset.

    The rows' LM states (both buffers) and automaton states live in the persistent state behind the plain layout, are
    cleared by ``reset`` and untouched by compaction; the LM's root token is ``lm_bos`` for the empty sequence only
    (``len`` counts committed tokens too).  The bias list is shared by all streams; ``set_bias`` swaps it between
    utterances.  Without an LM and without a list (or with an empty one) the plain kernels run until ``set_bias`` gives
    the search a list.  With an LM a frame is ``6 + L + lm.nlayers + 1`` launches on the fused steps.

    ``lm`` may be an ``edgedict_amd.ngram.NGramLM`` instead (``sync_beam_search_fusion`` states the score and the
    rules): the rows' n-gram states (one int32 each) live in the persistent state behind the fused rows' part, ``reset``
    puts them back on the table's ``start``, compaction does not touch them, and a frame is the plain search's
    ``6 + L`` launches.  ``lm_bos`` is not read with an n-gram.

    ``ilm_weight``: internal-LM estimation as in ``sync_beam_search_fusion``, with or without ``lm`` / ``bias``;
    ``nbest()`` is then bit for bit ``sync_beam_search_nbest_rows(..., ilm_weight=)``.  It carries no per-row state: the
    persistent state keeps its layout, and a frame its launch count on the fused step."""

    def __init__(self, model, n_streams, W=10, node_capacity=None, *, lm=None, lm_weight=None, length_bonus=0.0,
                 lm_bos=1, bias=None, ilm_weight=None):
        self._setup(model, n_streams, W, node_capacity, lm, lm_weight, length_bonus, lm_bos, bias, ilm_weight)


class StreamingCTCBeamSearch:
    """The CTC prefix beam search of ``loss.ctc_prefix_beam`` for S streams whose head logits arrive chunk by chunk
    (csrc/ctc_decode.hip, ``edgedict_ctc_stream_*``).  It works on raw head logits ``[S, Tc, V]`` and needs no model.

    Every stream's beam - up to W ranked prefixes with ``pb`` / ``pnb``, bias total, LM total, token-tree node, automaton
    state and n-gram state - lives in a persistent device state, so after any number of advances ``nbest()`` is bit for
    bit what ``ctc_prefix_beam`` (same ``W``, ``cand``, ``blank``, ``bias``, ``lm`` keywords) returns for the stream's
    frames since its reset: tokens, frames, ``token_logp`` and ``logp`` alike.  An advance is three launches whatever
    the chunk's length - the offline row pass on the chunk, one walk launch with one wave per stream that loads the beam,
    runs all of the chunk's frames and stores it, one compaction launch - and ONE device-to-host read, for the commits.

    The compaction commits the tokens from the tree's root down to the lowest common ancestor of the live prefixes' nodes
    (no later frame can change them; they move to a host-side log with their frames and log-probs), makes that ancestor
    the root and renumbers the nodes a live prefix still reaches densely, so the device tree stays bounded by
    ``node_capacity`` however long a stream runs.  A prefix that is in the beam is never cut away by its child: the
    ancestor of a set that holds both is the parent or above.

    ``node_capacity`` (NC): token-tree nodes per stream, default ``32 * W + 1024`` as ``StreamingSyncBeamSearch``.  An
    advance adds at most ``n_frames[s] * W`` nodes, so one with ``live[s] + n_frames[s] * W > NC`` (``live_nodes()``: 1
    after a reset) raises ``RuntimeError`` before anything is launched and leaves the state as it was.

    ``W`` in 1 .. 32, ``cand`` in 1 .. 64 (default ``min(V - 1, 32)``), ``bias`` a ``ContextGraph``, ``lm`` an
    ``edgedict_amd.ngram.NGramLM`` with ``lm_weight`` (an LSTM ``LMModel`` raises ``TypeError``) and ``length_bonus``:
    ``ctc_prefix_beam``'s rules, raised before anything is launched.  No ``skip_blank``, no rescoring inside the stream,
    no end-of-sentence term.  A stream with no frames since its reset holds the empty hypothesis with ``logp`` 0."""

    _EMPTY = (np.zeros(0, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float64))

    def __init__(self, n_streams, V, W=10, cand=None, blank=0, node_capacity=None, *, bias=None, lm=None, lm_weight=None,
                 length_bonus=0.0):
        from .bias import active, check_bias_args
        from .loss import CTC_BEAM_MAX_CAND, CTC_BEAM_MAX_W
        from .ngram import check_ngram_args
        S, V, W, blank = int(n_streams), int(V), int(W), int(blank)
        if S < 1:
            raise ValueError("n_streams must be >= 1")
        if V < 2:
            raise ValueError("V = %d: need at least the blank and one symbol" % V)
        if not 0 <= blank < V:
            raise ValueError("blank %d outside [0, %d)" % (blank, V))
        if not 1 <= W <= CTC_BEAM_MAX_W:
            raise ValueError("W = %d outside [1, %d]" % (W, CTC_BEAM_MAX_W))
        cand = min(V - 1, 32) if cand is None else int(cand)
        if not 1 <= cand <= CTC_BEAM_MAX_CAND:
            raise ValueError("cand = %d outside [1, %d]" % (cand, CTC_BEAM_MAX_CAND))
        NC = int(node_capacity) if node_capacity else 32 * W + 1024
        if NC < W:
            raise ValueError("node_capacity = %d is below W = %d: not even one frame fits" % (NC, W))
        check_bias_args(bias, V, False)
        check_ngram_args(lm, lm_weight, length_bonus, V, blank)
        self.S, self.V, self.W, self.cand, self.blank, self.NC = S, V, W, cand, blank, NC
        self.bias = active(bias)
        self.lm, self._lm_weight, self._length_bonus = lm, lm_weight, float(length_bonus)
        self.device = torch.device("cuda", torch.cuda.current_device())
        lib = _lib.load()
        sbytes = lib.edgedict_ctc_stream_state_bytes(S, W, NC)
        if sbytes == 0:
            raise ValueError("StreamingCTCBeamSearch: shapes out of range (S = %d, W = %d, node_capacity = %d)"
                             % (S, W, NC))
        self._state = torch.empty(sbytes, dtype=torch.uint8, device=self.device)
        self._ws, self._ws_tc = None, 0
        self._result, self._result_mt = None, 0
        self._live = np.ones(S, dtype=np.int32)              # token-tree nodes per stream after the last compaction
        self._frames = np.zeros(S, dtype=np.int64)           # frames per stream since its reset
        self._tail = np.zeros(S, dtype=np.int32)             # tokens of its longest uncommitted hypothesis tail
        # the advance's read: [S][1 + NC] records {int32, int32, float32 bits, 0}; record 0 = (commits, live nodes,
        # longest tail)
        self._commit_buf = np.zeros((S, NC + 1, 4), dtype=np.int32)
        self._committed = [self._EMPTY[0]] * S
        self._committed_frames = [self._EMPTY[1]] * S
        self._committed_logp = [self._EMPTY[2]] * S
        self.reset()

    def _opts(self):
        """``(const edgedict_ctc_beam_opts_t*, the objects it points into)`` of this search's native calls."""
        from .ngram import CtcBeamOpts
        opts = CtcBeamOpts()
        keep = [opts]
        if self.bias is not None:
            opts.bias = ctypes.addressof(self.bias.tables(self.device)["struct"])
        if self.lm is not None:
            lms = self.lm.struct(self.device, self._lm_weight, self._length_bonus)
            keep.append(lms)
            opts.ngram = ctypes.addressof(lms)
        return ctypes.byref(opts), keep

    def _mask(self, mask):
        if mask is None:
            return np.ones(self.S, dtype=bool)
        m = mask.detach().cpu().numpy() if torch.is_tensor(mask) else np.asarray(mask)
        return m.astype(bool).reshape(self.S)

    def reset(self, mask=None):
        """Every stream, or those where ``mask[s]`` is true, back to the empty hypothesis with an empty committed log;
        its frames count from 0 again."""
        sel = self._mask(mask)
        md = None if mask is None else torch.from_numpy(sel.astype(np.int32)).to(self.device)
        opts, keep = self._opts()
        rc = _lib.load().edgedict_ctc_stream_reset(self.S, self.W, self.NC, opts, _lib.ptr(md), _lib.ptr(self._state),
                                                   _lib.stream_ptr())
        _lib.check(rc, "ctc_stream_reset")
        self._frames[sel] = 0
        self._live[sel] = 1
        self._tail[sel] = 0
        for s in np.nonzero(sel)[0]:
            self._committed[s], self._committed_frames[s], self._committed_logp[s] = self._EMPTY

    def set_bias(self, graph, mask=None):
        """Swap the bias list (a ``ContextGraph``, or None / an empty one for "no bias"), with
        ``StreamingSyncBeamSearch.set_bias``'s rules: the list is shared by all streams and the entries of a stream in
        mid-utterance hold states of the old automaton, so EVERY stream must be fresh - no frames since its reset - or
        ``ValueError`` is raised.  ``mask`` (None: all) only names the streams the caller swaps the list for.  Nothing is
        launched: a fresh stream stands on state 0, the root of every automaton, and the state's layout does not depend
        on the list."""
        from .bias import active, check_bias_args
        check_bias_args(graph, self.V, False)
        sel = self._mask(mask)
        busy = np.nonzero(self._frames > 0)[0]
        for s in busy:
            if sel[s]:
                raise ValueError("set_bias: stream %d has advanced over %d frames since its reset (reset it first)"
                                 % (s, self._frames[s]))
        if len(busy):
            raise ValueError("set_bias: the bias list is shared by all streams and stream %d, outside the mask, is in "
                             "the middle of an utterance" % busy[0])
        self.bias = active(graph)

    def advance(self, logits, n_frames=None):
        """Advance every stream over the first ``n_frames[s]`` frames (host ints, default all Tc; 0: the stream sits
        this chunk out) of ``logits`` [S, Tc, V] (float32 or bfloat16, contiguous, on the device)."""
        if logits.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError("logits must be float32 or bfloat16, got %s" % logits.dtype)
        if logits.dim() != 3 or logits.shape[0] != self.S or logits.shape[2] != self.V:
            raise ValueError("advance: logits must be [S=%d, Tc, V=%d], got %s" % (self.S, self.V, tuple(logits.shape)))
        if not logits.is_contiguous():
            raise ValueError("logits must be contiguous")
        Tc = int(logits.shape[1])
        if Tc < 1:
            raise ValueError("advance: logits must hold at least one frame (Tc = %d)" % Tc)
        if n_frames is None:
            nf = np.full(self.S, Tc, dtype=np.int32)
        else:
            nf = np.ascontiguousarray(n_frames.cpu().numpy() if torch.is_tensor(n_frames) else n_frames, dtype=np.int32)
            if nf.shape != (self.S,) or (nf < 0).any() or (nf > Tc).any():
                raise ValueError("advance: n_frames must be [S] ints in [0, %d]" % Tc)
        _lib.require_cuda(logits)
        need = self._live.astype(np.int64) + nf.astype(np.int64) * self.W
        if (need > self.NC).any():
            s = int(np.argmax(need > self.NC))
            raise RuntimeError("StreamingCTCBeamSearch: stream %d may need %d token-tree nodes (%d live + %d frames x "
                               "W = %d), node_capacity is %d" % (s, need[s], self._live[s], nf[s], self.W, self.NC))
        lib = _lib.load()
        if Tc > self._ws_tc:                 # the chunk workspace grows with the longest chunk seen
            wbytes = lib.edgedict_ctc_stream_workspace_bytes(self.S, Tc, self.W, self.cand, self.NC)
            if wbytes == 0:
                raise ValueError("advance: S x Tc x cand = %d x %d x %d out of range" % (self.S, Tc, self.cand))
            self._ws, self._ws_tc = torch.empty(wbytes, dtype=torch.uint8, device=self.device), Tc
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        opts, keep = self._opts()
        rc = lib.edgedict_ctc_stream_advance(_lib.ptr(logits.detach()), _lib.dtype_code(logits.dtype), vp(nf), self.S, Tc,
                                             self.V, self.blank, self.W, self.cand, self.NC, opts, vp(self._live),
                                             vp(self._commit_buf), self.NC, _lib.ptr(self._state), _lib.ptr(self._ws),
                                             _lib.stream_ptr())
        _lib.check(rc, "ctc_stream_advance")
        self._frames += nf
        self._tail[:] = self._commit_buf[:, 0, 2]
        ncommit = self._commit_buf[:, 0, 0]
        for s in np.nonzero(ncommit)[0]:
            rec = self._commit_buf[s, 1:1 + ncommit[s]]
            lp = np.ascontiguousarray(rec[:, 2]).view(np.float32).astype(np.float64)
            self._committed[s] = np.concatenate([self._committed[s], rec[:, 0].astype(np.int64)])
            self._committed_frames[s] = np.concatenate([self._committed_frames[s], rec[:, 1]])
            self._committed_logp[s] = np.concatenate([self._committed_logp[s], lp])

    def live_nodes(self):
        """int32 [S]: every stream's token-tree nodes after the last advance's compaction (what the capacity rule
        counts; 1, the root, after a reset)."""
        return self._live.copy()

    def frames_done(self):
        """int64 [S]: frames per stream since its reset."""
        return self._frames.copy()

    def _read(self, top=False):
        """The read-out: the ranked uncommitted tails of every stream as host arrays ``(tokens, frames, token_logp, ntok,
        n_hyp, logp)``, [S, W, ...]; ``top=True``: entry 0 alone, [S, 1, ...] - one read of S rows instead of S W."""
        lib = _lib.load()
        S, W = self.S, self.W
        MT = 16 * ((max(1, int(self._tail.max())) + 15) // 16)        # the longest tail, in steps of 16
        if self._result_mt != MT:
            self._result_mt = MT
            self._result = (torch.empty(S * W * (3 * MT + 1), dtype=torch.int32, device=self.device),
                            torch.empty(S * W + S, dtype=torch.float64, device=self.device))
        ints, dbl = self._result
        n = S * W * MT
        tokens, frames, tlp, ntok = ints[:n], ints[n:2 * n], ints[2 * n:3 * n], ints[3 * n:]
        logp, nhyp = dbl[:S * W], dbl[S * W:].view(torch.int32)
        rc = lib.edgedict_ctc_stream_nbest(S, W, self.NC, _lib.ptr(self._state), MT, _lib.ptr(tokens), _lib.ptr(frames),
                                           _lib.ptr(tlp), _lib.ptr(ntok), _lib.ptr(nhyp), _lib.ptr(logp),
                                           _lib.stream_ptr())
        _lib.check(rc, "ctc_stream_nbest")
        if top:
            # entry 0 of every stream, packed on the device: tokens, frames, token_lp bits, ntok, n_hyp, logp as int32
            rows = lambda a: a.view(S, W, MT)[:, 0]
            hi = torch.cat([rows(tokens), rows(frames), rows(tlp), ntok.view(S, W)[:, :1], nhyp[:S].view(S, 1),
                            logp.view(S, W)[:, :1].contiguous().view(torch.int32)], dim=1).cpu().numpy()
            tlogp = np.ascontiguousarray(hi[:, 2 * MT:3 * MT]).view(np.float32).astype(np.float64)
            return (hi[:, None, :MT], hi[:, None, MT:2 * MT], tlogp[:, None], hi[:, 3 * MT:3 * MT + 1], hi[:, 3 * MT + 1],
                    np.ascontiguousarray(hi[:, 3 * MT + 2:]).view(np.float64))
        hi, hd = ints.cpu().numpy(), dbl.cpu().numpy()
        tlogp = np.ascontiguousarray(hi[2 * n:3 * n]).view(np.float32).reshape(S, W, MT).astype(np.float64)
        nhyp = np.ascontiguousarray(hd[S * W:]).view(np.int32)[:S]
        return (hi[:n].reshape(S, W, MT), hi[n:2 * n].reshape(S, W, MT), tlogp, hi[3 * n:].reshape(S, W), nhyp,
                hd[:S * W].reshape(S, W))

    def nbest(self):
        """Per stream a ranked ``NBestResult`` (``logp`` descending, entry 0 the answer): the list ``ctc_prefix_beam``
        returns for the stream's frames since its reset, every hypothesis the committed log followed by its uncommitted
        tail, in tokens, frames and ``token_logp`` alike.  Does not modify the state."""
        prefix = list(zip(self._committed, self._committed_frames, self._committed_logp))
        return _nbest_results(*self._read(), prefix)

    def best(self):
        """Per stream entry 0 of ``nbest()``: ``(list of int64 arrays (tokens, no blanks), fp64 tensor [S] = -log p)``."""
        tokens, _, _, ntok, _, logp = self._read(top=True)
        tails, n = tokens[:, 0].astype(np.int64), ntok[:, 0].tolist()
        seqs = [np.concatenate([c, tails[s, :n[s]]]) if len(c) else tails[s, :n[s]].copy()
                for s, c in enumerate(self._committed)]
        return seqs, torch.from_numpy(-logp[:, 0])

    def committed(self):
        """Per stream the committed tokens (int64 arrays): a prefix of every hypothesis of ``nbest()`` that no later
        frame can change."""
        return [c.copy() for c in self._committed]

    def committed_detail(self):
        """Per stream ``(tokens int64, frames int32, token_logp float64)`` of the committed log."""
        return [(t.copy(), f.copy(), l.copy())
                for t, f, l in zip(self._committed, self._committed_frames, self._committed_logp)]

    def idle_frames(self):
        """int64 [S]: frames since the last token of each stream's best hypothesis was created - frames so far minus one
        minus that token's frame -, or the frames since the reset where the best hypothesis is empty: what an
        endpointer waits on.  Host arithmetic on what ``best()`` reads."""
        _, frames, _, ntok, _, _ = self._read(top=True)
        out = self._frames.copy()
        for s in range(self.S):
            n = int(ntok[s, 0])
            if n > 0:
                out[s] = self._frames[s] - 1 - int(frames[s, 0, n - 1])
            elif len(self._committed_frames[s]):
                out[s] = self._frames[s] - 1 - int(self._committed_frames[s][-1])
        return out


def emission_times(frames, flags, time_reduction=2):
    """Seconds (float64 tensor, shape of ``frames``) at which the encoder frames of ``Transducer.align`` /
    ``loss.rnnt_align`` - or the decoder's own, ``NBestResult.frames`` of ``beam_search_nbest`` / ``nbest()`` (counted
    from the utterance's start, or from the stream's reset) - START: one encoder frame covers ``flags.hop_length * flags.downsample * time_reduction`` samples
    (feature hop x frame stacking, as ``stream.chunk_geometry`` counts a chunk's hop, x the encoder's time reductions:
    2 per reduced layer, ``enc_time_reductions=[1]`` by default -> 2).  The -1 padding behind an utterance's labels
    becomes NaN.  The frame's END is one such step later; a causal model cannot have seen the token's audio before."""
    frames = torch.as_tensor(frames)
    step = flags.hop_length * max(1, flags.downsample) * int(time_reduction) / float(getattr(flags, "sample_rate", 16000))
    out = frames.to(torch.float64) * step
    return torch.where(frames < 0, torch.full_like(out, float("nan")), out)


# ---------------------------------------------------------------------------------------------------------------------
# Confidence of N-best hypotheses: a post-pass over the lists any search returned (csrc/confidence.hip).
CONF_METHODS = ("prob", "max_prob", "entropy", "tsallis")
CONF_AGGREGATES = ("min", "mean", "prod")
CONF_LOGITS_BYTES = 64 << 20        # the fp32 logits buffer of one chunk of hypothesis_confidence stays at or under this


def confidence_measure(stats, V, method="tsallis", alpha=1.0 / 3.0):
    """A confidence in ``[0, 1]`` per row of ``stats`` [..., 5] (``loss.row_confidence``'s columns), on the host in
    float64.  The distribution is the row's softmax over all ``V`` symbols, the blank included.

        ``"prob"``      ``exp(logp)``: the probability of the row's token
        ``"max_prob"``  ``exp(logp_max)``: the largest probability of the row
        ``"entropy"``   ``1 - H / ln V``: one minus the Shannon entropy normalised by its maximum
        ``"tsallis"``   ``1 - (1 - sum_v p_v^alpha) / (1 - V^(1 - alpha))``: one minus the Tsallis entropy of order
                        ``alpha`` normalised by its maximum (Laptev & Ginsburg 2022), ``0 < alpha < 1``; ``alpha``
                        must be the one the statistics were computed with

    The result is clipped to ``[0, 1]``: a uniform row gives 0 for the two entropy measures, a one-hot row 1.  NaN
    statistics stay NaN.  No calibration is claimed for any of them."""
    stats = np.asarray(stats, dtype=np.float64)
    V, alpha = int(V), float(alpha)
    if stats.shape[-1] != 5:
        raise ValueError("confidence_measure: stats must be [..., 5]")
    if V < 2:
        raise ValueError("confidence_measure: V = %d, need at least two symbols" % V)
    if method == "prob":
        c = np.exp(stats[..., 0])
    elif method == "max_prob":
        c = np.exp(stats[..., 1])
    elif method == "entropy":
        c = 1.0 - stats[..., 3] / np.log(V)
    elif method == "tsallis":
        if not 0.0 < alpha < 1.0:
            raise ValueError("confidence_measure: alpha must lie inside (0, 1), got %r" % (alpha,))
        c = 1.0 - (1.0 - np.exp(stats[..., 4])) / (1.0 - V ** (1.0 - alpha))
    else:
        raise ValueError("confidence_measure: method must be one of %s, got %r" % (", ".join(CONF_METHODS), method))
    return np.clip(c, 0.0, 1.0)


class WordTable:
    """Which tokens end a word: ``word_end`` bool [V] (a token with it set is the LAST token of its word: the
    reference's CharBPE pieces ending in ``</w>``) and ``separators``, token ids that stand between words and belong to
    none (the char tokenizer's space)."""

    def __init__(self, word_end, separators=()):
        self.word_end = np.asarray(word_end, dtype=bool).reshape(-1)
        self.separators = sorted(int(k) for k in separators)
        if any(k < 0 or k >= self.word_end.size for k in self.separators):
            raise ValueError("WordTable: a separator id lies outside [0, %d)" % self.word_end.size)

    def spans(self, tokens):
        """``[(first, last), ...]``: the token index ranges (inclusive) of the words of one hypothesis.  A word ends at
        a token with ``word_end`` set; a separator ends the word before it and is part of none; a trailing run without
        an end marker is still a word."""
        out, start = [], None
        for u, k in enumerate(int(t) for t in tokens):
            if k in self.separators:
                if start is not None:
                    out.append((start, u - 1))
                start = None
                continue
            if start is None:
                start = u
            if 0 <= k < self.word_end.size and self.word_end[k]:
                out.append((start, u))
                start = None
        if start is not None:
            out.append((start, len(tokens) - 1))
        return out


def word_table(tokenizer, V):
    """The ``WordTable`` of a tokenizer's first ``V`` pieces, from their texts (``stream._token_text``): a piece that
    ends in ``</w>`` ends a word, a piece that is a single space is a separator."""
    from .stream import _token_text
    texts = [_token_text(tokenizer, i) for i in range(int(V))]
    return WordTable([bool(t) and t.endswith("</w>") for t in texts], [i for i, t in enumerate(texts) if t == " "])


def aggregate_confidence(values, how="min"):
    """``min`` / ``mean`` / ``prod`` of token confidences (float64); NaN for none."""
    values = np.asarray(values, dtype=np.float64)
    if how not in CONF_AGGREGATES:
        raise ValueError("aggregate must be one of %s, got %r" % (", ".join(CONF_AGGREGATES), how))
    if values.size == 0:
        return float("nan")
    return float({"min": np.min, "mean": np.mean, "prod": np.prod}[how](values))


def word_confidence(tokens, frames, values, table, aggregate="min"):
    """The words of one hypothesis as ``(first_token, last_token, start_frame, end_frame, confidence)``: token indices
    into the hypothesis, the frames of the word's first and last token (``emission_times`` turns them into seconds),
    and the ``aggregate`` of the tokens' confidences ``values``."""
    return [(a, b, int(frames[a]), int(frames[b]), aggregate_confidence(values[a:b + 1], aggregate))
            for a, b in table.spans(tokens)]


class Confidence:
    """The confidences of one utterance's N-best list, hypothesis ``i`` in the list's own order:

    ``token[i]``      float64 array, one value in ``[0, 1]`` per token (``confidence_measure`` with ``method``, ``alpha``)
    ``raw[i]``        float64 [len, 5]: the statistics behind them, ``loss.CONF_COLUMNS`` (``raw[i][:, 0]`` is the
                      acoustic model's own log-probability of the token: ``token_logp`` without LM and bias terms)
    ``top[i]``        int32 array: the most probable symbol at each token's place (the blank included)
    ``utterance``     float64 [n]: the ``aggregate`` over each hypothesis' tokens; NaN for an empty hypothesis
    ``word[i]``       None, or with ``words=`` a list of ``(first_token, last_token, start_frame, end_frame, confidence)``
    """

    def __init__(self, token, raw, top, utterance, word, method, alpha, aggregate):
        self.token, self.raw, self.top, self.word = list(token), list(raw), list(top), list(word)
        self.utterance = np.asarray(utterance, dtype=np.float64)
        self.method, self.alpha, self.aggregate = method, alpha, aggregate

    def __len__(self):
        return len(self.token)


def _check_confidence(what, method, alpha, aggregate, words):
    if method not in CONF_METHODS:
        raise ValueError("%s: method must be one of %s, got %r" % (what, ", ".join(CONF_METHODS), method))
    try:
        alpha = float(alpha)
    except (TypeError, ValueError):
        raise ValueError("%s: alpha must be a number inside (0, 1), got %r" % (what, alpha)) from None
    if not 0.0 < alpha < 1.0:
        raise ValueError("%s: alpha must lie inside (0, 1), got %r" % (what, alpha))
    if aggregate not in CONF_AGGREGATES:
        raise ValueError("%s: aggregate must be one of %s, got %r" % (what, ", ".join(CONF_AGGREGATES), aggregate))
    if words is not None and not isinstance(words, WordTable):
        raise TypeError("%s: words must be a decode.WordTable (decode.word_table builds one)" % what)
    return alpha


def _confidence_rows(what, results, enc_out, lens, V, blank):
    """The argument rules both passes share, then the compact rows: ``(results, lens, hyps, enc_row, tok)`` with
    ``hyps`` the (utterance, index, tokens, frames) of every non-empty hypothesis in list order and ``enc_row`` /
    ``tok`` int32 arrays with one entry per live token (``enc_row = b * T + frame``), hypothesis after hypothesis."""
    _lib.require_cuda(enc_out)
    if enc_out.dim() != 3:
        raise ValueError("%s: enc_out must be [B, T, P]" % what)
    B, T, _ = enc_out.shape
    results = list(results)
    if len(results) != B:
        raise ValueError("%s: %d lists for a batch of %d utterances" % (what, len(results), B))
    lens = np.full(B, T, dtype=np.int64) if lens is None else np.asarray(lens, dtype=np.int64).reshape(-1)
    if lens.shape != (B,) or (lens < 0).any() or (lens > T).any():
        raise ValueError("%s: lens must be [B] ints in [0, %d]" % (what, T))
    hyps, enc_row, tok = [], [], []
    for b, r in enumerate(results):
        for i in range(len(r)):
            t = np.asarray(r.tokens[i], dtype=np.int64).reshape(-1)
            f = np.asarray(r.frames[i], dtype=np.int64).reshape(-1)
            if t.shape != f.shape:
                raise ValueError("%s: utterance %d, hypothesis %d: %d tokens but %d frames" % (what, b, i, t.size, f.size))
            if t.size == 0:
                continue
            if (f < 0).any() or (f >= lens[b]).any():
                raise ValueError("%s: utterance %d, hypothesis %d: a frame outside [0, %d)" % (what, b, i, lens[b]))
            if (t < 0).any() or (t >= V).any() or (t == blank).any():
                raise ValueError("%s: utterance %d, hypothesis %d: a token that is blank or outside [0, %d)"
                                 % (what, b, i, V))
            hyps.append((b, i, t, f))
            enc_row.append(b * T + f)
            tok.append(t)
    cat = lambda a: np.concatenate(a).astype(np.int32) if a else np.zeros(0, dtype=np.int32)      # noqa: E731
    return results, lens, hyps, cat(enc_row), cat(tok)


def _confidence_results(results, hyps, host, R, V, method, alpha, aggregate, words):
    """One ``Confidence`` per utterance from the pass's single host read ``host`` (None: no live token): fp32 words,
    ``[R, 5]`` statistics and behind them the R int32 arg-maxes."""
    stats, top = np.zeros((0, 5)), np.zeros(0, dtype=np.int32)
    if R:
        stats = host[:R * 5].reshape(R, 5).astype(np.float64)
        top = host[R * 5:].view(np.int32)
    out, at, pos = [], {}, 0
    for b, i, t, f in hyps:
        at[(b, i)] = (pos, t.size)
        pos += t.size
    for b, r in enumerate(results):
        token, raw, tops, word = [], [], [], []
        for i in range(len(r)):
            o, n = at.get((b, i), (0, 0))
            raw.append(stats[o:o + n].copy() if n else np.zeros((0, 5)))
            tops.append(top[o:o + n].copy() if n else np.zeros(0, dtype=np.int32))
            token.append(confidence_measure(raw[-1], V, method, alpha))
            word.append(None if words is None else
                        word_confidence(r.tokens[i], r.frames[i], token[-1], words, aggregate))
        out.append(Confidence(token, raw, tops, [aggregate_confidence(c, aggregate) for c in token], word, method, alpha,
                              aggregate))
    return out


def confidence_hidden_rows(E1, D1, enc_row, dec_row, b1=None, out=None):
    """The raw call of csrc/confidence.hip ``conf_hidden_rows``: ``hid[r] = tanh(E1[enc_row[r]] + D1[dec_row[r]] + b1)``
    in the dtype of ``E1`` [n_enc_rows, J] and ``D1`` [n_dec_rows, J] (contiguous, on the device), ``enc_row`` /
    ``dec_row`` int32 [R] device tensors, ``b1`` fp32 [J] or None (nothing added).  A row with an index out of range is
    NaN and nothing is read for it.  Returns ``hid`` [R, J] (``out`` if given).  No host sync."""
    _lib.require_cuda(E1, D1, enc_row, dec_row, b1, out)
    if E1.dim() != 2 or D1.dim() != 2 or E1.dtype != D1.dtype or E1.shape[1] != D1.shape[1]:
        raise ValueError("confidence_hidden_rows: E1 and D1 must be [rows, J] of one dtype")
    if not (E1.is_contiguous() and D1.is_contiguous()):
        raise ValueError("confidence_hidden_rows: E1 and D1 must be contiguous")
    J, R = E1.shape[1], enc_row.shape[0]
    for v in (enc_row, dec_row):
        if v.dtype != torch.int32 or v.shape != (R,) or not v.is_contiguous():
            raise ValueError("confidence_hidden_rows: enc_row and dec_row must be contiguous int32 [R]")
    if b1 is not None and (b1.dtype != torch.float32 or b1.shape != (J,) or not b1.is_contiguous()):
        raise ValueError("confidence_hidden_rows: b1 must be contiguous fp32 [J]")
    if out is None:
        out = torch.empty(R, J, dtype=E1.dtype, device=E1.device)
    elif out.shape != (R, J) or out.dtype != E1.dtype or not out.is_contiguous():
        raise ValueError("confidence_hidden_rows: out must be contiguous [R, J] in the operands' dtype")
    if R and J:
        _lib.call("conf_hidden_rows", dtype_code(E1.dtype), E1 if E1.shape[0] else None, E1.shape[0],
                  D1 if D1.shape[0] else None, D1.shape[0], b1, enc_row, dec_row, R, J, out)
    return out


@torch.no_grad()
def hypothesis_confidence(model, enc_out, lens, results, *, method="tsallis", alpha=1.0 / 3.0, aggregate="min", words=None,
                          chunk_rows=None):
    """Token, word and utterance confidences of N-best lists from the transducer's own output distribution:
    ``results`` (one ``NBestResult`` per utterance of ``enc_out`` [B, T, P], compute dtype, device; ``lens`` host ints,
    encoder frames per utterance, or None for all T) from ANY search over this encoder output - best-first,
    frame-synchronous, ``skip_blank=`` (its frames are in the original numbering), a stream's ``nbest()`` on the kept
    encoder output, a list read from disk.  No search runs again: the joint is re-evaluated at every token's
    ``(frame, prefix)`` and each row of logits is reduced to ``loss.row_confidence``'s statistics.

    The pass: compact rows for the live tokens only (no ``[B, N, U]`` padding of the rows), ONE int32 upload (the padded
    hypotheses for the prediction network and per row ``enc_row = b T + frame``, ``dec_row``, ``token``); the prediction
    network teacher-forced on every non-empty hypothesis, BOS in front (row ``u`` is its output after ``y_<u``);
    ``joint_rows`` and ``D1 = dec W1d^T + b1`` through ``ops.gemm``; then per chunk of rows the gathered hidden kernel,
    the logits product (``ops.gemm``, fp32) and the row kernel; ONE read to the host.  A chunk keeps the fp32 logits
    buffer at or under 64 MiB (``chunk_rows`` overrides the rows per chunk).  Values are rounded where the search's
    composed step rounds them, so ``raw[i][:, 0]`` reproduces a plain search's ``token_logp`` up to summation order.

    This is the ACOUSTIC model's distribution: LM, internal-LM and bias terms of the search that made the list take no
    part (``token_logp`` contains them, ``raw[i][:, 0]`` does not).  ``method`` / ``alpha``: ``confidence_measure``;
    ``aggregate`` (``min`` / ``mean`` / ``prod``) folds token values into words and utterances; ``words``: a
    ``WordTable`` - ``Confidence.word`` is then filled.  Returns one ``Confidence`` per utterance.

    Raised before anything is launched: ``ValueError`` for a frame outside ``[0, lens[b])``, a token that is blank or
    outside ``[0, V)``, a ``results`` length other than ``B``, a bad ``method`` / ``alpha`` / ``aggregate``;
    ``RuntimeError`` for a CPU ``enc_out``.  If every hypothesis is empty nothing is launched.  No calibration is
    claimed: there is no corpus here to measure one on."""
    from .loss import _conf_row_stats
    what = "hypothesis_confidence"
    V = _vocab(model)
    alpha = _check_confidence(what, method, alpha, aggregate, words)
    if chunk_rows is not None and int(chunk_rows) < 1:
        raise ValueError("%s: chunk_rows must be >= 1" % what)
    results, lens, hyps, enc_row, tok = _confidence_rows(what, results, enc_out, lens, V, int(model.blank))
    R = int(tok.size)
    if R == 0:
        return _confidence_results(results, hyps, None, 0, V, method, alpha, aggregate, words)
    enc_out = enc_out.contiguous()
    B, T, P = enc_out.shape
    dev, cd = enc_out.device, enc_out.dtype
    Nh, U = len(hyps), max(t.size for _, _, t, _ in hyps)
    # one upload: the padded hypotheses [Nh, U], then enc_row, dec_row, token [R] each
    host = np.zeros(Nh * U + 3 * R, dtype=np.int32)
    padded, dec_row = host[:Nh * U].reshape(Nh, U), host[Nh * U + R:Nh * U + 2 * R]
    pos = 0
    for h, (_, _, t, _) in enumerate(hyps):
        padded[h, :t.size] = t
        dec_row[pos:pos + t.size] = h * (U + 1) + np.arange(t.size)
        pos += t.size
    host[Nh * U:Nh * U + R] = enc_row
    host[Nh * U + 2 * R:] = tok
    up = torch.from_numpy(host).to(dev)
    d_enc, d_dec, d_tok = (up[Nh * U + k * R:Nh * U + (k + 1) * R] for k in range(3))
    net = _SearchNet(model, cd)
    h_dec, _ = model.decoder(up[:Nh * U].view(Nh, U))               # [Nh, U + 1, P2]
    h_dec = h_dec.reshape(Nh * (U + 1), net.P2)
    if h_dec.dtype != cd:
        h_dec = ops.cast(h_dec, cd)
    E1 = net.e1(enc_out)
    D1 = ops.gemm(h_dec, net.w1c[:, P:], bias=net.b1)              # the search step's first product, bias included
    chunk = int(chunk_rows) if chunk_rows is not None else max(1, CONF_LOGITS_BYTES // (4 * V))
    chunk = min(chunk, R)
    out = torch.empty(R * 6, dtype=torch.float32, device=dev)       # stats [R, 5], then top [R] (int32 bits)
    stats, top = out[:R * 5].view(R, 5), out[R * 5:].view(torch.int32)
    hid = torch.empty(chunk, net.J, dtype=cd, device=dev)
    logits = torch.empty(chunk, V, dtype=torch.float32, device=dev)
    for lo in range(0, R, chunk):
        n = min(chunk, R - lo)
        confidence_hidden_rows(E1, D1, d_enc[lo:lo + n], d_dec[lo:lo + n], None, hid[:n])
        ops.gemm(hid[:n], net.w2c, out=logits[:n], bias=net.b2)
        _conf_row_stats(logits, V, n, None, d_tok[lo:lo + n], n, V, net.blank, alpha, stats[lo:lo + n], top[lo:lo + n])
    return _confidence_results(results, hyps, out.cpu().numpy(), R, V, method, alpha, aggregate, words)


@torch.no_grad()
def ctc_hypothesis_confidence(model, enc_out, lens, results, *, method="tsallis", alpha=1.0 / 3.0, aggregate="min",
                              words=None):
    """``hypothesis_confidence`` for lists of ``ctc_beam_search`` (or any list whose frames are the frames a CTC path
    creates its tokens on), from the CTC head's distribution: the rows are the head's logits (``model._ctc_logits``, in
    the compute dtype) on each token's frame, read by the row kernel through its gather index.  Neither the prediction
    network nor the joint runs.  One int32 upload, one launch, one read to the host.  The n-gram LM and bias terms of
    the search take no part.  Arguments, errors and the return value as there; ``RuntimeError`` on a model built
    without ``ctc_weight > 0``."""
    from .loss import _conf_row_stats
    what = "ctc_hypothesis_confidence"
    if getattr(model, "ctc_head", None) is None:
        raise RuntimeError("this model has no CTC head: construct it with Transducer(..., ctc_weight > 0)")
    V = _vocab(model)
    alpha = _check_confidence(what, method, alpha, aggregate, words)
    results, lens, hyps, enc_row, tok = _confidence_rows(what, results, enc_out, lens, V, int(model.blank))
    R = int(tok.size)
    if R == 0:
        return _confidence_results(results, hyps, None, 0, V, method, alpha, aggregate, words)
    enc_out = enc_out.contiguous()
    B, T, _ = enc_out.shape
    up = torch.from_numpy(np.concatenate([enc_row, tok])).to(enc_out.device)
    logits = model._ctc_logits(enc_out).contiguous().view(B * T, V)
    out = torch.empty(R * 6, dtype=torch.float32, device=enc_out.device)
    _conf_row_stats(logits, V, B * T, up[:R], up[R:], R, V, int(model.blank), alpha, out[:R * 5].view(R, 5),
                    out[R * 5:].view(torch.int32))
    return _confidence_results(results, hyps, out.cpu().numpy(), R, V, method, alpha, aggregate, words)
