"""Error rates: a batched edit distance on the device (csrc/edit_distance.hip) and what is built on it - token and word
error rates, the per-hypothesis errors of N-best lists, their oracle error rate and their expected number of errors.

**The quantity.**  For a hypothesis ``h`` and a reference ``r`` (int32 sequences, compared with ``==`` only: every
int32 value is a symbol), ``d(i, j)`` is the cheapest way to turn ``r[:j]`` into ``h[:i]`` with integer edge costs: a
hit (``h[i-1] == r[j-1]``) 0, a substitution ``K``, a deletion (a reference element without a hypothesis element)
``K``, an insertion (a hypothesis element without a reference element) ``K + 1``; ``K = 4096``, ``d(0, j) = j K``,
``d(i, 0) = i (K + 1)``.  With both lengths at most 1023, ``v = d(H, R)`` decomposes exactly: ``dist = v // K`` is the
Levenshtein distance and ``ins = v % K`` the number of insertions of the minimum-distance alignment with the FEWEST
insertions (the tie rule).  ``ins - del = H - R`` is fixed, so that alignment also has the fewest deletions and the most
substitutions: ``del = ins - (H - R)``, ``sub = dist - ins - del``, ``hits = R - sub - del``.  All integers: the kernel
and the host oracle (tests/edit_distance_ref.py) agree by equality, nothing here has a tolerance.

``edit_distance`` is the kernel call (device tensors in, a device tensor out, no host sync), ``edit_distance_lists`` the
host-side packer (one upload, one call, one read), ``ErrorRate`` an accumulator whose totals stay on the device.
``token_error_rate`` / ``word_error_rate`` are one-call host conveniences; ``nbest_errors``, ``oracle_error_rate`` and
``expected_errors`` take the ``decode.NBestResult`` lists of the searches.  The validation loop of the reference
(cli/train.py:273-319) is ``TrainEngine.evaluate`` / ``Transducer.evaluate_step``.

Limits: at most 32 hypotheses per utterance and kernel call (``edit_distance_lists`` splits longer lists over several
rows of the same call), at most 1023 elements per sequence.
"""
import collections

import numpy as np
import torch

from . import _lib

EDIT_MAX_N = 32
EDIT_MAX_U = 1023

ErrorRateResult = collections.namedtuple(
    "ErrorRateResult", ["rate", "sub_rate", "del_rate", "ins_rate", "sentence_rate", "errors", "substitutions",
                        "deletions", "insertions", "ref_len", "sequences", "wrong_sequences"])
ErrorRateResult.__doc__ = """The record of an error rate: ``rate = errors / ref_len`` (summed errors over summed
reference elements - the corpus-level figure; ``nan`` when ``ref_len == 0``), the three per-kind rates
``substitutions / ref_len``, ``deletions / ref_len``, ``insertions / ref_len``, ``sentence_rate = wrong_sequences /
sequences`` (``nan`` without a sequence), and the seven integer totals they are made of."""


def _record(errors, substitutions, deletions, insertions, ref_len, sequences, wrong_sequences):
    t = [int(v) for v in (errors, substitutions, deletions, insertions, ref_len, sequences, wrong_sequences)]
    nan = float("nan")
    per = [v / t[4] if t[4] else nan for v in t[:4]]
    return ErrorRateResult(per[0], per[1], per[2], per[3], t[6] / t[5] if t[5] else nan, *t)


def _certify_edit_distance_inputs(hyps, hyp_lens, refs, ref_lens, n_hyp):
    # error classes / wording of loss._certify_ctc_score_inputs
    named = (("hyps", hyps), ("hyp_lens", hyp_lens), ("refs", refs), ("ref_lens", ref_lens), ("n_hyp", n_hyp))
    for name, t in named:
        if t is not None and not torch.is_tensor(t):
            raise TypeError("%s must be a tensor, got %s" % (name, type(t).__name__))
    for name, t in named:
        if t is not None and t.dtype != torch.int32:
            raise TypeError("%s must be int32, got %s" % (name, t.dtype))
    for name, t in named:
        if t is not None and not t.is_contiguous():
            raise ValueError("%s must be contiguous" % name)
    if hyps.dim() != 3:
        raise ValueError("hyps must have 3 dimensions [B,N,Uh] (or 2, [B,Uh], for plain pairs), got %d" % hyps.dim())
    if hyp_lens.dim() != 2:
        raise ValueError("hyp_lens must have 2 dimensions [B,N], got %d" % hyp_lens.dim())
    if refs.dim() != 2:
        raise ValueError("refs must have 2 dimensions [B,Ur], got %d" % refs.dim())
    if ref_lens.dim() != 1 or (n_hyp is not None and n_hyp.dim() != 1):
        raise ValueError("ref_lens and n_hyp must have 1 dimension")
    B, N, Uh = hyps.shape
    Ur = refs.shape[1]
    if tuple(hyp_lens.shape) != (B, N):
        raise ValueError("must have a hypothesis length per slot (hyps is %s, hyp_lens %s)"
                         % (tuple(hyps.shape), tuple(hyp_lens.shape)))
    if refs.shape[0] != B or ref_lens.shape[0] != B:
        raise ValueError("must have a reference and its length per example (refs is %s, ref_lens has %d, batch is %d)"
                         % (tuple(refs.shape), ref_lens.shape[0], B))
    if n_hyp is not None and n_hyp.shape[0] != B:
        raise ValueError("must have a hypothesis count per example (n_hyp has %d, batch is %d)" % (n_hyp.shape[0], B))
    if B < 1:
        raise ValueError("hyps must hold at least one utterance (B = %d)" % B)
    if not 1 <= N <= EDIT_MAX_N:
        raise ValueError("N = %d hypotheses per utterance outside [1, %d]" % (N, EDIT_MAX_N))
    if Uh > EDIT_MAX_U:
        raise ValueError("Uh = %d exceeds the supported maximum of %d tokens per hypothesis" % (Uh, EDIT_MAX_U))
    if Ur > EDIT_MAX_U:
        raise ValueError("Ur = %d exceeds the supported maximum of %d tokens per reference" % (Ur, EDIT_MAX_U))


@torch.no_grad()
def edit_distance(hyps, hyp_lens, refs, ref_lens, n_hyp=None):
    """Error counts of hypotheses against references (csrc/edit_distance.hip): ``hyps`` int32 ``[B, N, Uh]``
    (``1 <= N <= 32``, ``Uh <= 1023``), ``hyp_lens`` int32 ``[B, N]``, ``refs`` int32 ``[B, Ur]`` (``Ur <= 1023``),
    ``ref_lens`` int32 ``[B]``, ``n_hyp`` int32 ``[B]`` (live slots per utterance; None: all ``N``) - the layout of
    ``loss.ctc_score_nbest``.  Plain pairs: ``hyps`` ``[B, Uh]`` with ``hyp_lens`` ``[B]``.  Contiguous device tensors
    only.  Returns an int32 device tensor ``[B, N, 4]`` (``[B, 4]`` for pairs) of ``(dist, sub, del, ins)`` as the
    module docstring defines them; ``-1`` in all four for the slots ``n >= n_hyp[b]``.  Lengths are clamped into
    ``[0, U]``; elements behind the lengths and slots behind ``n_hyp`` are never read.  ``Uh = 0`` / ``Ur = 0`` is
    legal.  One launch, one wave per ``(b, n)``; no gradient, no host sync, bit-identical from run to run."""
    pair = torch.is_tensor(hyps) and torch.is_tensor(hyp_lens) and hyps.dim() == 2 and hyp_lens.dim() == 1
    if pair:
        if n_hyp is not None:
            raise ValueError("n_hyp belongs to the [B,N,Uh] form: plain pairs have one hypothesis each")
        hyps, hyp_lens = hyps.unsqueeze(1), hyp_lens.unsqueeze(1)
    _certify_edit_distance_inputs(hyps, hyp_lens, refs, ref_lens, n_hyp)
    _lib.require_cuda(hyps, hyp_lens, refs, ref_lens, n_hyp)
    B, N, Uh = hyps.shape
    Ur = refs.shape[1]
    out = torch.empty(B, N, 4, dtype=torch.int32, device=hyps.device)
    _lib.call("edit_distance", hyps if Uh else None, hyp_lens, n_hyp, refs if Ur else None, ref_lens, B, N, Uh, Ur, out)
    return out[:, 0] if pair else out


def _seq(t, what):
    a = np.asarray(t)
    if a.size and a.dtype.kind not in "iu":
        raise TypeError("%s must hold integers, got %s" % (what, a.dtype))
    a = a.reshape(-1).astype(np.int64)
    if a.size > EDIT_MAX_U:
        raise ValueError("%s of %d elements exceeds the supported maximum of %d" % (what, a.size, EDIT_MAX_U))
    if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
        raise ValueError("%s holds a value outside int32" % what)
    return a


def _pack(hyp_lists, refs):
    """Host arrays of one kernel call: an utterance whose list is longer than 32 takes several rows (each with a copy
    of its reference).  Returns (host int32 buffer, (B, N, Uh, Ur), per utterance its (row, count) pieces) or None when
    there is no hypothesis at all."""
    pieces, rows = [], 0
    for seqs in hyp_lists:
        own = []
        for s in range(0, len(seqs), EDIT_MAX_N):
            own.append((rows, min(EDIT_MAX_N, len(seqs) - s)))
            rows += 1
        pieces.append(own)
    if rows == 0:
        return None
    B = rows
    N = max(c for own in pieces for _, c in own)
    Uh = max([t.size for seqs in hyp_lists for t in seqs], default=0)
    Ur = max([r.size for r, own in zip(refs, pieces) if own], default=0)
    # one buffer: hyps [B, N, Uh], refs [B, Ur], hyp_lens [B, N], ref_lens [B], n_hyp [B], back to back
    nh, nr, nl = B * N * Uh, B * Ur, B * N
    host = np.zeros(nh + nr + nl + 2 * B, dtype=np.int32)
    hyps, refa = host[:nh].reshape(B, N, Uh), host[nh:nh + nr].reshape(B, Ur)
    hyp_lens = host[nh + nr:nh + nr + nl].reshape(B, N)
    ref_lens, n_hyp = host[nh + nr + nl:nh + nr + nl + B], host[nh + nr + nl + B:]
    for seqs, r, own in zip(hyp_lists, refs, pieces):
        for k, (row, count) in enumerate(own):
            refa[row, :r.size] = r
            ref_lens[row] = r.size
            n_hyp[row] = count
            for n in range(count):
                t = seqs[k * EDIT_MAX_N + n]
                hyps[row, n, :t.size] = t
                hyp_lens[row, n] = t.size
    return host, (B, N, Uh, Ur), pieces


def edit_distance_lists(hyp_lists, refs, device=None):
    """Error counts of lists of hypotheses, from the host: ``hyp_lists[b]`` is a list of int sequences, ``refs[b]`` the
    one reference they are compared with (any int32 values, at most 1023 elements each).  ONE int32 upload holding all
    tokens and lengths back to back, ONE ``edit_distance`` call and ONE read.  Returns a list of int32 arrays
    ``[len(hyp_lists[b]), 4]`` of ``(dist, sub, del, ins)``.  A list longer than 32 is SPLIT over several rows of the
    same call (each with its own copy of the reference): there is no limit on the list length.  Without any hypothesis
    nothing is launched and the arrays are empty.  ``device``: where to run (None: the current HIP device)."""
    hyp_lists = [[_seq(t, "a hypothesis") for t in seqs] for seqs in hyp_lists]
    refs = [_seq(r, "a reference") for r in refs]
    if len(hyp_lists) != len(refs):
        raise ValueError("edit_distance_lists: %d lists for %d references" % (len(hyp_lists), len(refs)))
    packed = _pack(hyp_lists, refs)
    if packed is None:
        return [np.zeros((0, 4), dtype=np.int32) for _ in hyp_lists]
    host, (B, N, Uh, Ur), pieces = packed
    device = torch.device("cuda" if device is None else device)
    dev = torch.from_numpy(host).to(device)
    nh, nr, nl = B * N * Uh, B * Ur, B * N
    o = nh + nr + nl
    got = edit_distance(dev[:nh].view(B, N, Uh), dev[nh + nr:o].view(B, N), dev[nh:nh + nr].view(B, Ur), dev[o:o + B],
                        dev[o + B:]).cpu().numpy()
    return [np.concatenate([got[row, :count] for row, count in own], axis=0) if own
            else np.zeros((0, 4), dtype=np.int32) for own in pieces]


class ErrorRate:
    """Accumulator of an error rate whose seven totals live on the device as int64: errors, substitutions, deletions,
    insertions, reference length, number of sequences, number of sequences with at least one error.

    ``update(counts, ref_lens)`` adds the live rows of an ``edit_distance`` result (``counts`` ``[..., 4]``, ``ref_lens``
    the reference length of every row: ``[B]`` for ``[B, 4]`` and for ``[B, N, 4]``, where a reference counts once per
    live hypothesis; rows of -1 - the slots behind ``n_hyp`` - add nothing) with torch ops and without a host sync;
    ``compute()`` does the one read and returns an ``ErrorRateResult``; ``reset()`` clears the totals.  The tensors may
    live anywhere: the totals are created on the device of the first ``update`` (or on ``device=``)."""

    def __init__(self, device=None):
        self.device = None if device is None else torch.device(device)
        self.totals = None

    def reset(self):
        if self.totals is not None:
            self.totals.zero_()

    @torch.no_grad()
    def update(self, counts, ref_lens):
        if counts.dim() < 1 or counts.shape[-1] != 4:
            raise ValueError("counts must be [..., 4] rows of (dist, sub, del, ins), got %s" % (tuple(counts.shape),))
        if counts.dim() == 3 and ref_lens.dim() == 1:
            ref_lens = ref_lens.unsqueeze(1).expand(counts.shape[0], counts.shape[1])
        if tuple(ref_lens.shape) != tuple(counts.shape[:-1]):
            raise ValueError("must have a reference length per row (counts is %s, ref_lens %s)"
                             % (tuple(counts.shape), tuple(ref_lens.shape)))
        if self.totals is None:
            self.totals = torch.zeros(7, dtype=torch.int64, device=self.device or counts.device)
        rows = counts.reshape(-1, 4).to(device=self.totals.device, dtype=torch.int64)
        lens = ref_lens.reshape(-1).to(device=self.totals.device, dtype=torch.int64)
        live = (rows[:, 0] >= 0).to(torch.int64)
        add = torch.cat([(rows * live.unsqueeze(1)).sum(0), (lens * live).sum().reshape(1), live.sum().reshape(1),
                         (rows[:, 0] > 0).to(torch.int64).sum().reshape(1)])
        self.totals += add
        return self

    def compute(self):
        if self.totals is None:
            return _record(0, 0, 0, 0, 0, 0, 0)
        return _record(*self.totals.cpu().tolist())


def _rate_of(rows, refs):
    rows = np.concatenate([np.asarray(r, dtype=np.int64).reshape(-1, 4) for r in rows], axis=0) if rows \
        else np.zeros((0, 4), dtype=np.int64)
    return _record(rows[:, 0].sum(), rows[:, 1].sum(), rows[:, 2].sum(), rows[:, 3].sum(),
                   sum(len(r) for r in refs), rows.shape[0], (rows[:, 0] > 0).sum())


def token_error_rate(hyp_seqs, ref_seqs, device=None):
    """The error rate of token sequences, from the host: ``hyp_seqs[b]`` against ``ref_seqs[b]`` (int sequences), one
    ``edit_distance_lists`` call.  Returns an ``ErrorRateResult``: summed errors over summed reference tokens.  A
    character error rate is this function on character ids."""
    hyp_seqs, ref_seqs = list(hyp_seqs), list(ref_seqs)
    if len(hyp_seqs) != len(ref_seqs):
        raise ValueError("token_error_rate: %d hypotheses for %d references" % (len(hyp_seqs), len(ref_seqs)))
    refs = [_seq(r, "a reference") for r in ref_seqs]
    return _rate_of(edit_distance_lists([[h] for h in hyp_seqs], refs, device), refs)


def words_to_ids(hyp_texts, ref_texts):
    """The word sequences of two lists of sentences as int32 ids: a sentence is split on whitespace (``str.split()``:
    runs of blanks count once, empty words are dropped, an empty sentence is an empty sequence), every distinct word
    gets the next id of a dict built for this call.  No other text normalisation."""
    ids = {}

    def conv(text):
        if not isinstance(text, str):
            raise TypeError("a sentence must be a str, got %s" % type(text).__name__)
        return np.array([ids.setdefault(w, len(ids)) for w in text.split()], dtype=np.int64)

    return [conv(t) for t in hyp_texts], [conv(t) for t in ref_texts]


def word_error_rate(hyp_texts, ref_texts, device=None):
    """The word error rate of sentences, from the host: split on whitespace (``words_to_ids``; an empty reference is a
    legal row and contributes its hypothesis' words as insertions), then the same kernel as ``token_error_rate``.
    Returns an ``ErrorRateResult`` whose ``rate`` is the corpus-level figure - summed errors over summed reference
    words.  That is what the reference's ``jiwer.wer(true_seq, pred_seq)`` (cli/train.py:318) is understood to return
    for two lists of sentences; ``jiwer`` was not available where this was written, so this function is pinned against
    the Python oracle of the tests (tests/edit_distance_ref.py) and NOT against ``jiwer`` itself."""
    hyp_texts, ref_texts = list(hyp_texts), list(ref_texts)
    if len(hyp_texts) != len(ref_texts):
        raise ValueError("word_error_rate: %d hypotheses for %d references" % (len(hyp_texts), len(ref_texts)))
    hyps, refs = words_to_ids(hyp_texts, ref_texts)
    return token_error_rate(hyps, refs, device)


def nbest_errors(results, refs, device=None):
    """The error counts of every hypothesis of N-best lists: ``results`` one ``decode.NBestResult`` per utterance,
    ``refs[b]`` its reference tokens.  Returns one int32 ``[len(results[b]), 4]`` array per utterance (one
    ``edit_distance_lists`` call)."""
    results = list(results)
    return edit_distance_lists([r.tokens for r in results], refs, device)


def oracle_error_rate(results, refs, device=None):
    """The error rate of the best hypothesis of every list - what a perfect rescorer could reach: per utterance the
    hypothesis with the fewest errors, ties going to the lower index; an empty list counts as the empty hypothesis
    (every reference token deleted).  Returns ``(ErrorRateResult, indices)``, ``indices`` an int64 array (-1 for an
    empty list)."""
    refs = [_seq(r, "a reference") for r in refs]
    errs = nbest_errors(results, refs, device)
    rows, idx = [], np.full(len(errs), -1, dtype=np.int64)
    for b, (e, r) in enumerate(zip(errs, refs)):
        if e.shape[0] == 0:
            rows.append(np.array([[r.size, 0, r.size, 0]], dtype=np.int64))
            continue
        idx[b] = int(np.argmin(e[:, 0]))             # the first minimum
        rows.append(e[idx[b]][None])
    return _rate_of(rows, refs), idx


def expected_errors(results, refs, device=None):
    """``sum_n softmax(logp)_n * dist_n`` per utterance - the MWER risk of the list as a number (float64, on the host;
    no gradient, no training path).  A ``logp`` of -inf has weight 0; a list that is empty or whose ``logp`` are all
    -inf gives ``nan``.  Returns a float64 array ``[B]``."""
    results = list(results)
    errs = nbest_errors(results, refs, device)
    out = np.full(len(results), np.nan, dtype=np.float64)
    for b, (res, e) in enumerate(zip(results, errs)):
        logp = np.asarray(res.logp, dtype=np.float64)
        if logp.size == 0 or not np.isfinite(logp.max()):
            continue
        w = np.where(np.isneginf(logp), 0.0, np.exp(logp - logp.max()))
        out[b] = float((w * e[:, 0].astype(np.float64)).sum() / w.sum())
    return out
