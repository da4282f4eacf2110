"""GPU: the N-best CTC scorer (edgedict_ctc_score_nbest: one row pass per utterance, one alpha walk per hypothesis) and
CTC rescoring of the RNN-T searches' N-best lists, against the float64 oracle tests/ctc_score_ref.py (pinned on the CPU by
test_ctc_score_host.py).

Bound: the project's CTC cost bound (tests/test_ctc_gpu.py, tests/test_ctc_align_gpu.py) - fp32 rtol 1e-5 / atol 1e-4,
bf16 rtol 1e-4 / atol 1e-4 - the same arithmetic (fp32 log-sum-exp per frame, fp64 carry with an fp32 correction term);
for bf16 the oracle sees the rounded logits.  Cases: the construction of test_ctc_gpu._case (3-symbol alphabet, adjacent
repeats everywhere, V - 1 forced in once, logits 2 x normal), every length set deterministically.  Every test prints its
maximum error."""
import functools

import numpy as np
import pytest
import torch

import ctc_ref as CR
import ctc_score_ref as SR
from test_ctc_gpu import _model, _tiny

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
NEG = -np.inf

# (B, N, U, V): V = 29 takes the scalar row path; U = 31 / 32 sit on the lane boundary (63 / 65 states); U = 63 / 64
# straddle C = 2 -> 4 states per lane, U = 128 reaches C = 8; V = 4096 is the workload's vocabulary
SHAPES = [(1, 1, 0, 8), (1, 1, 1, 8), (3, 4, 5, 29), (2, 32, 31, 32), (2, 3, 32, 32), (2, 2, 63, 40), (2, 2, 64, 40),
          (2, 2, 128, 16), (2, 4, 9, 4096)]
SHAPE_IDS = ["%dx%dx%dx%d" % s for s in SHAPES]


def _need(y):
    return len(y) + CR.repeats(list(y))


def _fit(K, U):
    """A sequence of at most U tokens from {1, 2} with len + adjacent repeats == K; None if there is none."""
    if U < 1 or K < 1 or K > 2 * U - 1:
        return None
    if K <= U:
        return [1 + (i & 1) for i in range(K)]
    R = K - U
    return [1] * (R + 1) + [2 - (i & 1) for i in range(U - R - 1)]


@functools.lru_cache(maxsize=None)
def _case(B, N, U, V):
    """Slot 0 full length, slot 1 half, slot 2 empty, the further slots (5 ..) of lengths (7 n + 3 b) mod (U + 1);
    T = the largest U_n + repeats_n of those + 5.  Utterance 0 has T - 3 frames (B = 1: T) and NaN in its rows behind
    them, utterance 1 ONE frame (and, for N >= 8, only N - 8 live slots), utterance 2 no live slot.  Slot 3 is built to
    need exactly T_b frames (a single path), slot 4 to need T_b + 1 (no path) - where 2 U - 1 tokens-plus-repeats cannot
    reach that, the most the shape allows."""
    rng = np.random.default_rng(100000 * B + 1000 * N + 10 * U + V)
    hyps = rng.integers(1, 4, size=(B, N, U)).astype(np.int32)
    if U:
        hyps[0, 0, U // 2] = V - 1
    hl = np.zeros((B, N), dtype=np.int32)
    for b in range(B):
        for n in range(N):
            hl[b, n] = U if n == 0 else (U // 2 if n == 1 else (0 if n == 2 else (7 * n + 3 * b) % (U + 1)))
    regular = [_need(hyps[b, n, :hl[b, n]]) for b in range(B) for n in range(N) if n not in (3, 4)]
    T = max(regular) + 5
    act = np.full(B, T, dtype=np.int32)
    if B >= 2:
        act[0], act[1] = T - 3, 1
    nh = np.full(B, N, dtype=np.int32)
    if B >= 2 and N >= 8:
        nh[1] = N - 8
    if B >= 3:
        nh[2] = 0
    for b in range(B):
        for n, K in ((3, int(act[b])), (4, int(act[b]) + 1)):
            if n < N:
                seq = _fit(K, U) or _fit(min(K, 2 * U - 1), U) or []
                hyps[b, n, :len(seq)] = seq
                hl[b, n] = len(seq)
    z = (2.0 * rng.normal(size=(B, T, V))).astype(np.float32)
    return z, act, hyps, hl, nh


@functools.lru_cache(maxsize=None)
def _oracle(B, N, U, V, dtype):
    z, act, hyps, hl, nh = _case(B, N, U, V)
    seen = torch.tensor(z).to(dtype).double().numpy()                 # bf16: the oracle sees the rounded logits
    return SR.score_nbest(seen, act, hyps, hl, nh)


def _dev(*arrays):
    return [torch.tensor(np.ascontiguousarray(a), device="cuda") for a in arrays]


def _logits(z, act, dtype):
    """the device logits, NaN in every row t >= T_b: those rows are never read"""
    tz = torch.tensor(z, device="cuda").to(dtype)
    for b in range(z.shape[0]):
        tz[b, int(act[b]):] = float("nan")
    return tz


def _tol(dtype):
    return dict(rtol=1e-5, atol=1e-4) if dtype == F32 else dict(rtol=1e-4, atol=1e-4)


def _assert_scores(got, want, dtype, what):
    """-inf exactly where the oracle has it, no NaN, the finite values at the project's CTC cost bound"""
    assert got.dtype == np.float64 and got.shape == want.shape, what
    assert not np.isnan(got).any(), what
    fin = np.isfinite(want)
    assert ((got == NEG) == ~fin).all(), (what, got, want)
    if fin.any():
        err = np.abs(got[fin] - want[fin])
        print("ctc score", what, "max err %.3g (rel %.3g)" % (err.max(), (err / np.maximum(np.abs(want[fin]), 1e-30)).max()))
        np.testing.assert_allclose(got[fin], want[fin], **_tol(dtype))


@pytest.mark.parametrize("B,N,U,V", SHAPES, ids=SHAPE_IDS)
@DTYPES
def test_scores_against_the_oracle_the_loss_kernel_determinism_and_garbage(hip_lib, B, N, U, V, dtype):
    """Checks 1 - 4: the oracle; CTCLoss(reduction='none') rank by rank; two runs bit-identical; garbage behind n_hyp
    and behind hyp_lens changes nothing."""
    from edgedict_amd.loss import CTCLoss, ctc_score_nbest
    z, act, hyps, hl, nh = _case(B, N, U, V)
    T = z.shape[1]
    # which slots have a path, from the lengths and repeats alone
    path = np.zeros((B, N), dtype=bool)
    for b in range(B):
        for n in range(int(nh[b])):
            path[b, n] = SR.has_path(hyps[b, n, :hl[b, n]], int(act[b]))
    want = _oracle(B, N, U, V, dtype)
    assert (np.isfinite(want) == path).all()
    assert path[0, 0] and (B < 2 or not path[1, 0] or U <= 1) and (B < 3 or not path[2].any())
    needs = np.array([[_need(hyps[b, n, :hl[b, n]]) for n in range(N)] for b in range(B)])
    if N >= 4 and U >= 1:           # a single-path hypothesis: exactly T_b frames needed; on more than one frame too
        exact = (needs[:, 3] == act) & (nh > 3)
        assert exact.any() and path[exact, 3].all()
        assert U < 5 or exact[act > 1].any()
    if N >= 5:                      # one frame short: no path
        assert (needs[:, 4] == act + 1).all() and not path[:, 4].any()
    if B >= 2:
        assert act[0] == T - 3 and act[1] == 1

    tz = _logits(z, act, dtype)
    ta, th, tl, tn = _dev(act, hyps, hl, nh)
    got_t = ctc_score_nbest(tz, ta, th, tl, tn)
    assert got_t.dtype == torch.float64 and tuple(got_t.shape) == (B, N) and got_t.is_cuda
    got = got_t.cpu().numpy()
    _assert_scores(got, want, dtype, "%s %s T %d" % ((B, N, U, V), dtype, T))

    # 2. the existing kernel, rank by rank (every rank; the ranks whose live slots all have a path are among them)
    loss = CTCLoss(blank=0, reduction="none", check_lengths=False)
    equal_bits, compared, full_ranks = True, 0, 0
    for n in range(N):
        live = np.arange(B)[nh > n]
        if live.size == 0:
            continue
        cost = loss(tz, th[:, n].contiguous(), ta, tl[:, n].contiguous()).cpu().numpy()
        mine = got_t[:, n].float().cpu().numpy()
        full_ranks += bool(path[live, n].all())
        for b in live:
            if not path[b, n]:
                assert cost[b] == np.inf and mine[b] == NEG, (b, n)
                continue
            np.testing.assert_allclose(mine[b], -cost[b], **_tol(dtype))
            equal_bits &= bool(mine[b] == -cost[b])
            compared += 1
    assert compared >= 1
    print("ctc score vs CTCLoss", (B, N, U, V), dtype, "%d slots compared (%d ranks with a path in every live slot), "
          "bit-equal after the float cast: %s" % (compared, full_ranks, equal_bits))

    # 3. determinism
    assert torch.equal(ctc_score_nbest(tz, ta, th, tl, tn), got_t)

    # 4. out-of-range garbage behind n_hyp and behind hyp_lens
    dirty, dirty_l = hyps.copy(), hl.copy()
    for b in range(B):
        for n in range(N):
            if n >= nh[b]:
                dirty[b, n] = -7 if (b + n) & 1 else 10 ** 9
                dirty_l[b, n] = 10 ** 6 if n & 1 else -3
            else:
                dirty[b, n, hl[b, n]:] = 10 ** 9 if (b + n) & 1 else -7
    td, tdl = _dev(dirty, dirty_l)
    assert torch.equal(ctc_score_nbest(tz, ta, td, tdl, tn), got_t)

    # n_hyp=None: all N slots live - the utterances whose slots all were see the same bits
    all_t = ctc_score_nbest(tz, ta, th, tl)
    every = SR.score_nbest(torch.tensor(z).to(dtype).double().numpy(), act, hyps, hl, None)
    _assert_scores(all_t.cpu().numpy(), every, dtype, "n_hyp=None")
    for b in range(B):
        if nh[b] == N:
            assert torch.equal(all_t[b], got_t[b])


def test_a_token_outside_the_vocabulary_has_no_path(hip_lib):
    from edgedict_amd.loss import ctc_score_nbest
    z, act, hyps, hl, nh = _case(3, 4, 5, 29)
    base = ctc_score_nbest(_logits(z, act, F32), *_dev(act, hyps, hl, nh))
    bad = hyps.copy()
    bad[0, 0, 1], bad[0, 1, 0] = 29, -1
    got = ctc_score_nbest(_logits(z, act, F32), *_dev(act, bad, hl, nh))
    assert got[0, 0].item() == NEG and got[0, 1].item() == NEG and not torch.isnan(got).any()
    keep = torch.ones_like(base, dtype=torch.bool)
    keep[0, :2] = False
    assert torch.equal(got[keep], base[keep]) and torch.isfinite(base[0, :2]).all()


def test_workspace_does_not_grow_with_the_hypotheses(hip_lib):
    """Check 5: the workspace is equal for two values of U (and of N) and below 4096 + 16 B T bytes."""
    for B, N, U, V in SHAPES:
        T = _case(B, N, U, V)[0].shape[1]
        n = hip_lib.edgedict_ctc_score_workspace_bytes(B, T, N, U)
        assert n == hip_lib.edgedict_ctc_score_workspace_bytes(B, T, N, U + 100)
        assert n == hip_lib.edgedict_ctc_score_workspace_bytes(B, T, 32, 0)
        assert 0 < n < 4096 + 16 * B * T


# --------------------------------------------------------------------------------------------------- model level
W, WEIGHT, THR = 4, 0.3, 0.9
EM = 400        # the unsharpened tiny model's best-first search needs more than the default 8 W pops on some frames
                # (tests/test_nbest_gpu.py's value)


def _search_fn(s, search):
    """The model's search, run as inference code runs it: under ``torch.no_grad()``.  ``Transducer.beam_search_nbest``
    does not switch autograd off itself, and with autograd on the bf16 encoder takes its training path on these short
    utterances, whose output differs from the inference path's by bf16 roundings - the oracle, ``ctc_score`` and the
    frame-synchronous search all see the inference path's."""
    fn = getattr(s.m, search)
    if search == "beam_search_nbest":
        fn = functools.partial(fn, max_expansions=EM)

    def run(*args, **kw):
        with torch.no_grad():
            return fn(*args, **kw)

    return run


class _Setup:
    """The tiny LSTM model (tests/golden/transducer_tiny.npz's weights) with a CTC head whose blank bias puts the median
    frame's blank posterior on THR, its batch of 3 ragged utterances, and its own head logits read to the host."""

    def __init__(self, cd):
        cfg, sd, (xs, ys, xlen, ylen) = _tiny("tiny")
        m = _model(cfg, sd, cd, 0.3, output_loss=False).eval()
        self.m, self.xs, self.xlen, self.cfg, self.sd = m, xs.cuda(), xlen, cfg, sd
        assert xs.shape[0] == 3 and len(set(xlen.tolist())) > 1
        with torch.no_grad():
            enc, _ = m.encoder(self.xs)
            self.enc = enc.contiguous()
            self.lens = m.scale_length(self.enc, xlen).numpy().astype(np.int32)
            z = m._ctc_logits(self.enc).double().cpu().numpy()
            zm = z[:, :, 1:].max(axis=2)
            odds = z[:, :, 0] - (zm + np.log(np.exp(z[:, :, 1:] - zm[:, :, None]).sum(axis=2)))
            live = np.arange(z.shape[1])[None, :] < self.lens[:, None]
            m.ctc_head.bias[0] += float(np.log(THR / (1.0 - THR)) - np.median(odds[live]))
            self.logits = m._ctc_logits(self.enc).double().cpu().numpy()

    def oracle(self, b, tokens):
        return SR.score_one(self.logits[b, :int(self.lens[b])], tokens, self.m.blank)


@functools.lru_cache(maxsize=None)
def _setup(cd):
    return _Setup(cd)


def _check_ctc_logp(s, results, dtype, what):
    worst = 0.0
    for b, r in enumerate(results):
        assert r.ctc_logp is not None and r.ctc_logp.shape == (len(r),) and r.ctc_logp.dtype == np.float64
        want = np.array([s.oracle(b, t) for t in r.tokens])
        assert not np.isnan(r.ctc_logp).any()
        fin = np.isfinite(want)
        assert ((r.ctc_logp == NEG) == ~fin).all(), (what, b)
        np.testing.assert_allclose(r.ctc_logp[fin], want[fin], **_tol(dtype))
        if fin.any():
            worst = max(worst, np.abs(r.ctc_logp[fin] - want[fin]).max())
    print("ctc rescore", what, dtype, "max ctc_logp err %.3g" % worst)


def _same_lists(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert len(x) == len(y) and np.array_equal(x.logp, y.logp)
        for i in range(len(x)):
            assert np.array_equal(x.tokens[i], y.tokens[i]) and np.array_equal(x.frames[i], y.frames[i])
            assert np.array_equal(x.token_logp[i], y.token_logp[i])


@pytest.mark.parametrize("search", ["sync_beam_search_nbest", "beam_search_nbest"])
@pytest.mark.parametrize("cd", ["fp32", "bf16"])
def test_searches_rescore_their_lists(hip_lib, cd, search):
    """``ctc_rescore=0.3``: ctc_logp against the oracle on the model's own head logits; the hypotheses, their frames and
    their first-pass scores are the plain search's; the order is the stable sort of the returned combined scores;
    ``ctc_rescore=None`` is the plain search bit for bit; ``Transducer.ctc_score`` gives the same numbers."""
    s = _setup(cd)
    dtype = F32 if cd == "fp32" else BF16
    fn = _search_fn(s, search)
    plain = fn(s.xs, s.xlen, W)
    assert all(r.ctc_logp is None for r in plain)
    _same_lists(fn(s.xs, s.xlen, W, ctc_rescore=None), plain)
    got = fn(s.xs, s.xlen, W, ctc_rescore=WEIGHT)
    assert len(got) == 3
    _check_ctc_logp(s, got, dtype, search)
    finite = 0
    for b, (r, p) in enumerate(zip(got, plain)):
        assert len(r) == len(p) >= 1
        # the multiset of (tokens, frames, first-pass logp)
        key = lambda q, i: (tuple(q.tokens[i].tolist()), tuple(q.frames[i].tolist()))
        mine = sorted(range(len(r)), key=lambda i: key(r, i))
        theirs = sorted(range(len(p)), key=lambda i: key(p, i))
        for i, j in zip(mine, theirs):
            assert key(r, i) == key(p, j), b
            assert r.tokens[i].dtype == np.int64 and r.frames[i].dtype == p.frames[j].dtype
            assert np.array_equal(r.token_logp[i], p.token_logp[j])
            if np.isfinite(r.ctc_logp[i]):
                finite += 1
                np.testing.assert_allclose(r.logp[i] - WEIGHT * r.ctc_logp[i], p.logp[j], rtol=1e-12)
                assert r.logp[i] == p.logp[j] + WEIGHT * r.ctc_logp[i]          # exactly that expression
            else:
                assert r.logp[i] == NEG
        assert (r.logp[:-1] >= r.logp[1:]).all(), b
        # the order: the stable sort of the engine's own combined values over the plain search's order
        comb, order = SR.combine(p.logp, [r.ctc_logp[mine[theirs.index(j)]] for j in range(len(p))], WEIGHT)
        assert np.array_equal(comb[order], r.logp), b
        assert [p.tokens[j].tolist() for j in order] == [t.tolist() for t in r.tokens], b
        assert [p.frames[j].tolist() for j in order] == [f.tolist() for f in r.frames], b
    assert finite >= 3
    # Transducer.ctc_score on the same hypotheses
    scores = s.m.ctc_score(s.xs, s.xlen, [r.tokens for r in got])
    for r, sc in zip(got, scores):
        assert sc.dtype == np.float64 and np.array_equal(sc, r.ctc_logp)
    # weight 0: the scores are the plain search's, ctc_logp is filled, the order the stable sort of logp
    zero = fn(s.xs, s.xlen, W, ctc_rescore=0.0)
    for r, p in zip(zero, plain):
        order = SR.combine(p.logp, np.zeros(len(p)), 0.0)[1]
        assert np.array_equal(r.logp, p.logp[order]) and r.ctc_logp is not None


@pytest.mark.parametrize("search", ["sync_beam_search_nbest", "beam_search_nbest"])
@pytest.mark.parametrize("cd", ["fp32", "bf16"])
def test_rescoring_with_skipped_blank_frames(hip_lib, cd, search):
    """``skip_blank=0.9`` with ``ctc_rescore=0.3``: the head scores the UNSKIPPED encoder output - ctc_logp is the
    oracle's on all frames and equals the unskipped run's for the same token sequences - and frames are in the original
    numbering."""
    from edgedict_amd.decode import skip_blank_frames
    s = _setup(cd)
    dtype = F32 if cd == "fp32" else BF16
    fn = _search_fn(s, search)
    got = fn(s.xs, s.xlen, W, skip_blank=THR, ctc_rescore=WEIGHT)
    plain = fn(s.xs, s.xlen, W, skip_blank=THR)
    full = fn(s.xs, s.xlen, W, ctc_rescore=WEIGHT)
    _check_ctc_logp(s, got, dtype, search + " skip_blank")
    with torch.no_grad():
        sk = skip_blank_frames(s.m, s.enc, s.lens, THR)
    assert (sk.lens < s.lens).any() and sk.lens.sum() > 0              # frames were dropped, and not all of them
    shared = 0
    for b, (r, p) in enumerate(zip(got, plain)):
        kept = set(sk.frame_map[b, :int(sk.lens[b])].tolist())
        assert sorted(tuple(t.tolist()) for t in r.tokens) == sorted(tuple(t.tolist()) for t in p.tokens)
        for i in range(len(r)):
            f = r.frames[i].tolist()
            assert set(f) <= kept and all(0 <= t < s.lens[b] for t in f) and f == sorted(f), (b, i)
            j = [k for k in range(len(p)) if np.array_equal(p.tokens[k], r.tokens[i])
                 and np.array_equal(p.frames[k], r.frames[i])]
            assert j, (b, i)
            for k in range(len(full[b])):
                if np.array_equal(full[b].tokens[k], r.tokens[i]):
                    shared += 1
                    assert full[b].ctc_logp[k] == r.ctc_logp[i]
        assert (r.logp[:-1] >= r.logp[1:]).all()
    print("ctc rescore + skip_blank", search, cd, "kept", sk.lens.tolist(), "of", s.lens.tolist(),
          "- %d token sequences shared with the unskipped run" % shared)


@pytest.mark.parametrize("cd", ["fp32", "bf16"])
def test_rescore_nbest_on_ctc_beam_search_lists_and_the_missing_head(hip_lib, cd):
    s = _setup(cd)
    dtype = F32 if cd == "fp32" else BF16
    first = s.m.ctc_beam_search(s.xs, s.xlen, W=W, cand=8)
    got = s.m.rescore_nbest(s.xs, s.xlen, first, WEIGHT)
    _check_ctc_logp(s, got, dtype, "rescore_nbest(ctc_beam_search)")
    for r, p in zip(got, first):
        assert len(r) == len(p) and np.isfinite(r.ctc_logp).all()
        comb, order = SR.combine(p.logp, [r.ctc_logp[[np.array_equal(t, p.tokens[j]) for t in r.tokens].index(True)]
                                          for j in range(len(p))], WEIGHT)
        assert np.array_equal(comb[order], r.logp)
        # a prefix' beam score is a lower bound of its full CTC likelihood (the beam prunes paths) up to rounding
        for j in range(len(p)):
            i = [np.array_equal(t, p.tokens[j]) for t in r.tokens].index(True)
            assert p.logp[j] <= r.ctc_logp[i] + 1e-3
    # an empty list stays empty, and a second pass over rescored lists works on the combined score
    from edgedict_amd.decode import NBestResult
    mixed = [NBestResult([], [], [], []), first[1], first[2]]
    out = s.m.rescore_nbest(s.xs, s.xlen, mixed, WEIGHT)
    assert len(out[0]) == 0 and out[0].ctc_logp.shape == (0,)
    assert np.array_equal(out[1].ctc_logp, got[1].ctc_logp) and np.array_equal(out[2].logp, got[2].logp)
    plain = _model(s.cfg, s.sd, cd, 0.0, output_loss=False).eval()
    for call in (lambda: plain.sync_beam_search_nbest(s.xs, s.xlen, W, ctc_rescore=WEIGHT),
                 lambda: plain.beam_search_nbest(s.xs, s.xlen, W, ctc_rescore=WEIGHT),
                 lambda: plain.rescore_nbest(s.xs, s.xlen, first, WEIGHT),
                 lambda: plain.ctc_score(s.xs, s.xlen, [r.tokens for r in first])):
        with pytest.raises(RuntimeError, match="no CTC head"):
            call()
