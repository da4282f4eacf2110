"""GPU: the batched edit-distance kernel (edgedict_edit_distance: one wave64 per (b, n), C reference columns per lane)
and the error rates built on it, against the integer oracle tests/edit_distance_ref.py (pinned on the CPU by
test_edit_distance_host.py).  The quantity is an integer: every comparison is an equality, nothing has a tolerance."""
import functools

import numpy as np
import pytest
import torch

import edit_distance_ref as ER
from test_ctc_gpu import _flags, _model, _tiny

pytestmark = pytest.mark.gpu

# (B, N, Uh, Ur).  The kernel picks C = 1 / 2 / 4 / 8 / 16 reference columns per lane for Ur <= 64 / 128 / 256 / 512 /
# 1023: Ur = 64|65, 128|129, 256|257, 512|513 sit on either side of every switch; Ur = 63 / 65 / 127 / 511 leave the last
# lane partly or wholly idle; Uh = 64|65, 129, 130 cross the 64-token blocks the hypothesis is read in.
SHAPES = [(1, 1, 0, 0), (1, 1, 0, 5), (1, 1, 5, 0), (1, 1, 1, 1), (3, 4, 7, 5), (2, 32, 33, 31), (2, 3, 40, 63),
          (2, 3, 40, 64), (2, 3, 40, 65), (2, 2, 64, 127), (2, 2, 130, 128), (2, 2, 129, 129), (2, 2, 300, 256),
          (2, 2, 65, 257), (2, 2, 257, 511), (2, 6, 40, 512), (2, 6, 40, 513), (3, 6, 9, 7), (4, 12, 80, 70),
          (1, 2, 1023, 1023), (1, 1, 1, 1023), (1, 1, 1023, 1)]
SHAPE_IDS = ["%dx%dx%dx%d" % s for s in SHAPES]


def _max_ins(h, r):
    """(dist, the MOST insertions a minimum-distance alignment can have): above the oracle's count iff the tie between
    an insertion plus a deletion and two substitutions occurs."""
    H, R = len(h), len(r)
    prev = [(j, 0) for j in range(R + 1)]
    for i in range(1, H + 1):
        cur = [(i, -i)]
        for j in range(1, R + 1):
            d = prev[j - 1] if h[i - 1] == r[j - 1] else (prev[j - 1][0] + 1, prev[j - 1][1])
            cur.append(min(d, (prev[j][0] + 1, prev[j][1] - 1), (cur[j - 1][0] + 1, cur[j - 1][1])))
        prev = cur
    return prev[R][0], -prev[R][1]


@functools.lru_cache(maxsize=None)
def _case(B, N, Uh, Ur):
    """A 3-symbol alphabet {1, 2, 3}, so hits and ties are frequent.  Slot 0 has full length, slot 1 half, slot 2 is
    empty, slot 3 equals the reference (cut to Uh), slot 4 is the reference with its first symbol deleted and a symbol
    inserted behind its second (the tie: one deletion plus one insertion against two substitutions), slot 5 is from a
    disjoint alphabet (all substitutions), the further slots have the lengths (7 n + 3 b) mod (Uh + 1).  Utterance 0
    has the full reference; utterance 1 an empty one when B = 2, half of it when B >= 3 - and only N - 8 live slots
    where N >= 8; utterance 2 has no live slot; utterance 3 an empty reference."""
    rng = np.random.default_rng(1000003 * B + 10007 * N + 1031 * Uh + Ur)
    hyps = rng.integers(1, 4, size=(B, N, Uh)).astype(np.int32)
    refs = rng.integers(1, 4, size=(B, Ur)).astype(np.int32)
    if Ur >= 2:
        refs[:, 0], refs[:, 1] = 1, 2
    rl = np.full(B, Ur, dtype=np.int32)
    if B == 2:
        rl[1] = 0
    if B >= 3:
        rl[1] = Ur // 2
    if B >= 4:
        rl[3] = 0
    nh = np.full(B, N, dtype=np.int32)
    if B >= 2 and N >= 8:
        nh[1] = N - 8
    if B >= 3:
        nh[2] = 0
    hl = np.zeros((B, N), dtype=np.int32)
    for b in range(B):
        R = int(rl[b])
        for n in range(N):
            hl[b, n] = Uh if n == 0 else (Uh // 2 if n == 1 else (0 if n == 2 else (7 * n + 3 * b) % (Uh + 1)))
        if N > 3:
            k = min(R, Uh)
            hyps[b, 3, :k], hl[b, 3] = refs[b, :k], k
        if N > 4 and R >= 2:
            seq = np.concatenate([refs[b, 1:2], [3], refs[b, 2:R]])[:Uh]       # [1, 2, rest] -> [2, 3, rest]
            hyps[b, 4, :seq.size], hl[b, 4] = seq, seq.size
        if N > 5:
            k = min(R, Uh)
            hyps[b, 5, :k], hl[b, 5] = rng.integers(7, 10, size=k), k
    return hyps, hl, nh, refs, rl


@functools.lru_cache(maxsize=None)
def _oracle(B, N, Uh, Ur):
    return ER.counts_nbest(*_case(B, N, Uh, Ur))


def _dev(*arrays):
    return [None if a is None else torch.tensor(np.ascontiguousarray(a), device="cuda") for a in arrays]


def _run(hyps, hl, nh, refs, rl):
    from edgedict_amd.metrics import edit_distance
    th, tl, tn, tr, trl = _dev(hyps, hl, nh, refs, rl)
    return edit_distance(th, tl, tr, trl, tn)


def test_the_case_holds_what_it_promises():
    """On the CPU: the tie of slot 4 occurs (a minimum-distance alignment with more insertions than the one the rule
    picks exists), slot 3 has no error, slot 5 only substitutions; the dead and empty rows are there."""
    ties = 0
    for shape in SHAPES:
        B, N, Uh, Ur = shape
        hyps, hl, nh, refs, rl = _case(*shape)
        want = _oracle(*shape)
        for b in range(B):
            R = int(rl[b])
            if N > 3 and nh[b] > 3 and Uh >= R:
                assert want[b, 3].tolist() == [0, 0, 0, 0]
            if N > 4 and nh[b] > 4 and Uh >= R >= 2 and R <= 130:
                h, r = hyps[b, 4, :hl[b, 4]].tolist(), refs[b, :R].tolist()
                dist, most = _max_ins(h, r)
                assert want[b, 4].tolist() == [2, 2, 0, 0] and dist == 2 and most == 1, shape
                ties += 1
            if N > 5 and nh[b] > 5 and Uh >= R:
                assert want[b, 5].tolist() == [R, R, 0, 0]
    assert ties >= 3
    assert (_case(4, 12, 80, 70)[4] == [70, 35, 70, 0]).all() and (_case(4, 12, 80, 70)[2] == [12, 4, 0, 12]).all()
    assert (_case(2, 32, 33, 31)[2] == [32, 24]).all() and (_case(2, 3, 40, 64)[4] == [64, 0]).all()


@pytest.mark.parametrize("B,N,Uh,Ur", SHAPES, ids=SHAPE_IDS)
def test_counts_equal_the_oracle_twice_and_with_garbage_behind_the_lengths(hip_lib, B, N, Uh, Ur):
    """The oracle; two runs bit-identical; the memory behind hyp_lens / ref_lens and the dead slots filled with symbols
    that are live on the other side: nothing changes, dead slots return -1; n_hyp = None: all N slots live."""
    hyps, hl, nh, refs, rl = _case(B, N, Uh, Ur)
    want = _oracle(B, N, Uh, Ur)
    got_t = _run(hyps, hl, nh, refs, rl)
    assert got_t.dtype == torch.int32 and tuple(got_t.shape) == (B, N, 4) and got_t.is_cuda
    got = got_t.cpu().numpy()
    assert np.array_equal(got, want), (got, want)
    for b in range(B):
        assert (got[b, int(nh[b]):] == -1).all()
        live = got[b, :int(nh[b])]
        assert (live >= 0).all() and (live[:, 0] == live[:, 1:].sum(axis=1)).all()
        assert (live[:, 3] - live[:, 2] == hl[b, :int(nh[b])] - rl[b]).all()
    assert torch.equal(_run(hyps, hl, nh, refs, rl), got_t)
    # garbage: behind a hypothesis the reference's own continuation, behind the reference a live hypothesis symbol
    bad_h, bad_hl, bad_r = hyps.copy(), hl.copy(), refs.copy()
    for b in range(B):
        R = int(rl[b])
        for n in range(N):
            if n >= nh[b]:
                bad_h[b, n], bad_hl[b, n] = (refs[b, :1] if Ur else 1), Uh
            else:
                k = int(hl[b, n])
                tail = np.resize(refs[b, k:] if k < Ur else refs[b], Uh - k) if Ur else 2
                bad_h[b, n, k:] = tail
        if Uh and Ur:
            bad_r[b, R:] = np.resize(hyps[b, 0, R:] if R < Uh else hyps[b, 0], Ur - R)
    assert torch.equal(_run(bad_h, bad_hl, nh, bad_r, rl), got_t)
    # every slot live
    all_t = _run(hyps, hl, None, refs, rl).cpu().numpy()
    assert np.array_equal(all_t, ER.counts_nbest(hyps, hl, None, refs, rl))


def test_every_int32_value_is_a_symbol(hip_lib):
    lo, hi = -2 ** 31, 2 ** 31 - 1
    table = np.array([hi, lo, -1, 0, hi, hi, hi, hi, hi, hi], dtype=np.int64)
    for shape in ((3, 6, 9, 7), (2, 6, 40, 65)):
        hyps, hl, nh, refs, rl = _case(*shape)
        mh, mr = table[hyps].astype(np.int32), table[refs].astype(np.int32)
        assert {lo, -1, 0, hi} <= set(mh.reshape(-1).tolist()) | set(mr.reshape(-1).tolist())
        got = _run(mh, hl, nh, mr, rl).cpu().numpy()
        assert np.array_equal(got, ER.counts_nbest(mh, hl, nh, mr, rl))


def test_lengths_are_clamped_and_pairs_equal_one_slot(hip_lib):
    from edgedict_amd.metrics import edit_distance
    hyps, hl, nh, refs, rl = _case(3, 4, 7, 5)
    wild_hl, wild_rl, wild_nh = hl.copy(), rl.copy(), nh.copy()
    wild_hl[0, 0], wild_hl[0, 1], wild_rl[0], wild_rl[1], wild_nh[0], wild_nh[1] = 7 + 9, -3, 5 + 100, -1, 4 + 7, -2
    got = _run(hyps, wild_hl, wild_nh, refs, wild_rl).cpu().numpy()
    assert np.array_equal(got, ER.counts_nbest(hyps, wild_hl, wild_nh, refs, wild_rl))
    assert (got[1] == -1).all() and (got[0] >= 0).all()
    # the pair form [B, Uh] / [B] is the N = 1 call
    for shape in ((3, 4, 7, 5), (2, 3, 40, 65)):
        hyps, hl, nh, refs, rl = _case(*shape)
        th, tl, tr, trl = _dev(hyps[:, 0], hl[:, 0], refs, rl)
        pair = edit_distance(th, tl, tr, trl)
        assert tuple(pair.shape) == (shape[0], 4)
        assert torch.equal(pair, edit_distance(th.unsqueeze(1).contiguous(), tl.unsqueeze(1).contiguous(), tr, trl)[:, 0])
        assert np.array_equal(pair.cpu().numpy(), ER.counts_nbest(hyps[:, :1], hl[:, :1], None, refs, rl)[:, 0])


def test_lists_from_the_host_and_the_accumulator(hip_lib):
    """``edit_distance_lists`` (ragged lists, a list of 40 split over two rows, an empty list, empty sequences) and
    ``ErrorRate`` over two updates against the oracle's totals."""
    from edgedict_amd import metrics
    rng = np.random.default_rng(5)
    seq = lambda n: rng.integers(0, 3, size=n)
    lists = [[seq(5), seq(0), seq(9)], [], [seq(rng.integers(0, 12)) for _ in range(40)], [seq(3)]]
    refs = [seq(6), seq(4), seq(8), seq(0)]
    got = metrics.edit_distance_lists(lists, refs)
    assert [g.shape for g in got] == [(3, 4), (0, 4), (40, 4), (1, 4)]
    for g, seqs, r in zip(got, lists, refs):
        assert g.dtype == np.int32
        assert np.array_equal(g, np.array([ER.counts_fast(h, r) for h in seqs], dtype=np.int32).reshape(-1, 4))
    rec = metrics.token_error_rate([l[0] for l in lists if l], [r for l, r in zip(lists, refs) if l])
    rows = [g[0] for g in got if g.shape[0]]
    want = ER.totals(rows, [len(r) for l, r in zip(lists, refs) if l])
    assert all(getattr(rec, k) == v for k, v in want.items())
    assert rec.rate == want["errors"] / want["ref_len"]
    rec = metrics.word_error_rate(["a  b c", "", "x"], ["a c", "d e", ""])
    assert (rec.errors, rec.substitutions, rec.deletions, rec.insertions, rec.ref_len) == (4, 0, 2, 2, 4)
    # the accumulator on the device: a pair result and an N-best result with dead slots
    acc = metrics.ErrorRate()
    a, b = (3, 4, 7, 5), (2, 32, 33, 31)
    rows, lens = [], []
    for shape in (a, b):
        hyps, hl, nh, refs_, rl = _case(*shape)
        out = _run(hyps, hl, nh, refs_, rl)
        acc.update(out, torch.tensor(rl, device="cuda"))
        want = _oracle(*shape)
        for bb in range(shape[0]):
            rows += want[bb, :int(nh[bb])].tolist()
            lens += [int(rl[bb])] * int(nh[bb])
    assert acc.totals.is_cuda and acc.totals.dtype == torch.int64
    rec, want = acc.compute(), ER.totals(rows, lens)
    assert all(getattr(rec, k) == v for k, v in want.items()), (rec, want)
    acc.reset()
    assert acc.compute().sequences == 0


class _Words:
    """A stub of the reference's tokenizer: ``decode_plus`` maps every token to a word."""

    def decode_plus(self, batch):
        return [" ".join("w%d" % int(t) for t in tokens) for tokens in batch]


def _word_counts(pred, true):
    ids = {}
    conv = lambda s: [ids.setdefault(w, len(ids)) for w in s.split()]
    rows = [ER.counts(conv(p), conv(t)) for p, t in zip(pred, true)]
    return ER.totals(rows, [len(t.split()) for t in true])


@functools.lru_cache(maxsize=None)
def _setup():
    cfg, sd, (xs, ys, xlen, ylen) = _tiny("tiny")
    m = _model(cfg, sd, "fp32", 0.3).eval()
    refs = [ys[b, :int(ylen[b])].numpy().astype(np.int64) for b in range(ys.shape[0])]
    return m, xs.cuda(), ys.cuda(), xlen, ylen, refs


@pytest.mark.parametrize("search", ["sync_beam_search_nbest", "ctc_beam_search"])
def test_nbest_lists_errors_oracle_rate_and_risk(hip_lib, search):
    from edgedict_amd import metrics
    m, xs, ys, xlen, ylen, refs = _setup()
    with torch.no_grad():
        results = getattr(m, search)(xs, xlen, 4)
    assert sum(len(r) for r in results) > len(results)
    want = [np.array([ER.counts_fast(t, r) for t in res.tokens], dtype=np.int32).reshape(-1, 4)
            for res, r in zip(results, refs)]
    for got in (metrics.nbest_errors(results, refs), metrics.edit_distance_lists([r.tokens for r in results], refs)):
        assert len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want))
    rec, idx = metrics.oracle_error_rate(results, refs)
    best = [int(np.argmin(w[:, 0])) for w in want]
    assert idx.tolist() == best
    tot = ER.totals([w[i] for w, i in zip(want, best)], [len(r) for r in refs])
    assert all(getattr(rec, k) == v for k, v in tot.items())
    first = metrics.token_error_rate([r.tokens[0] for r in results], refs)
    assert rec.errors <= first.errors
    risk = metrics.expected_errors(results, refs)
    for b, (res, w) in enumerate(zip(results, want)):
        p = np.exp(res.logp - res.logp.max())
        assert risk.dtype == np.float64 and risk[b] == (p * w[:, 0]).sum() / p.sum()
        # a weighted mean lies between the extremes up to its own float64 roundings: n products, two sums of n terms
        # and one division, each within 2^-53 relative (all terms are >= 0, nothing cancels)
        slack = (2 * len(res) + 2) * 2.0 ** -53
        assert w[:, 0].min() * (1 - slack) <= risk[b] <= w[:, 0].max() * (1 + slack)


@pytest.mark.parametrize("search,kw", [("greedy", {}), ("ctc_greedy", {}), ("beam", dict(W=4, max_expansions=400)),
                                       ("sync_beam", dict(W=4))], ids=["greedy", "ctc_greedy", "beam", "sync_beam"])
def test_model_evaluate_step(hip_lib, search, kw):
    """The loss is ``forward``'s, the hypotheses the named search's, the rate the oracle's on the returned sequences -
    tokens without a tokenizer, words with one."""
    m, xs, ys, xlen, ylen, refs = _setup()
    with torch.no_grad():
        want_loss = float(m(xs, ys, xlen, ylen))
        if search == "greedy":
            hyp = [s[s != m.blank] for s in m.greedy_decode(xs, xlen)[0]]
        elif search == "ctc_greedy":
            hyp = m.ctc_greedy_decode(xs, xlen)[0]
        elif search == "beam":
            hyp = m.beam_search(xs, xlen, **kw)[0]
        else:
            hyp = m.sync_beam_search(xs, xlen, **kw)[0]
    loss, rate, pred, true = m.evaluate_step(xs, ys, xlen, ylen, search=search, **kw)
    assert isinstance(loss, float) and loss == want_loss
    assert len(pred) == len(true) == len(refs)
    assert all(np.array_equal(p, h) for p, h in zip(pred, hyp)) and all(np.array_equal(t, r) for t, r in zip(true, refs))
    tot = ER.totals([ER.counts_fast(p, t) for p, t in zip(pred, true)], [len(t) for t in true])
    assert rate == tot["errors"] / tot["ref_len"]
    assert all(getattr(m.last_error_rate, k) == v for k, v in tot.items())
    assert not m.training
    loss2, wrate, wpred, wtrue = m.evaluate_step(xs, ys, xlen, ylen, search=search, tokenizer=_Words(), **kw)
    assert loss2 == want_loss and wpred == _Words().decode_plus(hyp) and wtrue == _Words().decode_plus(refs)
    wtot = _word_counts(wpred, wtrue)
    assert wrate == wtot["errors"] / wtot["ref_len"]
    assert all(getattr(m.last_error_rate, k) == v for k, v in wtot.items())
    assert wtot["errors"] == tot["errors"]           # one word per token


def test_train_engine_evaluate_leaves_training_untouched(hip_lib):
    """``evaluate`` returns the reference's means (of batch losses, of batch rates), ``last_eval`` the corpus-level
    record; a ``train_step`` after it gives the loss of a ``train_step`` without it, bit for bit."""
    from edgedict_amd.trainer import TrainEngine
    g = torch.Generator(device="cpu").manual_seed(5)
    wave = (0.1 * torch.randn(4, 9600, generator=g)).cuda()
    ys = torch.randint(4, 40, (4, 6), generator=g, dtype=torch.int32).cuda()
    ylen = torch.tensor([6, 4, 5, 6], dtype=torch.int32)
    wave2 = (0.1 * torch.randn(2, 6400, generator=g)).cuda()
    ys2 = torch.randint(4, 40, (2, 3), generator=g, dtype=torch.int32).cuda()
    ylen2 = torch.tensor([3, 2], dtype=torch.int32)
    batches = [(wave, None, ys, ylen), (wave2, None, ys2, ylen2)]
    torch.manual_seed(0)
    a = TrainEngine(_flags(0.3), vocab_size=40, device="cuda", compute_dtype="fp32")
    try:
        sd = {k: v.detach().clone() for k, v in a.model.state_dict().items()}
        want = a.train_step(wave, None, ys, ylen).clone()
        want2 = a.train_step(wave2, None, ys2, ylen2).clone()
    finally:
        a.close()
    b = TrainEngine(_flags(0.3), vocab_size=40, device="cuda", compute_dtype="fp32", state_dict=sd)
    try:
        keep = wave.clone()
        steps = [b.evaluate_step(*batch) for batch in batches]
        loss, rate, pred, true = b.evaluate(batches)
        assert torch.equal(wave, keep)
        assert b.model.training and b.step_count == 0 and b._pref is None
        assert not b.flat.grad.any()
        assert loss == float(np.mean([s[0] for s in steps])) and rate == float(np.mean([s[1] for s in steps]))
        assert len(pred) == len(true) == 6
        assert all(np.array_equal(p, q) for p, q in zip(pred, steps[0][2] + steps[1][2]))
        refs = [ys[i, :int(ylen[i])].cpu().numpy() for i in range(4)] + [ys2[i, :int(ylen2[i])].cpu().numpy() for i in range(2)]
        assert all(np.array_equal(t, r) for t, r in zip(true, refs))
        tot = ER.totals([ER.counts_fast(p, t) for p, t in zip(pred, true)], [len(t) for t in true])
        assert all(getattr(b.last_eval, k) == v for k, v in tot.items())
        assert b.last_eval.rate == tot["errors"] / 26 and tot["ref_len"] == 21 + 5
        # the two figures: batch rates of 21 and 5 reference tokens weigh alike in the mean
        r1 = sum(ER.counts_fast(p, t)[0] for p, t in zip(pred[:4], true[:4])) / 21
        r2 = sum(ER.counts_fast(p, t)[0] for p, t in zip(pred[4:], true[4:])) / 5
        assert rate == float(np.mean([r1, r2]))
        assert len(b.evaluate(batches, sample_size=5)[2]) == 5
        assert np.isnan(b.evaluate([])[0]) and b.last_eval.sequences == 0
        got = b.train_step(wave, None, ys, ylen)
        grads, params, moments = b.flat.grad.clone(), b.flat.data.clone(), b.optim.m.clone()
        b.evaluate_step(*batches[1], search="ctc_greedy")
        assert torch.equal(b.flat.grad, grads) and torch.equal(b.flat.data, params) and torch.equal(b.optim.m, moments)
        got2 = b.train_step(wave2, None, ys2, ylen2)
        assert torch.equal(got, want) and torch.equal(got2, want2) and b.step_count == 2
    finally:
        b.close()
