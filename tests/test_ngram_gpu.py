"""GPU: the n-gram kernels of csrc/ngram.hip against the host restatement ``NGramLM.step`` / ``NGramLM.score``.  Every
score is a chain of float64 additions made in the same order on both sides, so everything is compared by EQUALITY:
the dense rows with ``np.float32(step)``, the sentence scores bit for bit."""
import numpy as np
import pytest
import torch

import ngram_ref as NR

pytestmark = pytest.mark.gpu


def _rows_on_host(lm):
    lp = np.zeros((lm.n_states, lm.V), dtype=np.float32)
    nxt = np.zeros((lm.n_states, lm.V), dtype=np.int32)
    for s in range(lm.n_states):
        for k in range(lm.V):
            if k == lm.blank:
                nxt[s, k] = s
                continue
            l, n = lm.step(s, k)
            lp[s, k] = np.float32(l)
            nxt[s, k] = n
    return lp, nxt


def _check_rows(lm, what):
    states = torch.arange(lm.n_states, dtype=torch.int32, device="cuda")
    lp, nxt = lm.logprobs(states, return_next=True)
    want_lp, want_next = _rows_on_host(lm)
    assert lp.dtype == torch.float32 and tuple(lp.shape) == (lm.n_states, lm.V)
    assert (lp.cpu().numpy() == want_lp).all(), what
    assert (nxt.cpu().numpy() == want_next).all(), what
    assert (lp[:, lm.blank] == 0).all()
    # rows in any order, repeated and out-of-range states (clamped); without the next states; run to run
    pick = torch.tensor([lm.n_states - 1, 0, lm.n_states - 1, lm.n_states + 5, -3], dtype=torch.int32, device="cuda")
    some = lm.logprobs(pick)
    assert (some.cpu().numpy() == want_lp[[lm.n_states - 1, 0, lm.n_states - 1, lm.n_states - 1, 0]]).all(), what
    assert torch.equal(lm.logprobs(states), lp)
    print("ngram rows", what, "%d states, %d arcs" % (lm.n_states, lm.n_arcs))


@pytest.mark.parametrize("V,order", [(8, 1), (29, 2), (40, 3), (80, 5)], ids=["V8-o1", "V29-o2", "V40-o3", "V80-o5"])
def test_dense_rows_of_all_states_equal_the_host_step(hip_lib, V, order):
    _check_rows(NR.model(V, order), (V, order))


def test_dense_rows_of_a_three_round_row_and_of_arcless_states(hip_lib):
    """V = 520: the row of (3,) holds more than 128 arcs; the ARPA model: states the suffix closure added have none."""
    lm = NR.wide_model()
    s = lm._index[(3,)]
    assert lm.row_ptr[s + 1] - lm.row_ptr[s] > 128
    _check_rows(lm, "wide")
    _check_rows(NR.closure_model(), "closure")
    assert lm.logprobs(torch.zeros(0, dtype=torch.int32, device="cuda")).shape == (0, 520)


def _depth(lm, s, k):
    """How many times step(s, k) backs off."""
    d = 0
    while s != 0:
        lo, hi = int(lm.row_ptr[s]), int(lm.row_ptr[s + 1])
        if k in lm.arc_tok[lo:hi]:
            break
        s = int(lm.fail[s])
        d += 1
    return d


def _score_case():
    """Ragged [B = 3, N = 4, U = 17] lists on the order-5 model: corpus sentences (explicit arcs of every order), random
    tokens (back-off to the unigrams), an empty hypothesis, bad tokens, a slot behind n_hyp, an utterance with n_hyp 0."""
    V = 80
    lm = NR.model(V, 5)
    rng = np.random.default_rng(3)
    corpus = NR.corpus(V)
    long = [s for s in corpus if len(s) >= 8]
    # six tokens of a sentence (a four-token context), then id 1, which no context has: order - 1 back-offs
    mixed = long[0][:6] + [1] + [int(k) for k in rng.integers(3, V, 3)] + long[1][:7]
    # two tokens from <s> (a three-token context), then id 1: order - 2 back-offs; random ids behind it
    lists = [[corpus[0], [], mixed[:17], long[2][:2] + [1] + [int(k) for k in rng.integers(1, V, 14)]],
             [corpus[1] + corpus[2][:5], [5, 0, 6], [7, V, 8], [9, -1]],
             [corpus[3], corpus[4]]]
    n_hyp = [4, 4, 0]
    B, N, U = 3, 4, 17
    hyps = np.full((B, N, U), -7, dtype=np.int32)          # behind the lengths: never read
    lens = np.zeros((B, N), dtype=np.int32)
    for b, seqs in enumerate(lists):
        for n, t in enumerate(seqs):
            hyps[b, n, :len(t)] = t
            lens[b, n] = len(t)
    lens[2, 3] = 40                                        # a slot behind n_hyp with a wild length
    return lm, lists, hyps, lens, np.array(n_hyp, dtype=np.int32)


def test_sentence_scores_equal_the_host_score_bit_for_bit(hip_lib):
    lm, lists, hyps, lens, n_hyp = _score_case()
    B, N, U = hyps.shape
    # the case backs off through every level, 0 .. order - 1 times
    depths = set()
    for t in lists[0] + lists[1][:1]:
        s = lm.start
        for k in t:
            depths.add(_depth(lm, s, k))
            s = lm.step(s, k)[1]
    assert depths == set(range(lm.order)), depths
    dh, dl, dn = (torch.tensor(a, device="cuda") for a in (hyps, lens, n_hyp))
    for bos in (True, False):
        for eos in (True, False):
            total, tlp = lm.score_nbest(dh, dl, dn, bos=bos, eos=eos, return_token_lp=True)
            total, tlp = total.cpu().numpy(), tlp.cpu().numpy()
            assert total.dtype == np.float64 and tlp.dtype == np.float32
            for b in range(B):
                for n in range(N):
                    t = hyps[b, n, :min(lens[b, n], U)].tolist()
                    if n >= n_hyp[b]:
                        assert total[b, n] == -np.inf and (tlp[b, n] == 0).all()
                        continue
                    want = lm.score(t, bos=bos, eos=eos)
                    assert total[b, n] == want, (b, n, bos, eos, total[b, n], want)
                    if np.isfinite(want):
                        s = lm.start if bos else 0
                        for u, k in enumerate(t):
                            l, s = lm.step(s, k)
                            assert tlp[b, n, u] == np.float32(l), (b, n, u)
                    assert (tlp[b, n, len(t):] == 0).all()
            assert np.isfinite(total[0]).all() and total[0, 1] == (lm.step(lm.start if bos else 0, lm.eos)[0] if eos else 0.0)
            assert (total[1, 1:] == -np.inf).all() and (total[2] == -np.inf).all()
            again = lm.score_nbest(dh, dl, dn, bos=bos, eos=eos)
            assert (again.cpu().numpy() == total).all()
    # n_hyp = None: every slot is live
    full = lm.score_nbest(dh[:2], dl[:2]).cpu().numpy()
    assert (full == lm.score_nbest(dh, dl, dn).cpu().numpy()[:2]).all()
    # U = 0: every hypothesis is empty
    none = lm.score_nbest(torch.zeros(2, 3, 0, dtype=torch.int32, device="cuda"),
                          torch.zeros(2, 3, dtype=torch.int32, device="cuda"), eos=True).cpu().numpy()
    assert (none == lm.step(lm.start, lm.eos)[0]).all()


def test_score_lists_and_a_row_of_three_rounds(hip_lib):
    """``score_lists`` (one upload, one call, one read) on the V = 520 model: tokens at the start, the middle and the
    end of the 141-arc row of (3,), a token the row lacks, and a token beyond its last arc."""
    lm = NR.wide_model()
    lists = [[[3, 10], [3, 75], [3, 149], [3, 519], [3, 200], [3, 9], [3, 150]], [], [[5, 6, 7], [200, 3, 519, 3, 80]]]
    for eos in (False, True):
        got = lm.score_lists(lists, eos=eos)
        assert [len(g) for g in got] == [7, 0, 2]
        for seqs, g in zip(lists, got):
            assert g.dtype == np.float64
            for t, x in zip(seqs, g):
                assert x == lm.score(t, eos=eos), t
