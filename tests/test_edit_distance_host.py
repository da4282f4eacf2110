"""CPU: the host side of the error-rate metrics.  The integer oracle tests/edit_distance_ref.py that the GPU tests
compare against is pinned here on the enumeration of every alignment; the word splitting, the accumulator's arithmetic,
the list packer and every argument error (raised before anything is launched) are checked without a device."""
import ctypes
import itertools
import math

import numpy as np
import pytest
import torch

import edit_distance_ref as ER

_KW = dict(vocab_embed_size=8, vocab_size=12, input_size=16, enc_hidden_size=16, enc_layers=2, enc_dropout=0.0,
           enc_proj_size=12, dec_hidden_size=8, dec_layers=1, dec_dropout=0.0, dec_proj_size=8, joint_size=16)


def _identities(got, h, r):
    dist, sub, dele, ins = got
    H, R = len(h), len(r)
    hits = R - sub - dele
    assert dist == sub + dele + ins
    assert ins - dele == H - R
    assert sub + dele + hits == R and hits >= 0
    assert min(sub, dele, ins) >= 0
    assert max(H, R) >= dist >= abs(H - R)


def test_dp_equals_the_enumeration_of_every_alignment_two_symbols():
    n = 0
    for H in range(5):
        for R in range(5):
            for h in itertools.product((0, 1), repeat=H):
                for r in itertools.product((0, 1), repeat=R):
                    got = ER.counts(h, r)
                    assert got == ER.enumerate_all(h, r), (h, r)
                    assert got == ER.counts_fast(h, r), (h, r)
                    _identities(got, h, r)
                    n += 1
    assert n == 31 * 31


def test_dp_equals_the_enumeration_on_random_pairs():
    rng = np.random.default_rng(1)
    mixed = 0
    for _ in range(2000):
        h = rng.integers(0, 3, size=rng.integers(0, 8)).tolist()
        r = rng.integers(0, 3, size=rng.integers(0, 8)).tolist()
        got = ER.counts(h, r)
        assert got == ER.enumerate_all(h, r), (h, r)
        _identities(got, h, r)
        mixed += got[2] > 0 and got[3] > 0           # the optimum itself needs an insertion and a deletion
    assert mixed > 20


def test_row_form_equals_the_dp():
    rng = np.random.default_rng(2)
    for k in range(60):
        A = 2 + k % 3
        h = rng.integers(0, A, size=rng.integers(0, 131)).tolist()
        r = rng.integers(0, A, size=rng.integers(0, 131)).tolist()
        got = ER.counts_fast(h, r)
        assert got == ER.counts(h, r), (h, r)
        _identities(got, h, r)
    # the extremes the packing has to hold: all substitutions, all insertions, all deletions at length 1023
    assert ER.counts_fast(np.zeros(1023), np.ones(1023)) == (1023, 1023, 0, 0)
    assert ER.counts_fast(np.zeros(1023), []) == (1023, 0, 0, 1023)
    assert ER.counts_fast([], np.zeros(1023)) == (1023, 0, 1023, 0)


def test_known_answers():
    k, s = [ord(c) for c in "kitten"], [ord(c) for c in "sitting"]
    for f in (ER.counts, ER.counts_fast, ER.enumerate_all):
        assert f(s, k) == (3, 2, 0, 1)               # hypothesis "sitting", reference "kitten"
        assert f(k, s) == (3, 2, 1, 0)
        assert f(k, k) == (0, 0, 0, 0)
        assert f([], []) == (0, 0, 0, 0)
        assert f([], [1, 2, 3, 4, 5]) == (5, 0, 5, 0)
        assert f([1, 2, 3, 4, 5], []) == (5, 0, 0, 5)
        # a genuine tie: turning r = [1, 2] into h = [2, 3] costs 2 either as two substitutions or as one deletion
        # (the 1) plus one insertion (the 3) around the hit on 2 - the rule picks the substitutions
        assert f([2, 3], [1, 2]) == (2, 2, 0, 0)
        # symbols are only compared: the int32 extremes are ordinary symbols
        lo, hi = -2 ** 31, 2 ** 31 - 1
        assert f([lo, -1, 0, hi], [lo, 0, hi]) == (1, 0, 0, 1)


def test_tie_really_exists():
    """Both alignments of the tie case cost 2: the one with ins + del is an alignment, and it is not the one picked."""
    h, r = [2, 3], [1, 2]
    # delete r[0], hit 2 == 2, insert h[1]: distance 2 with one insertion
    alt = (2, 1)
    best = ER.enumerate_all(h, r)
    assert (best[0], best[3]) < alt and best[0] == alt[0]


def test_word_splitting_and_the_corpus_level_sum(monkeypatch):
    from edgedict_amd import metrics
    hyps, refs = metrics.words_to_ids(["  the  cat sat ", "", "a b"], ["the cat  sat down", "x", ""])
    assert [h.tolist() for h in hyps] == [[0, 1, 2], [], [3, 4]]
    assert [r.tolist() for r in refs] == [[0, 1, 2, 5], [6], []]
    with pytest.raises(TypeError, match="str"):
        metrics.words_to_ids([["a"]], ["a"])

    seen = []

    def fake_lists(hyp_lists, refs, device=None):
        seen.append((hyp_lists, refs))
        return [np.array([ER.counts(h, r) for h in seqs], dtype=np.int32).reshape(-1, 4)
                for seqs, r in zip(hyp_lists, refs)]

    monkeypatch.setattr(metrics, "edit_distance_lists", fake_lists)
    rec = metrics.word_error_rate(["  the  cat sat ", "", "a b"], ["the cat  sat down", "x", ""])
    # one deletion, one deletion, two insertions over 4 + 1 + 0 reference words
    assert (rec.errors, rec.substitutions, rec.deletions, rec.insertions) == (4, 0, 2, 2)
    assert rec.ref_len == 5 and rec.sequences == 3 and rec.wrong_sequences == 3
    assert rec.rate == 4 / 5 and rec.del_rate == 2 / 5 and rec.ins_rate == 2 / 5 and rec.sub_rate == 0.0
    assert rec.sentence_rate == 1.0
    assert len(seen) == 1                            # one packer call for the whole corpus
    # the corpus-level figure is not the mean of the sentence rates
    rec = metrics.word_error_rate(["a", "a b c d"], ["b", "a b c d"])
    assert rec.rate == 1 / 5 and rec.sentence_rate == 0.5
    rec = metrics.token_error_rate([[1, 2, 3]], [[1, 3]])
    assert (rec.errors, rec.insertions, rec.ref_len) == (1, 1, 2)
    rec = metrics.token_error_rate([[]], [[]])
    assert math.isnan(rec.rate) and rec.sentence_rate == 0.0 and rec.sequences == 1
    with pytest.raises(ValueError, match="2 hypotheses for 1 references"):
        metrics.word_error_rate(["a", "b"], ["a"])


def test_packer_layout_and_split_of_long_lists():
    from edgedict_amd import metrics
    conv = lambda lists: [[np.asarray(t, dtype=np.int64) for t in seqs] for seqs in lists]
    lists = conv([[[1, 2, 3], [4]], [], [[7]] * 40])
    refs = [np.array([1, 2]), np.array([9, 9, 9, 9, 9]), np.array([7, 8, 9, 10])]
    host, (B, N, Uh, Ur), pieces = metrics._pack(lists, refs)
    assert (B, N, Uh, Ur) == (3, 32, 3, 4)           # the empty list takes no row, its reference is not uploaded
    assert pieces == [[(0, 2)], [], [(1, 32), (2, 8)]]
    nh, nr, nl = B * N * Uh, B * Ur, B * N
    assert host.dtype == np.int32 and host.size == nh + nr + nl + 2 * B
    hyps = host[:nh].reshape(B, N, Uh)
    assert hyps[0, 0].tolist() == [1, 2, 3] and hyps[0, 1].tolist() == [4, 0, 0] and hyps[2, 7, 0] == 7
    assert host[nh:nh + nr].reshape(B, Ur).tolist() == [[1, 2, 0, 0], [7, 8, 9, 10], [7, 8, 9, 10]]
    assert host[nh + nr:nh + nr + nl].reshape(B, N)[0, :3].tolist() == [3, 1, 0]
    assert host[nh + nr + nl:nh + nr + nl + B].tolist() == [2, 4, 4]
    assert host[nh + nr + nl + B:].tolist() == [2, 32, 8]
    # nothing to score: no launch, no device needed
    assert metrics._pack(conv([[], []]), refs[:2]) is None
    got = metrics.edit_distance_lists([[], []], [[1], [2]])
    assert [g.shape for g in got] == [(0, 4), (0, 4)] and got[0].dtype == np.int32
    with pytest.raises(ValueError, match="1 lists for 2 references"):
        metrics.edit_distance_lists([[]], [[1], [2]])
    with pytest.raises(ValueError, match="1023"):
        metrics.edit_distance_lists([[np.zeros(1024, dtype=np.int64)]], [[1]])
    with pytest.raises(ValueError, match="outside int32"):
        metrics.edit_distance_lists([[[2 ** 31]]], [[1]])
    with pytest.raises(TypeError, match="integers"):
        metrics.edit_distance_lists([[[0.5]]], [[1]])


def test_error_rate_accumulator_on_cpu_tensors():
    from edgedict_amd.metrics import ErrorRate
    acc = ErrorRate()
    empty = acc.compute()
    assert math.isnan(empty.rate) and math.isnan(empty.sentence_rate) and empty.sequences == 0
    pairs = torch.tensor([[3, 2, 0, 1], [0, 0, 0, 0]], dtype=torch.int32)
    acc.update(pairs, torch.tensor([6, 4], dtype=torch.int32))
    lists = torch.tensor([[[2, 1, 1, 0], [-1, -1, -1, -1]], [[5, 0, 5, 0], [1, 0, 0, 1]]], dtype=torch.int32)
    acc.update(lists, torch.tensor([7, 5], dtype=torch.int32))
    assert acc.totals.dtype == torch.int64
    rec = acc.compute()
    want = ER.totals([[3, 2, 0, 1], [0, 0, 0, 0], [2, 1, 1, 0], [5, 0, 5, 0], [1, 0, 0, 1]], [6, 4, 7, 5, 5])
    for k, v in want.items():
        assert getattr(rec, k) == v, k
    assert rec.rate == 11 / 27 and rec.sub_rate == 3 / 27 and rec.del_rate == 6 / 27 and rec.ins_rate == 2 / 27
    assert rec.sentence_rate == 4 / 5
    acc.reset()
    assert acc.compute().sequences == 0 and math.isnan(acc.compute().rate)
    with pytest.raises(ValueError, match="\\[\\.\\.\\., 4\\]"):
        acc.update(torch.zeros(2, 3, dtype=torch.int32), torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="reference length per row"):
        acc.update(pairs, torch.zeros(3, dtype=torch.int32))


def test_nbest_helpers_through_the_oracle(monkeypatch):
    from edgedict_amd import metrics
    from edgedict_amd.decode import NBestResult

    def fake_lists(hyp_lists, refs, device=None):
        return [np.array([ER.counts(h, r) for h in seqs], dtype=np.int32).reshape(-1, 4)
                for seqs, r in zip(hyp_lists, refs)]

    monkeypatch.setattr(metrics, "edit_distance_lists", fake_lists)

    def nbest(seqs, logp):
        seqs = [np.asarray(s, dtype=np.int64) for s in seqs]
        return NBestResult(seqs, [np.zeros(s.size, np.int32) for s in seqs], [np.zeros(s.size) for s in seqs], logp)

    results = [nbest([[1, 2, 9], [1, 2, 3], [1, 2, 3, 4]], [-1.0, -2.0, -np.inf]),
               nbest([[5], [6]], [-3.0, -3.0]), nbest([], []), nbest([[7, 7]], [-np.inf])]
    refs = [[1, 2, 3], [4, 4], [1, 2], [7]]
    errs = metrics.nbest_errors(results, refs)
    assert errs[0][:, 0].tolist() == [1, 0, 1] and errs[1][:, 0].tolist() == [2, 2] and errs[2].shape == (0, 4)
    rec, idx = metrics.oracle_error_rate(results, refs)
    assert idx.tolist() == [1, 0, -1, 0]             # ties go to the lower index; -1: an empty list
    assert (rec.errors, rec.deletions, rec.ref_len, rec.sequences, rec.wrong_sequences) == (0 + 2 + 2 + 1, 3, 8, 4, 3)
    risk = metrics.expected_errors(results, refs)
    w = np.exp(np.array([-1.0, -2.0]))
    assert risk[0] == pytest.approx((w[0] * 1 + w[1] * 0) / w.sum(), rel=1e-15)
    assert risk[1] == 2.0 and math.isnan(risk[2]) and math.isnan(risk[3])


def test_edit_distance_refuses_cpu_tensors_and_bad_inputs():
    from edgedict_amd.metrics import edit_distance
    i32 = dict(dtype=torch.int32)
    hyps, hl = torch.ones(2, 3, 4, **i32), torch.full((2, 3), 2, **i32)
    refs, rl, nh = torch.ones(2, 5, **i32), torch.tensor([5, 4], **i32), torch.tensor([3, 1], **i32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        edit_distance(hyps, hl, refs, rl, nh)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        edit_distance(hyps, hl, refs, rl)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        edit_distance(hyps[:, 0].contiguous(), hl[:, 0].contiguous(), refs, rl)
    for name, args in (("hyps", (hyps.long(), hl, refs, rl, nh)), ("hyp_lens", (hyps, hl.long(), refs, rl, nh)),
                       ("refs", (hyps, hl, refs.float(), rl, nh)), ("ref_lens", (hyps, hl, refs, rl.long(), nh)),
                       ("n_hyp", (hyps, hl, refs, rl, nh.long()))):
        with pytest.raises(TypeError, match="%s must be int32" % name):
            edit_distance(*args)
    with pytest.raises(TypeError, match="must be a tensor"):
        edit_distance(hyps.numpy(), hl, refs, rl)
    with pytest.raises(ValueError, match="3 dimensions \\[B,N,Uh\\]"):
        edit_distance(hyps[0, 0].contiguous(), hl, refs, rl)
    with pytest.raises(ValueError, match="2 dimensions \\[B,N\\]"):
        edit_distance(hyps, hl[:, 0].contiguous(), refs, rl)
    with pytest.raises(ValueError, match="2 dimensions \\[B,Ur\\]"):
        edit_distance(hyps, hl, refs[0].contiguous(), rl)
    with pytest.raises(ValueError, match="1 dimension"):
        edit_distance(hyps, hl, refs, rl.unsqueeze(1))
    with pytest.raises(ValueError, match="contiguous"):
        edit_distance(hyps.transpose(1, 2), hl, refs, rl)
    with pytest.raises(ValueError, match="contiguous"):
        edit_distance(hyps, hl, refs.t(), rl)
    with pytest.raises(ValueError, match="hypothesis length per slot"):
        edit_distance(hyps, hl[:, :2].contiguous(), refs, rl)
    with pytest.raises(ValueError, match="reference and its length per example"):
        edit_distance(hyps, hl, refs[:1], rl)
    with pytest.raises(ValueError, match="reference and its length per example"):
        edit_distance(hyps, hl, refs, rl[:1])
    with pytest.raises(ValueError, match="hypothesis count per example"):
        edit_distance(hyps, hl, refs, rl, nh[:1])
    with pytest.raises(ValueError, match="at least one utterance"):
        edit_distance(torch.ones(0, 3, 4, **i32), torch.ones(0, 3, **i32), torch.ones(0, 5, **i32), torch.ones(0, **i32))
    with pytest.raises(ValueError, match="outside \\[1, 32\\]"):
        edit_distance(torch.ones(2, 33, 4, **i32), torch.ones(2, 33, **i32), refs, rl)
    with pytest.raises(ValueError, match="outside \\[1, 32\\]"):
        edit_distance(torch.ones(2, 0, 4, **i32), torch.ones(2, 0, **i32), refs, rl)
    with pytest.raises(ValueError, match="Uh = 1024"):
        edit_distance(torch.ones(2, 1, 1024, **i32), torch.ones(2, 1, **i32), refs, rl)
    with pytest.raises(ValueError, match="Ur = 1024"):
        edit_distance(hyps, hl, torch.ones(2, 1024, **i32), rl)
    with pytest.raises(ValueError, match="plain pairs"):
        edit_distance(hyps[:, 0].contiguous(), hl[:, 0].contiguous(), refs, rl, nh)


def test_new_symbol_is_declared_and_exported(hip_lib):
    from edgedict_amd import _lib
    assert "edgedict_edit_distance" in _lib.declared_symbols()
    assert hasattr(hip_lib, "edgedict_edit_distance")
    assert hip_lib.edgedict_abi_version() == 2


def test_native_argument_errors_are_raised_before_any_launch(hip_lib):
    """B = 0, N outside [1, 32], a U of 1024 or below 0, a null pointer that is needed: -1 with a message, no device
    needed.  (That U = 0 may leave the token pointer null and that n_hyp may always be null takes a launch to show:
    test_edit_distance_gpu.py.)"""
    buf = ctypes.create_string_buffer(128)
    fake = ctypes.c_void_p(ctypes.addressof(buf))

    def dist(hyps=fake, hl=fake, nh=fake, refs=fake, rl=fake, B=2, N=2, Uh=3, Ur=3, out=fake):
        return hip_lib.edgedict_edit_distance(hyps, hl, nh, refs, rl, B, N, Uh, Ur, out, None)

    for kw, word in ((dict(B=0), b"B must be positive"), (dict(B=-1), b"B must be positive"), (dict(N=0), b"N = 0"),
                     (dict(N=33), b"N = 33"), (dict(Uh=1024), b"Uh = 1024"), (dict(Ur=1024), b"Ur = 1024"),
                     (dict(Uh=-1), b"Uh = -1"), (dict(Ur=-1), b"Ur = -1"), (dict(B=1 << 30, N=32), b"exceeds the grid")):
        assert dist(**kw) == -1, kw
        assert word in hip_lib.edgedict_last_error(), kw
        assert b"edit_distance" in hip_lib.edgedict_last_error(), kw
    for name in ("hyps", "hl", "refs", "rl", "out"):
        assert dist(**{name: None}) == -1, name
        assert b"null pointer" in hip_lib.edgedict_last_error(), name


def test_evaluate_step_refuses_an_unknown_search():
    from edgedict_amd.models import Transducer
    m = Transducer(**_KW)
    xs, ys = torch.zeros(1, 4, 16), torch.ones(1, 2, dtype=torch.int32)
    xlen, ylen = torch.tensor([4], dtype=torch.int32), torch.tensor([2], dtype=torch.int32)
    with pytest.raises(ValueError, match="search must be one of"):
        m.evaluate_step(xs, ys, xlen, ylen, search="nonsense")
    with pytest.raises(ValueError, match="takes no search arguments"):
        m.evaluate_step(xs, ys, xlen, ylen, search="greedy", W=4)
