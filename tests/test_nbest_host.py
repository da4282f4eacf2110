"""CPU: the detail-carrying restatement of the beam search (tests/nbest_ref.py) earns its keep against
oracle/beam_ref.beam_search_one - entry 0 (tokens, the score as a Python float) and the pop count are equal exactly on
the tiny golden model (W = 1, 2, 4, 10) and on the random ragged batch of
test_beam_random_model_ragged_batch_matches_oracle - its frames and increments re-score to its own log p through the
dense lattice, and ``NBestResult.ranked`` orders and merges a hand-made list as documented."""
import os

import numpy as np
import pytest
import torch

import nbest_ref as N
from oracle import beam_ref, models_ref as M

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "beam_tiny.npz"))
CFG = dict(vocab_embed_size=16, vocab_size=40, input_size=24, enc_hidden_size=32, enc_layers=2,
           enc_proj_size=24, dec_hidden_size=32, dec_layers=2, dec_proj_size=24, joint_size=32)


def _golden():
    sd = {k[3:]: torch.from_numpy(G[k]) for k in G.files if k.startswith("sd/")}
    return sd, torch.from_numpy(G["xs"]), torch.from_numpy(G["xlen"])


def _check_against_beam_ref(sd, xs, xlen, W):
    h_enc, lens = N.encode(sd, xs, xlen)
    for b in range(h_enc.shape[0]):
        res, nexp, gap = N.nbest_one(sd, h_enc[b, :lens[b]], W)
        k, score, rexp = beam_ref.beam_search_one(sd, h_enc[b, :lens[b]], W)
        assert res[0]["tokens"] == k
        assert isinstance(score, float) and -res[0]["logp"] == score          # the same Python float
        assert nexp == rexp
        assert 1 <= len(res) <= W and gap > 0
        lp_cache = {}
        for h in res:
            assert len(h["frames"]) == len(h["tokens"]) == len(h["token_logp"])
            assert all(0 <= f < lens[b] for f in h["frames"]) and h["frames"] == sorted(h["frames"])
            # the detail describes a path of the lattice whose log p is the hypothesis' (fp64 sums of the same fp32 terms)
            key = tuple(h["tokens"])
            if key not in lp_cache:
                lp_cache[key] = N.lattice_logp(sd, h_enc[b, :lens[b]], h["tokens"])
            total, terms = N.path_logp(lp_cache[key], h["tokens"], h["frames"])
            np.testing.assert_allclose(total, h["logp"], rtol=0, atol=1e-5)
            np.testing.assert_allclose(terms, h["token_logp"], rtol=0, atol=1e-5)


@pytest.mark.parametrize("W", [1, 2, 4, 10])
def test_helper_entry_zero_and_pops_equal_beam_ref_on_the_golden_model(W):
    sd, xs, xlen = _golden()
    _check_against_beam_ref(sd, xs, xlen, W)


def test_helper_entry_zero_and_pops_equal_beam_ref_on_the_random_ragged_batch():
    sd = M.make_state_dict(CFG, 3)
    xs, ys, xlen, ylen = M.make_batch(CFG, 4, 5, 17, 4)
    xlen = torch.tensor([17, 9, 17, 3, 12], dtype=torch.int32)
    _check_against_beam_ref(sd, xs, xlen, 3)


def test_helper_zero_frames_is_one_empty_hypothesis():
    sd, xs, _ = _golden()
    res, nexp, gap = N.nbest_one(sd, N.encode(sd, xs)[0][0, :0], 4)
    assert res == [dict(tokens=[], frames=[], token_logp=[], logp=0.0)] and nexp == 0


def _result(entries):
    from edgedict_amd.decode import NBestResult
    return NBestResult([np.array(t, dtype=np.int64) for t, _, _ in entries],
                       [np.arange(len(t), dtype=np.int32) + off for t, off, _ in entries],
                       [np.full(len(t), -0.5 - off) for t, off, _ in entries], [lp for _, _, lp in entries])


def test_ranked_orders_stably_and_merges_duplicates_with_log_add():
    la = lambda *v: float(np.log(np.sum(np.exp(np.array(v)))))
    # (tokens, frame offset - which marks the member -, logp) in "insertion order"
    r = _result([([5, 6], 0, -3.0), ([5], 1, -2.0), ([5, 6], 2, -2.5), ([7], 3, -2.0), ([], 4, -4.0), ([5, 6], 5, -2.5),
                 ([9], 6, -1.0)])
    assert len(r) == 7
    plain = r.ranked(merge=False)
    # descending, ties in B's order: -1.0 | -2.0 (entry 1 before entry 3) | -2.5 (entry 2 before entry 5) | -3.0 | -4.0
    assert [int(f[0]) if len(f) else 4 for f in plain.frames] == [6, 1, 3, 2, 5, 0, 4]
    assert np.array_equal(plain.logp, [-1.0, -2.0, -2.0, -2.5, -2.5, -3.0, -4.0])
    assert len(r) == 7 and r.logp[0] == -3.0                    # ranked() leaves the result itself alone
    merged = r.ranked()                                          # merge=True is the default
    # [5, 6] folds three members: log-add, detail of its most probable member (entry 2: the first of the -2.5 tie)
    want56 = la(-3.0, -2.5, -2.5)
    assert [t.tolist() for t in merged.tokens] == [[9], [5, 6], [5], [7], []]
    np.testing.assert_allclose(merged.logp, [-1.0, want56, -2.0, -2.0, -4.0], rtol=1e-12)
    assert want56 > -2.0                                          # the merged entry overtakes the two single -2.0 ones
    assert merged.frames[1].tolist() == [2, 3] and np.array_equal(merged.token_logp[1], [-2.5, -2.5])
    assert merged.frames[2].tolist() == [1] and merged.frames[3].tolist() == [3]      # the -2.0 tie keeps B's order
    for t, f, l in zip(merged.tokens, merged.frames, merged.token_logp):
        assert t.dtype == np.int64 and len(t) == len(f) == len(l)
    assert merged.logp.dtype == np.float64


def test_ranked_of_an_empty_and_of_a_single_result():
    from edgedict_amd.decode import NBestResult
    e = NBestResult([], [], [], []).ranked()
    assert len(e) == 0 and e.logp.shape == (0,)
    one = _result([([], 0, 0.0)]).ranked()
    assert len(one) == 1 and one.logp[0] == 0.0 and len(one.tokens[0]) == 0
