"""CPU: the streaming CTC prefix beam search's host side (include/edgedict_hip.h ``edgedict_ctc_stream_*``,
decode.StreamingCTCBeamSearch, stream.BatchedStreamCTCBeamDecoder): the symbols and size queries, every argument
refusal (before the device is touched: the pointers here are host memory), the Python argument errors, and - with the
float64 oracle of tests/ctc_beam_ref.py - that the compaction cases of tests/test_ctc_stream_gpu.py fit the capacities
chosen for them and would not fit without compaction."""
import ctypes

import pytest

import ctc_beam_ref as BR
import ctc_stream_ref as SR
from search_abi import fake_pointer

NAMES = {"edgedict_ctc_stream_state_bytes", "edgedict_ctc_stream_workspace_bytes", "edgedict_ctc_stream_reset",
         "edgedict_ctc_stream_advance", "edgedict_ctc_stream_nbest"}


def test_symbols_are_declared_and_the_size_queries_grow(hip_lib):
    from edgedict_amd import _lib
    assert NAMES <= set(_lib.declared_symbols())
    for name in NAMES:
        assert hasattr(hip_lib, name), name
    st, ws = hip_lib.edgedict_ctc_stream_state_bytes, hip_lib.edgedict_ctc_stream_workspace_bytes
    assert st.restype is ctypes.c_size_t and ws.restype is ctypes.c_size_t
    # (S, W, NC)
    for bad in ((0, 4, 64), (-1, 4, 64), (2, 0, 64), (2, 33, 64), (2, 4, 3), (2, 4, 0), (1 << 30, 32, 64)):
        assert st(*bad) == 0, bad
    # (S, Tc, W, cand, NC)
    for bad in ((0, 5, 4, 8, 64), (2, 0, 4, 8, 64), (2, 5, 0, 8, 64), (2, 5, 33, 8, 64), (2, 5, 4, 0, 64),
                (2, 5, 4, 65, 64), (2, 5, 4, 8, 3), (1 << 20, 1 << 10, 4, 64, 64)):
        assert ws(*bad) == 0, bad
    n = st(2, 4, 64)
    # four fp64 and six int32 fields per entry, the tree's 16-byte nodes
    assert n >= 2 * 4 * (4 * 8 + 6 * 4) + 2 * 64 * 16 and n % 256 == 0
    assert st(3, 4, 64) > n and st(2, 4, 65 + 16) > n and st(64, 32, 64) > st(64, 10, 64)
    m = ws(2, 5, 4, 8, 64)
    assert m >= 2 * 5 * 8 * 8 + 2 * 65 * 16 and m % 256 == 0
    sizes = [ws(S, 5, 4, 8, 64) for S in (1, 2, 7, 64, 256)]
    assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    sizes = [ws(8, Tc, 4, 8, 64) for Tc in (1, 2, 16, 17, 128)]
    assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    sizes = [ws(8, 5, 4, 8, NC) for NC in (4, 64, 65, 1344, 100000)]
    assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    sizes = [st(8, 4, NC) for NC in (4, 64, 1344, 100000)]
    assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)


def _bad_bias(V):
    from edgedict_amd.bias import BeamBias
    b = BeamBias()
    b.S, b.V, b.n_exc = 1, V, 0
    return b


def _ngram(fake, V=16, blank=0, weight=0.5, order=3, **kw):
    from edgedict_amd.ngram import NGramStruct
    s = NGramStruct()
    s.V, s.order, s.S, s.n_arcs, s.start, s.blank = V, order, 4, 0, 1, blank
    for name in ("uni_lp", "uni_next", "row_ptr", "fail", "backoff", "arc_tok", "arc_lp", "arc_next"):
        setattr(s, name, fake.value)
    s.weight, s.length_bonus = weight, 0.0
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _opts(bias=None, ngram=None):
    from edgedict_amd.ngram import CtcBeamOpts
    o = CtcBeamOpts()
    o.bias = None if bias is None else ctypes.addressof(bias)
    o.ngram = None if ngram is None else ctypes.addressof(ngram)
    return o


def test_every_refusal_names_the_call_and_comes_before_any_launch(hip_lib):
    """W, cand, dtype, blank, V, node_capacity < W, null and non-pointer arguments, the bias list's and the n-gram's
    vocabulary, blank and tables, the capacity rule: -1 with a message naming ctc_stream_*; no device needed."""
    buf, fake = fake_pointer(512)
    fake = ctypes.c_void_p((fake.value + 15) & ~15)          # the calls want 16-byte aligned state and workspace
    S, W, NC = 2, 4, 64
    nf = (ctypes.c_int32 * S)(3, 5)
    live = (ctypes.c_int32 * S)(1, 1)
    commit = ctypes.create_string_buffer(S * (NC + 1) * 16)
    err = hip_lib.edgedict_last_error
    small = ctypes.c_void_p(8)

    def advance(logits=fake, dtype=0, nf=nf, S=S, Tc=5, V=16, blank=0, W=W, cand=8, NC=NC, opts=None, live=live,
                commit=commit, max_commit=NC, state=fake, ws=fake):
        return hip_lib.edgedict_ctc_stream_advance(logits, dtype, nf, S, Tc, V, blank, W, cand, NC, opts, live, commit,
                                                   max_commit, state, ws, None)

    def refused(rc, word, what):
        assert rc == -1, what
        msg = err()
        assert b"ctc_stream_" in msg and word in msg, (what, msg)

    for name in ("logits", "nf", "live", "commit", "state", "ws"):
        refused(advance(**{name: None}), b"null pointer", name)
    for name in ("logits", "state", "ws"):
        refused(advance(**{name: small}), b"not a pointer", name)
    refused(advance(opts=small), b"opts is not a pointer", "opts")
    for kw, word in ((dict(W=0), b"W = 0"), (dict(W=33, NC=64), b"W = 33"), (dict(cand=0), b"cand = 0"),
                     (dict(cand=65), b"cand = 65"), (dict(V=1), b"V = 1"), (dict(blank=16), b"blank"),
                     (dict(blank=-1), b"blank"), (dict(dtype=7), b"dtype"), (dict(NC=3), b"node_capacity = 3"),
                     (dict(S=0), b"S = 0"), (dict(Tc=0), b"Tc = 0"), (dict(max_commit=-1), b"max_commit"),
                     (dict(ws=ctypes.c_void_p(fake.value + 4)), b"aligned"),
                     (dict(state=ctypes.c_void_p(fake.value + 8)), b"aligned")):
        refused(advance(**kw), word, kw)
    # the options
    bad = _bad_bias(12)
    refused(advance(opts=ctypes.byref(_opts(bias=bad))), b"vocabulary", "bias V")
    bad = _bad_bias(16)
    refused(advance(opts=ctypes.byref(_opts(bias=bad))), b"null bias table", "bias tables")
    o = _opts(bias=bad)
    o.bias = 8
    refused(advance(opts=ctypes.byref(o)), b"not a pointer", "bias pointer")
    for kw, word in ((dict(V=12), b"vocabulary"), (dict(blank=3), b"blank"), (dict(weight=-1.0), b"weight"),
                     (dict(weight=float("nan")), b"weight"), (dict(order=9), b"order"), (dict(uni_lp=None), b"null n-gram"),
                     (dict(start=7), b"start")):
        ng = _ngram(fake, **kw)
        refused(advance(opts=ctypes.byref(_opts(ngram=ng))), word, kw)
    # the frames and the capacity rule
    refused(advance(nf=(ctypes.c_int32 * S)(3, 6)), b"n_frames[1] = 6", "n_frames")
    refused(advance(nf=(ctypes.c_int32 * S)(-1, 0)), b"n_frames[0] = -1", "n_frames")
    refused(advance(live=(ctypes.c_int32 * S)(1, 0)), b"live[1] = 0", "live")
    refused(advance(live=(ctypes.c_int32 * S)(1, 45)), b"node_capacity is 64", "capacity")        # 45 + 5 x 4 = 65
    refused(advance(max_commit=3), b"max_commit = 3", "max_commit")
    assert list(live) == [1, 1]

    def reset(S=S, W=W, NC=NC, opts=None, mask=None, state=fake):
        return hip_lib.edgedict_ctc_stream_reset(S, W, NC, opts, mask, state, None)

    ng0, bias0 = _ngram(fake, order=0), _bad_bias(16)
    o_ng, o_bias = _opts(ngram=ng0), _opts(bias=bias0)
    for kw, word in ((dict(W=0), b"W = 0"), (dict(W=33), b"W = 33"), (dict(NC=3), b"node_capacity = 3"),
                     (dict(S=0), b"S = 0"), (dict(state=None), b"null pointer"), (dict(opts=small), b"not a pointer"),
                     (dict(mask=small), b"mask is not a pointer"), (dict(opts=ctypes.byref(o_ng)), b"order"),
                     (dict(opts=ctypes.byref(o_bias)), b"null bias table")):
        rc = reset(**kw)
        refused(rc, word, kw)
        assert b"ctc_stream_reset" in err()

    def nbest(S=S, W=W, NC=NC, state=fake, MT=8, tokens=fake, frames=fake, tlp=fake, ntok=fake, nhyp=fake, logp=fake):
        return hip_lib.edgedict_ctc_stream_nbest(S, W, NC, state, MT, tokens, frames, tlp, ntok, nhyp, logp, None)

    for name in ("state", "tokens", "frames", "tlp", "ntok", "nhyp", "logp"):
        refused(nbest(**{name: None}), b"null pointer", name)
    for kw, word in ((dict(W=0), b"W = 0"), (dict(W=33), b"W = 33"), (dict(NC=3), b"node_capacity = 3"),
                     (dict(S=0), b"S = 0"), (dict(MT=0), b"max_tokens = 0")):
        refused(nbest(**kw), word, kw)
        assert b"ctc_stream_nbest" in err()
    del buf


def test_python_argument_errors_need_no_device():
    from edgedict_amd.bias import ContextGraph
    from edgedict_amd.decode import StreamingCTCBeamSearch
    from edgedict_amd.lm import LMModel
    from edgedict_amd.ngram import NGramLM
    for kw, word in ((dict(W=0), "W = 0"), (dict(W=33), "W = 33"), (dict(cand=0), "cand = 0"), (dict(cand=65), "cand = 65"),
                     (dict(blank=8), "blank"), (dict(blank=-1), "blank"), (dict(node_capacity=3), "node_capacity = 3")):
        with pytest.raises(ValueError, match=word):
            StreamingCTCBeamSearch(2, 8, **dict(dict(W=4), **kw))
    with pytest.raises(ValueError, match="n_streams"):
        StreamingCTCBeamSearch(0, 8)
    with pytest.raises(ValueError, match="V = 1"):
        StreamingCTCBeamSearch(2, 1)
    with pytest.raises(ValueError, match="ContextGraph"):
        StreamingCTCBeamSearch(2, 8, bias=[[1, 2]])
    with pytest.raises(ValueError, match="vocabulary"):
        StreamingCTCBeamSearch(2, 8, bias=ContextGraph([[1, 2]], 1.0, 9, blank=0, bos=-1))
    with pytest.raises(TypeError, match="NGramLM"):
        StreamingCTCBeamSearch(2, 8, lm=LMModel(8, 4, 4, 1), lm_weight=0.5)
    lm = NGramLM.train([[3, 4, 5], [4, 5, 6]], 2, 8)
    with pytest.raises(ValueError, match="lm_weight is required"):
        StreamingCTCBeamSearch(2, 8, lm=lm)
    with pytest.raises(ValueError, match="lm_weight without lm"):
        StreamingCTCBeamSearch(2, 8, lm_weight=0.5)
    with pytest.raises(ValueError, match="lm_weight must be"):
        StreamingCTCBeamSearch(2, 8, lm=lm, lm_weight=-1.0)
    with pytest.raises(ValueError, match="vocabulary"):
        StreamingCTCBeamSearch(2, 9, lm=lm, lm_weight=0.5)


def test_decoder_on_a_model_without_a_head_raises_what_ctc_beam_search_raises():
    from edgedict_amd.flags import make_flags
    from edgedict_amd.models import Transducer
    from edgedict_amd.stream import BatchedStreamCTCBeamDecoder
    kw = dict(vocab_embed_size=8, vocab_size=12, input_size=16, enc_hidden_size=16, enc_layers=2, enc_dropout=0.0,
              enc_proj_size=12, dec_hidden_size=8, dec_layers=1, dec_dropout=0.0, dec_proj_size=8, joint_size=16)
    with pytest.raises(RuntimeError, match="no CTC head: construct it with"):
        BatchedStreamCTCBeamDecoder(Transducer(**kw), make_flags("E6D2"), 2)


def test_chunkings_and_the_tree_a_compaction_leaves():
    for T in (1, 5, 8, 33, 47, 65):
        for kind in SR.CHUNKINGS:
            c = SR.chunking(kind, T)
            assert sum(c) == T and min(c) >= 1, (kind, T)
    assert SR.chunking("357", 47) == [3, 5, 7, 3, 5, 7, 3, 5, 7, 2] and SR.chunking("fours", 10) == [4, 4, 2]
    assert SR.tree_after([[]]) == (1, 0)
    # one hypothesis: everything is committed, its node is the root
    assert SR.tree_after([[(5, 0), (6, 2)]]) == (1, 2)
    # a prefix and its child: the ancestor is the prefix itself, never the child
    assert SR.tree_after([[(5, 0)], [(5, 0), (6, 2)]]) == (2, 1)
    # the empty prefix in the beam: nothing is committed
    assert SR.tree_after([[], [(5, 0), (6, 2)], [(5, 0), (7, 2)]]) == (4, 0)
    # the same tokens in different nodes (created on different frames) share nothing
    assert SR.tree_after([[(5, 0), (6, 2)], [(5, 1), (6, 2)]]) == (5, 0)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_compaction_cases_fit_their_capacity_and_need_the_compaction(dtype):
    """By the oracle: before every advance of the GPU test ``live + frames x W <= NC`` holds, while the nodes the whole
    utterance creates (search_one's third return) exceed NC - without compaction the case would be refused."""
    for shape, step, NC in SR.COMPACTION:
        T, V, W, cand = shape
        z, hyps, _, nodes = BR.case(shape, dtype)
        trace, live = SR.capacity_trace(z, W, cand, step, BR.search_one)
        assert len(trace) >= 2 and sum(n for _, n in trace) == T
        assert all(lv + n * W <= NC for lv, n in trace), (shape, NC, max(lv + n * W for lv, n in trace))
        assert nodes > NC >= W, (shape, nodes, NC)
        print("compaction", shape, dtype, "nodes created %d, capacity %d, most needed %d, live at the end %d"
              % (nodes, NC, max(lv + n * W for lv, n in trace), live))
