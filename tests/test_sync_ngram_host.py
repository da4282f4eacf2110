"""Host tests (no GPU) of the back-off n-gram in the frame-synchronous beam search: the oracle glue
tests/sync_ngram_ref.py (``NGramAdapter`` against ``NGramLM.score`` / ``step``), the Python entry points' argument rules,
the native entry points' - with fake pointers, every call fails a check before the device is touched - and the margin
assertions of every oracle case tests/test_sync_ngram_gpu.py compares the device with, so that a bad working point is
found here."""
import ctypes

import numpy as np
import pytest
import torch

import ngram_ref as NR
import sync_ngram_ref as R
from search_abi import SEARCH_ENTRY_POINTS, assert_search_surface, make_opts
from test_search_abi_host import _Calls, _lm, _stream_advance
from test_sync_beam_host import CFG

V = 40


# ------------------------------------------------------------------------------------------- the adapter
@pytest.mark.parametrize("which", ["model", "wide", "closure"])
def test_adapter_chain_is_score_and_the_state_sequence_of_step(which):
    """Chaining ``forward`` over a token list gives ``NGramLM.score(tokens)`` bit for bit (the same float64 additions
    in the same order) and the states of repeated ``step``; ``lm_bos`` is not read."""
    lm = {"model": lambda: NR.model(40, 3), "wide": NR.wide_model, "closure": NR.closure_model}[which]()
    ad = R.NGramAdapter(lm)
    assert ad.zero() is None
    rng = np.random.default_rng(11)
    fixed = {"model": [NR.corpus(40)[0], NR.corpus(40)[5]], "wide": [[3, 17], [200, 3, 519], [3, 149, 3, 10]],
             "closure": [[5, 6, 7, 8], [5, 6, 7, 9], [7, 7], [6, 7, 8]]}[which]
    lists = fixed + [[int(k) for k in rng.integers(3, lm.V, size=n)] for n in (0, 1, 2, 5, 9, 14)]
    for toks in lists:
        for bos_tok in (1, 7):
            lp, hidden = ad.forward(torch.tensor([[bos_tok]]), None)
            assert hidden == lm.start and lp.dtype == torch.float64 and tuple(lp.shape) == (1, lm.V)
            assert lp[0, lm.blank].item() == 0.0
            total, s, states = 0.0, lm.start, [lm.start]
            for k in toks:
                total = total + float(lp[0, k])
                want_l, s = lm.step(s, k)
                assert float(lp[0, k]) == want_l
                lp, hidden = ad.forward(torch.tensor([[k]]), hidden)
                states.append(hidden)
                assert hidden == s
            assert total == lm.score(toks), (toks, total, lm.score(toks))
            assert len(states) == len(toks) + 1


# ------------------------------------------------------------------------------------------- the Python entry points
def _calls(m, cfg):
    from edgedict_amd import decode
    from edgedict_amd.flags import make_flags
    from edgedict_amd.stream import BatchedStreamSyncFusionBeamDecoder
    xs = torch.zeros(2, 8, cfg["input_size"])
    enc = torch.zeros(2, 4, cfg["enc_proj_size"])
    e1 = torch.zeros(8, cfg["joint_size"])
    P = cfg["enc_proj_size"]
    flags = make_flags("E6D2")
    return [lambda **kw: m.sync_beam_search(xs, None, 4, **kw), lambda **kw: m.sync_beam_search_nbest(xs, None, 4, **kw),
            lambda **kw: decode.sync_beam_search_fusion(m, xs, None, 4, **kw),
            lambda **kw: decode.sync_beam_search_nbest(m, xs, None, 4, **kw),
            lambda **kw: decode.sync_beam_search_enc(m, enc, None, 4, **kw),
            lambda **kw: decode.sync_beam_search_nbest_enc(m, enc, None, 4, **kw),
            lambda **kw: decode.sync_beam_search_rows(m, e1, 2, 4, P, None, 4, **kw),
            lambda **kw: decode.sync_beam_search_nbest_rows(m, e1, 2, 4, P, None, 4, **kw),
            lambda **kw: decode.StreamingSyncFusionBeamSearch(m, 2, W=4, **kw),
            lambda **kw: BatchedStreamSyncFusionBeamDecoder(m, flags, 2, W=4, dither=0, **kw)]


def test_python_entry_points_check_the_ngram_arguments_first():
    """On a CPU model: every n-gram argument error is a ValueError raised before the device is asked for."""
    from edgedict_amd import decode
    from edgedict_amd.bias import ContextGraph
    from edgedict_amd.models import Transducer
    from edgedict_amd.ngram import SYNC_NGRAM_MAX_V, NGramLM
    m = Transducer(enc_dropout=0.0, dec_dropout=0.0, output_loss=False, **CFG).eval()
    lm = NR.model(V, 3)
    lm_other = NGramLM.train([[3, 4, 5]], 2, V + 1)
    lm_blank = NGramLM.train([[3, 4, 5]], 2, V, blank=1)
    for call in _calls(m, CFG):
        with pytest.raises(ValueError, match="lm_weight is required"):
            call(lm=lm)
        for bad in (-0.5, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="lm_weight must be a finite number >= 0"):
                call(lm=lm, lm_weight=bad)
        for bad in (float("inf"), float("-inf"), float("nan")):
            with pytest.raises(ValueError, match="length_bonus must be finite"):
                call(lm=lm, lm_weight=0.5, length_bonus=bad)
        with pytest.raises(ValueError, match="vocab_size = 41\\) differs from the transducer's"):
            call(lm=lm_other, lm_weight=0.5)
        with pytest.raises(ValueError, match="blank \\(1\\) differs"):
            call(lm=lm_blank, lm_weight=0.5)
        with pytest.raises(ValueError, match="must be an edgedict_amd.lm.LMModel or an edgedict_amd.ngram.NGramLM"):
            call(lm=object(), lm_weight=0.5)
        # accepted arguments reach the device check; lm_bos is taken and not read
        for kw in (dict(lm=lm, lm_weight=0.5), dict(lm=lm, lm_weight=0.0, length_bonus=-1.5, lm_bos=7),
                   dict(lm=lm, lm_weight=np.float32(0.25), bias=ContextGraph([[3, 4]], 2.0, V), ilm_weight=0.2)):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                call(**kw)
    # the LDS bound: one symbol more than the image holds
    big = dict(CFG, vocab_size=SYNC_NGRAM_MAX_V + 1)
    mb = Transducer(enc_dropout=0.0, dec_dropout=0.0, output_loss=False, **big).eval()
    lm_big = NGramLM.train([[3, 4, 5]], 1, SYNC_NGRAM_MAX_V + 1)
    for call in _calls(mb, big):
        with pytest.raises(ValueError, match="exceeds %d" % SYNC_NGRAM_MAX_V):
            call(lm=lm_big, lm_weight=0.5)
    # the plain signatures stay plain, and the best-first searches keep refusing an n-gram
    xs = torch.zeros(2, 8, CFG["input_size"])
    with pytest.raises(TypeError):
        decode.sync_beam_search(m, xs, None, 4, lm=lm, lm_weight=0.5)
    for call in (lambda **kw: m.beam_search(xs, None, 4, **kw), lambda **kw: m.beam_search_nbest(xs, None, 4, **kw),
                 lambda **kw: decode.StreamingBeamSearch(m, 2, W=4, **kw)):
        with pytest.raises(ValueError, match="must be an edgedict_amd.lm.LMModel"):
            call(lm=lm, lm_weight=0.5)


# ------------------------------------------------------------------------------------------- the native entry points
def _ngram(fake, **kw):
    """An ``edgedict_ngram_lm_t`` over fake pointers: good enough for every check before a launch."""
    from edgedict_amd.ngram import _TABLES, NGramStruct
    s = NGramStruct()
    s.V, s.order, s.S, s.n_arcs, s.start, s.blank = V, 3, 7, 11, 1, 0
    for name in _TABLES:
        setattr(s, name, fake.value)
    s.weight, s.length_bonus = 0.5, 0.25
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _opts(ng=None, **kw):
    """``make_opts`` with the fourth member; the struct keeps ``ng`` alive (the other members are the caller's)."""
    o = make_opts(**kw)
    o.ngram = None if ng is None else ctypes.addressof(ng)
    o.keep = ng
    return o


SYNC_NAMES = {"edgedict_sync_beam_workspace_bytes", "edgedict_sync_beam_search", "edgedict_sync_stream_state_bytes",
              "edgedict_sync_stream_workspace_bytes", "edgedict_sync_stream_reset", "edgedict_sync_stream_advance"}


def test_the_opts_struct_grew_at_its_end_and_no_symbol_was_added(hip_lib):
    from edgedict_amd import _lib
    from edgedict_amd.decode import SearchOpts
    assert ctypes.sizeof(SearchOpts) == hip_lib.edgedict_search_struct_bytes(1) == 32
    assert [f[0] for f in SearchOpts._fields_] == ["lm", "bias", "ilm_weight", "ngram"] and SearchOpts.ngram.offset == 24
    assert hip_lib.edgedict_abi_version() == 2
    assert_search_surface(hip_lib, SYNC_NAMES)
    declared = {n for n in _lib.declared_symbols() if n.startswith(("edgedict_beam_", "edgedict_sync_"))}
    assert declared | {"edgedict_search_struct_bytes"} == SEARCH_ENTRY_POINTS | {"edgedict_beam_lm_struct_bytes",
                                                                                "edgedict_beam_bias_struct_bytes"}


def test_size_queries_with_an_ngram(hip_lib):
    c = _Calls(hip_lib)
    ng = _ngram(c.fake)
    net = ctypes.byref(c.net())                                # V 40, L 2, H 36
    none, on = None, ctypes.byref(_opts(ng))
    B, T, W, S, NC = 2, 9, 4, 3, 64
    f, g, w = (hip_lib.edgedict_sync_beam_workspace_bytes, hip_lib.edgedict_sync_stream_state_bytes,
               hip_lib.edgedict_sync_stream_workspace_bytes)
    a256 = lambda n: 256 * ((n + 255) // 256)
    # ng_st [rows] and the candidates' next states [rows][W]: nothing the size of [rows, V], no state buffers
    assert f(net, B, T, W, on) == f(net, B, T, W, none) + a256(B * W * 4) + a256(B * W * W * 4) > 0
    assert g(on, S, 2, 36, W, NC) == g(none, S, 2, 36, W, NC) + a256(S * W * 4) > 0
    assert w(net, S, W, NC, on) == w(net, S, W, NC, none) + a256(S * W * W * 4) > 0
    # appended: with a list in front, the list's part keeps its place and the n-gram's follows
    from test_sync_fusion_host import _structs
    keep, _, bias = _structs(c.fake)
    both, lst = ctypes.byref(_opts(ng, bias=bias)), ctypes.byref(_opts(bias=bias))
    assert g(both, S, 2, 36, W, NC) == g(lst, S, 2, 36, W, NC) + a256(S * W * 4)
    # refused arguments: 0
    lm = _lm(c.fake, V=V)
    bad = [dict(V=V + 1), dict(blank=1), dict(V=5377), dict(order=0), dict(order=7), dict(S=0), dict(start=7),
           dict(weight=-0.5), dict(weight=float("nan")), dict(length_bonus=float("inf")), dict(arc_lp=None)]
    for kw in bad:
        o = _opts(_ngram(c.fake, **kw))
        netk = ctypes.byref(c.net(V=5377)) if kw == dict(V=5377) else net
        assert f(netk, B, T, W, ctypes.byref(o)) == 0, kw
        assert w(netk, S, W, NC, ctypes.byref(o)) == 0, kw
        if "V" not in kw and "blank" not in kw or kw == dict(V=5377):       # (the state query knows neither V nor blank)
            assert g(ctypes.byref(o), S, 2, 36, W, NC) == 0, kw
    assert f(ctypes.byref(c.net(V=5376)), B, T, W, ctypes.byref(_opts(_ngram(c.fake, V=5376)))) > 0
    o = _opts(ng, lm=lm)
    assert f(net, B, T, W, ctypes.byref(o)) == 0 and g(ctypes.byref(o), S, 2, 36, W, NC) == 0
    assert w(net, S, W, NC, ctypes.byref(o)) == 0


def test_native_ngram_argument_errors_come_before_any_launch(hip_lib):
    """Each rule from the offline search, the streaming advance and the streaming reset: -1, and a message that the
    entry point's name leads.  No call here gets as far as the device."""
    c = _Calls(hip_lib)
    ll = ctypes.c_longlong

    def offline(o, net=None):
        return c.sync(net or c.net(), o)

    def advance(o, net=None):
        nf, live = (ctypes.c_int32 * 2)(5, 3), (ctypes.c_int32 * 2)(0, 0)
        return hip_lib.edgedict_sync_stream_advance(
            ctypes.byref(net or c.net()), c.fake, ll(5 * 32), ll(32), 2, 5, nf, 4, 64, live,
            ctypes.pointer(ctypes.c_int32(0)), c.fake, 64, ctypes.byref(o), c.fake, c.fake, None)

    def reset(o, net=None):
        return hip_lib.edgedict_sync_stream_reset(ctypes.byref(o), 2, 2, 36, 4, 64, 2, None, 0, c.fake, None)

    cases = [(dict(V=V + 1), b"V = 41"), (dict(blank=1), b"blank (1) differs"), (dict(V=5377), b"exceeds 5376"),
             (dict(order=0), b"order = 0"), (dict(order=7), b"order = 7"), (dict(S=0), b"bad n-gram tables"),
             (dict(n_arcs=-1), b"bad n-gram tables"), (dict(start=7), b"start state 7"), (dict(blank=V), b"blank 40"),
             (dict(V=1), b"V = 1"), (dict(weight=-0.5), b"weight = -0.5"), (dict(weight=float("nan")), b"weight = nan"),
             (dict(weight=float("inf")), b"weight = inf"), (dict(length_bonus=float("-inf")), b"length_bonus"),
             (dict(length_bonus=float("nan")), b"length_bonus")]
    cases += [({name: None}, b"null n-gram table pointer")
              for name in ("uni_lp", "uni_next", "row_ptr", "fail", "backoff", "arc_tok", "arc_lp", "arc_next")]
    for call, what in ((offline, b"sync_beam_search:"), (advance, b"sync_stream_advance:"),
                       (reset, b"sync_stream_reset:")):
        for kw, word in cases:
            net = c.net(V=5377) if kw == dict(V=5377) else None
            if call is reset and word in (b"V = 41", b"blank (1) differs"):
                continue            # (the reset knows neither V nor blank: the advance checks them)
            ng = _ngram(c.fake, **kw)
            assert call(_opts(ng), net) == -1, (what, kw)
            msg = c.error()
            assert msg.startswith(what) and word in msg, (what, kw, msg)
        # one LM at a time
        ng, lm = _ngram(c.fake), _lm(c.fake, V=V)
        assert call(_opts(ng, lm=lm)) == -1
        assert c.error().startswith(what) and b"one LM at a time" in c.error(), c.error()
        # the struct's address in the first page: an integer, not a pointer
        o = _opts()
        o.ngram = 8
        assert call(o) == -1 and c.error().startswith(what) and b"not a pointer" in c.error(), c.error()
        # the other checks still come first / still work with the n-gram set
        if call is not reset:       # (the reset does not read ilm_weight)
            w = ctypes.c_double(-1.0)
            assert call(_opts(_ngram(c.fake), ilm_weight=w)) == -1 and b"ilm_weight" in c.error()


def test_expansion_searches_refuse_an_ngram(hip_lib):
    """opts->ngram is the frame-synchronous search's: the four expansion entry points say so before they touch the
    device, their size queries return 0."""
    c = _Calls(hip_lib)
    ng = _ngram(c.fake)
    opts = _opts(ng)
    for call, what in ((lambda: c.beam(c.net(), opts), b"beam_search:"),
                       (lambda: c.beam(c.net(), opts, nbest=True), b"beam_search_nbest:"),
                       (lambda: _stream_advance(c, c.net(), opts), b"beam_stream_advance:")):
        assert call() == -1
        assert c.error().startswith(what) and b"ngram is not supported" in c.error(), c.error()
    assert hip_lib.edgedict_beam_stream_reset(ctypes.byref(opts), 2, 2, 36, 4, 64, 2, None, 0, c.fake, None, None) == -1
    assert b"beam_stream_reset: ngram is not supported" in c.error()
    net = ctypes.byref(c.net())
    assert hip_lib.edgedict_beam_workspace_bytes(net, 2, 5, 4, 16, 0, None) > 0
    assert hip_lib.edgedict_beam_workspace_bytes(net, 2, 5, 4, 16, 0, ctypes.byref(opts)) == 0
    assert hip_lib.edgedict_beam_stream_state_bytes(ctypes.byref(opts), 2, 2, 36, 4, 64) == 0
    assert hip_lib.edgedict_beam_stream_workspace_bytes(net, 2, 4, 16, 64, ctypes.byref(opts)) == 0


# ------------------------------------------------------------------------------------------- the working points
@pytest.mark.parametrize("W", R.WIDTHS)
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("name", R.NAMES)
def test_every_gpu_case_is_decisive_on_the_oracle(name, mode, W):
    import sync_beam_ref as S
    from test_sync_beam_gpu import _inputs
    ref, infos = R.reference(name, mode, W)
    R.assert_decisive(infos, W, ref)
    sd, xs, xlen = _inputs(name)
    plain, _ = S.search(sd, xs, xlen, W)
    assert sum(r[0]["tokens"] != p[0]["tokens"] for r, p in zip(ref, plain)) >= 1      # the fusion acts on a best one


@pytest.mark.parametrize("edge", list(R.EDGES))
def test_every_back_off_edge_is_decisive_and_reaches_its_edge(edge):
    ref, infos = R.edge_reference(edge)
    R.assert_decisive(infos, R.EDGES[edge][2], ref)
    lm = R.edge_lm(edge)
    assert lm.V == R.EDGES[edge][1]
    hyps = [h for r in ref for h in r]
    T = 5

    def state(tokens):
        s = lm.start
        for k in tokens:
            s = lm.step(s, k)[1]
        return s

    # rows that were in the beam for at least one frame after their last token: the top-W kernel filled their image
    sat = [state(h["tokens"]) for h in hyps if h["tokens"] and h["frames"][-1] < T - 1]
    if edge == "order1":
        assert lm.order == 1 and lm.n_arcs == 0 and lm.n_states == 1
    if edge == "order6":
        assert lm.order == 6 and max(len(lm.contexts[s]) for s in sat) >= 2 and max(len(h["tokens"]) for h in hyps) >= 4
    if edge == "wide":
        s3 = lm._index[(3,)]
        assert lm.row_ptr[s3 + 1] - lm.row_ptr[s3] >= 140 and s3 in sat
    if edge == "closure":
        bare = [s for s in sat if s != 0 and lm.row_ptr[s + 1] == lm.row_ptr[s]]
        assert bare and any(lm.backoff[s] != 0.0 for s in bare)
    if edge == "longest":
        s1, s2 = lm._index[(17,)], lm._index[(17, 17)]
        bi, tri = lm.step(s1, 17)[0], lm.step(s2, 17)[0]
        w = R.EDGES[edge][3]
        assert w * abs(tri - bi) > 1.0          # the bigram's value in the trigram's place would move logp by > 1
        assert s2 in sat and any(h["tokens"][:3] == [17, 17, 17] for h in hyps)
