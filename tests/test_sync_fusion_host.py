"""Host tests (no GPU) of the fused frame-synchronous search's oracle tests/sync_fusion_ref.py - the contract of the
*_fused kernels of csrc/decode_sync.hip - and of the argument checks of the edgedict_sync_*_fusion entry points, which
come before any launch."""
import ctypes

import numpy as np
import pytest
import torch

import sync_beam_ref as S
import sync_fusion_ref as F
from bias_ref import BruteBias
from test_lm_fusion_gpu import RefLM, _lm_sd
from test_sync_beam_host import CFG, _table_model

V = 40
PHRASES = [(5, 9, 3), (5, 9, 7, 6), (9, 3), (11,)]


def _lm():
    return RefLM(_lm_sd(V, 16, 32, 2, seed=2, scale=4.0))


# ------------------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("W,seed,T", [(1, 3, 6), (4, 5, 7), (10, 7, 6)])
def test_without_fusion_the_oracle_is_search_core(W, seed, T):
    """Weight 0, bonus 0 and no list - with the LM present, so the terms are there and vanish: lists, frames, floats."""
    _, expand = _table_model(V, seed)
    want, winfo = S.search_core(T, W, expand, (), -1, blank=0)
    for fusion in (F.Fusion(), F.Fusion(lm=_lm(), lm_weight=0.0, length_bonus=0.0), F.Fusion(bias=BruteBias([], 2.0))):
        _, expand = _table_model(V, seed)
        got, info = F.search_core(T, W, expand, (), -1, fusion, blank=0)
        assert got == want
        assert {k: info[k] for k in winfo} == winfo and info["retractions"] == 0


def test_width_one_with_a_list_adds_the_sequence_bias():
    """At W = 1 nothing merges: logp is the path's RNN-T log-probs plus ``BruteBias.score`` of its tokens."""
    bias = BruteBias(PHRASES, 3.0)
    n_biased = 0
    for seed in range(6):
        T = 8
        lp, expand = _table_model(V, seed)
        got, info = F.search_core(T, W=1, expand=expand, root_state=(), root_tok=-1, fusion=F.Fusion(bias=bias), blank=0)
        assert len(got) == 1 and info["merges"] == 0
        h = got[0]
        seq, total = (), 0.0
        for t in range(T):
            if t in h["frames"]:
                k = h["tokens"][h["frames"].index(t)]
                total += lp(t, seq)[k]
                seq = seq + (k,)
            else:
                total += lp(t, seq)[0]
        assert list(seq) == h["tokens"]
        assert abs(h["logp"] - (total + bias.score(h["tokens"]))) <= 1e-12
        n_biased += bias.score(h["tokens"]) != 0.0
    assert n_biased >= 1


def test_context_graph_tables_reproduce_the_brute_force_increments():
    from edgedict_amd.bias import ContextGraph
    boosts = [None, 1.5, None, 0.5]
    bias = BruteBias(PHRASES, 2.0, boosts)
    graph = ContextGraph([list(p) for p in PHRASES], 2.0, V, phrase_boosts=boosts)
    fusion = F.Fusion(bias=bias)
    for W, seed in ((4, 1), (10, 2), (32, 3)):
        _, expand = _table_model(V, seed)
        F.search_core(6, W, expand, (), -1, fusion, blank=0)
    assert len({s for s, _ in fusion.visited}) >= 3 and len(fusion.visited) >= 3 * (V - 1)

    def sid(path):
        s = 0
        for k in path:
            s = graph.goto(s, k)
        return s

    for path, k in fusion.visited:
        assert abs(graph.delta(sid(path), k) - bias.delta(path, k)) <= 1e-12, (path, k)
        assert graph.goto(sid(path), k) == sid(bias.state(path + (k,))), (path, k)


@pytest.mark.parametrize("W,seed", [(4, 15), (10, 14)])
def test_chunked_oracle_equals_the_offline_oracle(W, seed):
    """Table seeds whose searches merge (2 and 1 merges; the second also holds a retraction)."""
    T = 9
    fuse = dict(lm_weight=0.6, length_bonus=0.3, lm_bos=1)
    lm, bias = _lm(), BruteBias(PHRASES, 2.5)
    _, expand = _table_model(V, seed)
    want, winfo = F.search_core(T, W, expand, (), -1, F.Fusion(lm=lm, bias=bias, **fuse), blank=0)
    for split in ([1] * T, [2, 3, 1, 3], [4, 0, 5]):
        _, expand = _table_model(V, seed)
        st = F.StreamSearch(W, expand, (), -1, F.Fusion(lm=lm, bias=bias, **fuse), blank=0)
        for n in split:
            st.advance(n)
        assert st.beam() == want
        assert (st.margin, st.merges, st.retractions) == (winfo["margin"], winfo["merges"], winfo["retractions"])
    assert winfo["merges"] >= 1


# ------------------------------------------------------------------------------------------- the native entry points
NAMES = {"edgedict_sync_beam_workspace_bytes", "edgedict_sync_beam_search", "edgedict_sync_stream_state_bytes",
         "edgedict_sync_stream_workspace_bytes", "edgedict_sync_stream_reset", "edgedict_sync_stream_advance"}


def _fake():
    buf = ctypes.create_string_buffer(4096)
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def _structs(fake, lm_V=V, lm_H=32, bias_V=V, weight=0.5, null_lm=None, null_bias=None):
    """(keep-alive, BeamLM, BeamBias) whose pointers are all ``fake``: good enough for every check before a launch."""
    from edgedict_amd.bias import BeamBias
    from edgedict_amd.lm import BeamLM
    layers = (ctypes.c_void_p * 2)(fake.value, fake.value)
    lp = ctypes.cast(layers, ctypes.c_void_p).value
    lm = BeamLM()
    lm.L, lm.E, lm.H, lm.V = 2, 16, lm_H, lm_V
    lm.emb, lm.emb_dtype, lm.Wo, lm.bo = fake.value, 0, fake.value, fake.value
    lm.w_ih = lm.w_hh = lm.b_ih = lm.b_hh = lp
    lm.bos, lm.weight, lm.length_bonus = 1, weight, 0.0
    if null_lm:
        setattr(lm, null_lm, None)
    bias = BeamBias()
    bias.S, bias.V, bias.n_exc = 3, bias_V, 0
    for name in ("root_next", "held", "pend", "row_ptr", "exc_tok", "exc_next"):
        setattr(bias, name, fake.value)
    if null_bias:
        setattr(bias, null_bias, None)
    return layers, lm, bias


def test_fusion_symbols_are_declared_exported_and_sized(hip_lib):
    from search_abi import assert_search_surface, make_net, make_opts
    assert_search_surface(hip_lib, NAMES)
    buf, fake = _fake()
    keep, lm, bias = _structs(fake)
    none, empty = None, ctypes.byref(make_opts())
    rl, rb, rlb = (ctypes.byref(make_opts(**kw)) for kw in (dict(lm=lm), dict(bias=bias), dict(lm=lm, bias=bias)))
    net = ctypes.byref(make_net())                      # J 32, V 40, E 16, L 2, H 32, P2 24, fp32
    f = hip_lib.edgedict_sync_beam_workspace_bytes
    assert f.restype is ctypes.c_size_t
    dims = (net, 2, 9, 4)                               # B, T, W
    plain = f(*dims, none)
    assert f(*dims, empty) == plain > 0
    rows = 2 * 4
    # a list adds the rows' automaton states, an LM at least both (h, c) buffers and the LM's logits
    assert plain < f(*dims, rb) <= plain + 256 * ((rows * 4 + 255) // 256)
    assert f(*dims, rl) >= plain + 4 * rows * 2 * 32 * 4 + rows * V * 4
    assert f(*dims, rlb) > f(*dims, rl) and f(*dims, rlb) % 256 == 0
    _, lm_bad, _ = _structs(fake, lm_V=V + 1)
    assert f(*dims, ctypes.byref(make_opts(lm=lm_bad))) == 0
    g = hip_lib.edgedict_sync_stream_state_bytes
    assert g.restype is ctypes.c_size_t
    sdims = (3, 2, 32, 4, 64)                           # S, L, H, W, NC (behind opts)
    splain = g(none, *sdims)
    assert g(empty, *sdims) == splain > 0
    assert g(rl, *sdims) >= splain + 4 * (3 * 4) * 2 * 32 * 4 and splain < g(rb, *sdims) < g(rlb, *sdims)
    assert g(rlb, 3, 2, 32, 33, 64) == 0
    w = hip_lib.edgedict_sync_stream_workspace_bytes
    assert w.restype is ctypes.c_size_t
    wdims = (net, 3, 4, 64)                             # S, W, NC
    wplain = w(*wdims, none)
    assert w(*wdims, empty) == wplain == w(*wdims, rb) > 0 and w(*wdims, rlb) > wplain


def test_native_fusion_argument_errors_come_before_any_launch(hip_lib):
    """An LM or a list of another vocabulary, null tables, a weight that is not finite, W = 33: -1 with a message from
    the offline search, the streaming advance and the streaming reset, and no device needed to get it."""
    from search_abi import make_net, make_opts
    buf, fake = _fake()
    layers = (ctypes.c_void_p * 2)(fake.value, fake.value)
    lens = (ctypes.c_int32 * 2)(5, 3)
    net = ctypes.byref(make_net(fake, w_ih=layers, w_hh=layers, b_ih=layers, b_hh=layers))

    def offline(lm, bias, W=4):
        return hip_lib.edgedict_sync_beam_search(
            net, fake, ctypes.c_longlong(5 * 32), ctypes.c_longlong(32), 2, 5, lens, W, fake, fake, fake, 5, fake, fake,
            fake, ctypes.byref(make_opts(lm, bias)), fake, fake, None)

    def advance(lm, bias, W=4):
        nf, live = (ctypes.c_int32 * 2)(5, 3), (ctypes.c_int32 * 2)(0, 0)
        return hip_lib.edgedict_sync_stream_advance(
            net, fake, ctypes.c_longlong(5 * 32), ctypes.c_longlong(32), 2, 5, nf, W, 64, live,
            ctypes.pointer(ctypes.c_int32(0)), fake, 64, ctypes.byref(make_opts(lm, bias)), fake, fake, None)

    def reset(lm, bias, W=4):
        return hip_lib.edgedict_sync_stream_reset(ctypes.byref(make_opts(lm, bias)), 2, 2, 32, W, 64, 2, None, 0, fake, None)

    cases = [(dict(lm_V=V + 1), "lm", b"ntoken = 41"), (dict(bias_V=V + 2), "bias", b"vocabulary = 42"),
             (dict(weight=float("nan")), "lm", b"not finite"), (dict(lm_H=30), "lm", b"multiple of 4"),
             (dict(null_lm="Wo"), "lm", b"null LM pointer")]
    cases += [(dict(null_bias=n), "bias", b"null bias table pointer")
              for n in ("root_next", "held", "pend", "row_ptr", "exc_tok", "exc_next")]
    for call, what in ((offline, b"sync_beam_search"), (advance, b"sync_stream_advance"), (reset, b"sync_stream_reset")):
        for kw, which, word in cases:
            if call is reset and (b"ntoken" in word or b"vocabulary" in word):
                continue            # (the reset does not know V: the advance checks the vocabularies)
            keep, lm, bias = _structs(fake, **kw)
            for args in (((lm, None) if which == "lm" else (None, bias)), (lm, bias)):
                assert call(*args) == -1, (what, kw)
                msg = hip_lib.edgedict_last_error()
                assert word in msg and msg.startswith(what), (what, kw, msg)
        keep, lm, bias = _structs(fake)
        assert call(lm, bias, W=33) == -1
        assert b"W = 33" in hip_lib.edgedict_last_error()


# ------------------------------------------------------------------------------------------- the Python entry points
def test_python_entry_points_check_the_fusion_arguments_first():
    """On a CPU model: every fusion argument error is a ValueError raised before the device is asked for."""
    from edgedict_amd import decode
    from edgedict_amd.bias import ContextGraph
    from edgedict_amd.flags import make_flags
    from edgedict_amd.lm import LMModel
    from edgedict_amd.models import Transducer
    from edgedict_amd.stream import BatchedStreamSyncFusionBeamDecoder
    m = Transducer(enc_dropout=0.0, dec_dropout=0.0, output_loss=False, **CFG).eval()
    xs = torch.zeros(2, 8, CFG["input_size"])
    enc = torch.zeros(2, 4, CFG["enc_proj_size"])
    e1 = torch.zeros(8, CFG["joint_size"])
    P = CFG["enc_proj_size"]
    flags = make_flags("E6D2")
    calls = [lambda **kw: m.sync_beam_search(xs, None, 4, **kw), lambda **kw: m.sync_beam_search_nbest(xs, None, 4, **kw),
             lambda **kw: decode.sync_beam_search_fusion(m, xs, None, 4, **kw),
             lambda **kw: decode.sync_beam_search_nbest(m, xs, None, 4, **kw),
             lambda **kw: decode.sync_beam_search_enc(m, enc, None, 4, **kw),
             lambda **kw: decode.sync_beam_search_nbest_enc(m, enc, None, 4, **kw),
             lambda **kw: decode.sync_beam_search_rows(m, e1, 2, 4, P, None, 4, **kw),
             lambda **kw: decode.sync_beam_search_nbest_rows(m, e1, 2, 4, P, None, 4, **kw),
             lambda **kw: decode.StreamingSyncFusionBeamSearch(m, 2, W=4, **kw),
             lambda **kw: BatchedStreamSyncFusionBeamDecoder(m, flags, 2, W=4, dither=0, **kw)]
    lm, lm_other = LMModel(V, 16, 32, 2, dropout=0.0), LMModel(V + 1, 16, 32, 2, dropout=0.0)
    for call in calls:
        with pytest.raises(ValueError, match="needs lm_weight"):
            call(lm=lm)
        with pytest.raises(ValueError, match="ntoken = 41"):
            call(lm=lm_other, lm_weight=0.5)
        with pytest.raises(ValueError, match="must be an edgedict_amd.lm.LMModel"):
            call(lm=object(), lm_weight=0.5)
        with pytest.raises(ValueError, match="vocab_size = 41"):
            call(bias=ContextGraph([[3, 4]], 2.0, V + 1))
        with pytest.raises(ValueError, match="ContextGraph"):
            call(bias=[[3, 4]])
        # accepted arguments reach the device check (an empty list is "no list")
        for kw in (dict(lm=lm, lm_weight=0.5, length_bonus=0.1, lm_bos=2), dict(bias=ContextGraph([[3, 4]], 2.0, V)),
                   dict(bias=ContextGraph([], 2.0, V)), dict(lm=None, bias=None)):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                call(**kw)
