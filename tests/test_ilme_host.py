"""Host tests (no GPU) of internal-LM estimation: the oracle tests/ilme_ref.py - the contract of sync_row_topw_ilm
(csrc/decode_sync.hip) and of csrc/ilm_score.hip -, the argument rules of every Python entry point that takes
``ilm_weight``, and the argument checks of the edgedict_*_ilme / edgedict_ilm_* entry points, which come before any
launch."""
import ctypes
import math

import numpy as np
import pytest
import torch

import ilme_ref as I
import sync_fusion_ref as F
from oracle import models_ref as M
from test_lm_fusion_gpu import RefLM, _lm_sd
from test_sync_beam_gpu import _inputs
from test_sync_beam_host import CFG
from test_sync_fusion_host import _fake, _structs

V = 40
LM_W, LM_B = 0.6, 0.3           # tests/test_sync_fusion_gpu.py's LM working point
ILM_W = 0.6                     # CFG, W = 4, with that LM: the best hypothesis of all 3 utterances changes (oracle)


def _lm():
    return RefLM(_lm_sd(V, 16, 32, 2, seed=2, scale=4.0))


# ------------------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("raise_blank", [0.0, 10.0])
def test_the_internal_lm_is_a_distribution_over_the_non_blank_symbols(raise_blank):
    """exp(lp_ilm) over the non-blank symbols sums to 1 - also when the blank would own the maximum."""
    sd, _, _ = _inputs("CFG")
    sd = dict(sd)
    sd["joint.joint.2.bias"] = sd["joint.joint.2.bias"].clone()
    sd["joint.joint.2.bias"][M.NUL] += raise_blank
    ilm = I.model_ilm(sd)
    L, H = M.n_dec_layers(sd), sd["decoder.lstm.weight_hh_l0"].shape[1]
    state = (torch.zeros(L, 1, H), torch.zeros(L, 1, H))
    for tok in (M.BOS, 5, 39):
        lp = ilm(tok, state)
        assert lp[M.NUL] is None and len(lp) == V
        assert abs(sum(math.exp(v) for k, v in enumerate(lp) if k != M.NUL) - 1.0) <= 1e-12
        if raise_blank:
            z = M.joint_forward(sd, torch.zeros(1, CFG["enc_proj_size"]),
                                M.decoder_forward(sd, torch.tensor([[tok]]), state)[0][:, 0])[0]
            assert int(z.argmax()) == M.NUL         # the blank does own the maximum of the raw logits
    # teacher-forced: position 0 is the row after BOS
    got = I.ilm_logprobs(sd, torch.tensor([[5, 7]]), [1])
    assert abs(got[0][0] - ilm(M.BOS, state)[5]) <= 1e-6 and got[0][1] == 0.0


@pytest.mark.parametrize("W", [1, 4, 10])
@pytest.mark.parametrize("with_lm", [False, True])
def test_weight_zero_is_the_oracle_without_ilme(W, with_lm):
    sd, xs, xlen = _inputs("CFG")
    kw = dict(lm=_lm(), lm_weight=LM_W, length_bonus=LM_B) if with_lm else {}
    want, winfo = F.search(sd, xs, xlen, W, F.Fusion(**kw))
    got, info = I.search(sd, xs, xlen, W, I.Fusion(ilm=I.model_ilm(sd), ilm_weight=0.0, **kw))
    assert got == want and info == winfo
    none, ninfo = I.search(sd, xs, xlen, W, I.Fusion(ilm=None, ilm_weight=None, **kw))
    assert none == want and ninfo == winfo


def test_ilme_changes_a_best_hypothesis_against_lm_only_and_streams():
    W = 4
    sd, xs, xlen = _inputs("CFG")
    kw = dict(lm=_lm(), lm_weight=LM_W, length_bonus=LM_B)
    lm_only, _ = F.search(sd, xs, xlen, W, F.Fusion(**kw))
    fusion = I.Fusion(ilm=I.model_ilm(sd), ilm_weight=ILM_W, **kw)
    got, infos = I.search(sd, xs, xlen, W, fusion)
    assert sum(a[0]["tokens"] != b[0]["tokens"] for a, b in zip(got, lm_only)) >= 1
    assert sum(i["merges"] for i in infos) >= 1
    # the chunked oracle equals the offline one
    import sync_beam_ref as S
    h_enc, lens = S.encode(sd, xs, xlen)
    for split in ([1] * int(lens[0]), [3, 0, int(lens[0]) - 3]):
        st = I.stream_search(sd, h_enc[0, :lens[0]], W, fusion)
        for n in split:
            st.advance(n)
        assert st.beam() == got[0]


# ------------------------------------------------------------------------------------------- the Python entry points
def test_python_entry_points_check_ilm_weight_first():
    """On a CPU model: a bad ``ilm_weight`` is a ValueError raised before the device is asked for; a good one gets as
    far as "no CPU fallback"; the best-first searches refuse the keyword."""
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
    lm = LMModel(V, 16, 32, 2, dropout=0.0)
    for call in calls:
        for bad in (-0.1, float("inf"), float("-inf"), float("nan"), "0.3", [0.3], True):
            with pytest.raises(ValueError, match="ilm_weight"):
                call(ilm_weight=bad)
            with pytest.raises(ValueError, match="ilm_weight"):
                call(ilm_weight=bad, lm=lm, lm_weight=0.5)
        for kw in (dict(ilm_weight=0.0), dict(ilm_weight=0.3), dict(ilm_weight=1, lm=lm, lm_weight=0.5),
                   dict(ilm_weight=np.float32(0.25), bias=ContextGraph([[3, 4]], 2.0, V)), dict(ilm_weight=None)):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                call(**kw)
    # the plain signatures stay plain
    for call in (lambda **kw: decode.sync_beam_search(m, xs, None, 4, **kw),
                 lambda **kw: decode.StreamingSyncBeamSearch(m, 2, W=4, **kw)):
        with pytest.raises(TypeError):
            call(ilm_weight=0.3)
    # the best-first search has another expand kernel
    for call in (lambda **kw: m.beam_search(xs, None, 4, **kw), lambda **kw: m.beam_search_nbest(xs, None, 4, **kw)):
        with pytest.raises(ValueError, match="ilm_weight is not supported"):
            call(ilm_weight=0.3)
    with pytest.raises(TypeError):
        decode.beam_search_batch(m, xs, None, 4, ilm_weight=0.3)
    # the scorer: shapes first, then the device
    with pytest.raises(ValueError, match="ys must be"):
        m.ilm_logprobs(torch.zeros(3, dtype=torch.int64), torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="ylen must be"):
        m.ilm_score(torch.zeros(3, 2, dtype=torch.int64), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.ilm_score(torch.full((3, 2), 5, dtype=torch.int64), torch.tensor([2, 1, 0]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        decode.ilm_logits(m, torch.zeros(4, CFG["dec_proj_size"]))


# ------------------------------------------------------------------------------------------- the native entry points
NAMES = {"edgedict_sync_beam_workspace_bytes", "edgedict_sync_beam_search", "edgedict_sync_stream_workspace_bytes",
         "edgedict_sync_stream_advance"}
ILM_NAMES = {"edgedict_ilm_workspace_bytes", "edgedict_ilm_logits", "edgedict_ilm_logprobs"}


def test_ilme_symbols_are_declared_exported_and_sized(hip_lib):
    from edgedict_amd import _lib
    from edgedict_amd.lm import BeamLM
    from search_abi import assert_search_surface, make_net, make_opts
    assert_search_surface(hip_lib, NAMES)
    assert ILM_NAMES <= set(_lib.declared_symbols())
    for name in ILM_NAMES:
        assert hasattr(hip_lib, name), name
    assert hip_lib.edgedict_beam_lm_struct_bytes() == ctypes.sizeof(BeamLM)         # the mirrored struct kept its size
    buf, fake = _fake()
    keep, lm, bias = _structs(fake)
    w = ctypes.c_double(0.3)
    opts = lambda lm=None, bias=None, w=None: ctypes.byref(make_opts(lm, bias, w))
    f = hip_lib.edgedict_sync_beam_workspace_bytes
    assert f.restype is ctypes.c_size_t
    net = ctypes.byref(make_net(V=V))                  # fp32, J 32, E 16, L 2, H 32, P2 24
    dims = (net, 2, 9, 4)                              # B, T, W
    rows, J = 2 * 4, 32
    assert f(*dims, opts()) == f(*dims, None) > 0
    for fa in ((None, None), (lm, None), (None, bias), (lm, bias)):
        # ILME adds hidden vectors and fp32 logits for twice the rows, and a zero encoder row
        extra = f(*dims, opts(*fa, w)) - f(*dims, opts(*fa))
        assert 2 * rows * (J + V) * 4 + J * 4 <= extra <= 2 * rows * (J + V) * 4 + J * 4 + 3 * 255
        assert f(*dims, opts(*fa, w)) % 256 == 0
    for bad in (-0.5, float("nan"), float("inf")):
        assert f(*dims, opts(w=ctypes.c_double(bad))) == 0
    assert f(ctypes.byref(make_net(V=V, H=30)), 2, 9, 4, opts(w=w)) == 0       # H no multiple of 4
    assert f(net, 2, 9, 33, opts(w=w)) == 0                                    # W = 33
    _, lm_bad, _ = _structs(fake, lm_V=V + 1)
    assert f(*dims, opts(lm_bad, None, w)) == 0
    fs = hip_lib.edgedict_sync_stream_workspace_bytes
    assert fs.restype is ctypes.c_size_t
    wdims = (net, 3, 4, 64)                            # S, W, NC
    assert fs(*wdims, opts()) == fs(*wdims, None) > 0
    assert fs(*wdims, opts(lm, bias, w)) > fs(*wdims, opts(lm, bias)) and fs(*wdims, opts(w=w)) > fs(*wdims, None)
    assert fs(*wdims, opts(w=ctypes.c_double(-1.0))) == 0
    assert fs(net, 3, 4, 2, opts(w=w)) == 0                                    # node_capacity < W
    # ILME carries no per-row state: the state's size does not see the weight
    g = hip_lib.edgedict_sync_stream_state_bytes
    assert g(opts(w=w), 3, 2, 32, 4, 64) == g(None, 3, 2, 32, 4, 64) > 0
    q = hip_lib.edgedict_ilm_workspace_bytes
    assert q.restype is ctypes.c_size_t
    assert q(0, 10, 32) >= 2 * 10 * 32 * 4 + 32 * 4 and q(1, 10, 32) < q(0, 10, 32)
    assert q(0, 0, 32) == 0 and q(0, 10, 0) == 0 and q(7, 10, 32) == 0


def test_native_ilme_argument_errors_come_before_any_launch(hip_lib):
    buf, fake = _fake()
    layers = (ctypes.c_void_p * 2)(fake.value, fake.value)
    lens = (ctypes.c_int32 * 2)(5, 3)

    from search_abi import make_net, make_opts
    net = ctypes.byref(make_net(fake, V=V, w_ih=layers, w_hh=layers, b_ih=layers, b_hh=layers))

    def offline(lm, bias, w, W=4):
        return hip_lib.edgedict_sync_beam_search(
            net, fake, ctypes.c_longlong(5 * 32), ctypes.c_longlong(32), 2, 5, lens, W, fake, fake, fake, 5, fake, fake,
            fake, ctypes.byref(make_opts(lm, bias, w)), fake, fake, None)

    def advance(lm, bias, w, W=4):
        nf, live = (ctypes.c_int32 * 2)(5, 3), (ctypes.c_int32 * 2)(0, 0)
        return hip_lib.edgedict_sync_stream_advance(
            net, fake, ctypes.c_longlong(5 * 32), ctypes.c_longlong(32), 2, 5, nf, W, 64, live,
            ctypes.pointer(ctypes.c_int32(0)), fake, 64, ctypes.byref(make_opts(lm, bias, w)), fake, fake, None)

    keep, lm, bias = _structs(fake)
    good = ctypes.c_double(0.3)
    for call, what in ((offline, b"sync_beam_search"), (advance, b"sync_stream_advance")):
        for bad in (-0.25, float("nan"), float("inf"), float("-inf")):
            for fa in ((None, None), (lm, bias)):
                assert call(*fa, ctypes.c_double(bad)) == -1
                msg = hip_lib.edgedict_last_error()
                assert msg.startswith(what) and b"ilm_weight" in msg, msg
        # the fusion checks still come, with a good weight
        _, lm_bad, _ = _structs(fake, lm_V=V + 1)
        assert call(lm_bad, None, good) == -1 and b"ntoken = 41" in hip_lib.edgedict_last_error()
        assert call(None, None, good, W=33) == -1 and b"W = 33" in hip_lib.edgedict_last_error()
    # the scorer
    assert hip_lib.edgedict_ilm_logits(0, None, 4, 24, 32, fake, ctypes.c_longlong(56), fake, fake, fake, V, 0, 16, 32,
                                       fake, fake, None) == -1
    assert b"ilm_logits: null pointer" in hip_lib.edgedict_last_error()
    assert hip_lib.edgedict_ilm_logits(0, fake, 0, 24, 32, fake, ctypes.c_longlong(56), fake, fake, fake, V, 0, 16, 32,
                                       fake, fake, None) == -1
    assert b"ilm_logits: bad shape" in hip_lib.edgedict_last_error()
    assert hip_lib.edgedict_ilm_logits(5, fake, 4, 24, 32, fake, ctypes.c_longlong(56), fake, fake, fake, V, 0, 16, 32,
                                       fake, fake, None) == -1
    assert b"bad dtype" in hip_lib.edgedict_last_error()
    assert hip_lib.edgedict_ilm_logprobs(fake, fake, fake, 2, 3, V, V, fake, None) == -1
    assert b"blank 40 outside" in hip_lib.edgedict_last_error()
    assert hip_lib.edgedict_ilm_logprobs(fake, None, fake, 2, 3, V, 0, fake, None) == -1
    assert b"ilm_logprobs: null pointer" in hip_lib.edgedict_last_error()
    assert hip_lib.edgedict_ilm_logprobs(fake, fake, fake, 2, 0, V, 0, fake, None) == -1
    assert b"ilm_logprobs: bad shape" in hip_lib.edgedict_last_error()
