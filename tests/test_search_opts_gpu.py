"""GPU: an ``edgedict_search_opts_t`` whose three members are null is the null ``opts`` pointer (include/edgedict_hip.h) -
the one path the Python API never takes, since ``decode._opts`` passes null when no feature is asked for.  The native
offline expansion search and the native frame-synchronous search, called once each way on the committed trained tiny
model (tests/golden/beam_tiny.npz; fp32, B = 2, T = 6, W = 4): tokens, token counts, scores and expansion counts
bit-identical between the two calls and to what the Python API returns for the same rows."""
import ctypes
import os

import numpy as np
import pytest
import torch

from search_abi import make_opts

pytestmark = pytest.mark.gpu
CFG = dict(vocab_embed_size=16, vocab_size=40, input_size=24, enc_hidden_size=32, enc_layers=2,
           enc_proj_size=24, dec_hidden_size=32, dec_layers=2, dec_proj_size=24, joint_size=32)
B, T, W = 2, 6, 4
G = np.load(os.path.join(os.path.dirname(__file__), "golden", "beam_tiny.npz"))


def test_all_null_opts_is_the_null_opts_pointer(hip_lib):
    from edgedict_amd import _lib, decode
    from edgedict_amd.models import Transducer
    sd = {k[3:]: torch.from_numpy(G[k]) for k in G.files if k.startswith("sd/")}
    xs = torch.from_numpy(G["xs"])[:B, :2 * T]         # the encoder halves the frame rate
    m = Transducer(enc_dropout=0.0, dec_dropout=0.0, output_loss=False, **CFG)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    m.compute_dtype = "fp32"
    with torch.no_grad():
        enc, _ = m.encoder(xs.cuda())
        enc = enc.contiguous()
        assert enc.shape[:2] == (B, T) and enc.dtype == torch.float32
        P = enc.shape[2]
        E1 = decode.joint_rows(m, enc)
    net = decode._SearchNet(m, torch.float32)
    nref = net.ref(P)
    lens = np.array([T, T - 2], dtype=np.int32)
    EM = 8 * W
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    e1 = (_lib.ptr(E1), ctypes.c_longlong(T * net.J), ctypes.c_longlong(net.J), B, T, vp(lens))
    empty = make_opts()
    assert (empty.lm, empty.bias, empty.ilm_weight) == (None, None, None)

    def expansion(opts):
        nbytes = hip_lib.edgedict_beam_workspace_bytes(nref, B, T, W, EM, 0, opts)
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        MT = T * EM + 1
        tokens, ntok = np.zeros((B, MT), dtype=np.int32), np.zeros(B, dtype=np.int32)
        score, nexp = np.zeros(B, dtype=np.float64), ctypes.c_longlong(-1)
        rc = hip_lib.edgedict_beam_search(nref, *e1, W, EM, 0, vp(tokens), MT, vp(ntok), vp(score), ctypes.byref(nexp),
                                          opts, _lib.ptr(ws), _lib.stream_ptr())
        _lib.check(rc, "beam_search")
        return nbytes, tokens, ntok, score, nexp.value

    def synchronous(opts):
        nbytes = hip_lib.edgedict_sync_beam_workspace_bytes(nref, B, T, W, opts)
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        res = torch.empty(hip_lib.edgedict_sync_beam_result_bytes(B, W, T), dtype=torch.uint8, device="cuda")
        tokens, frames = np.zeros((B, W, T), dtype=np.int32), np.zeros((B, W, T), dtype=np.int32)
        tlogp, logp = np.zeros((B, W, T), dtype=np.float64), np.zeros((B, W), dtype=np.float64)
        ntok, nhyp = np.zeros((B, W), dtype=np.int32), np.zeros(B, dtype=np.int32)
        rc = hip_lib.edgedict_sync_beam_search(nref, *e1, W, vp(tokens), vp(frames), vp(tlogp), T, vp(ntok), vp(nhyp),
                                               vp(logp), opts, _lib.ptr(ws), _lib.ptr(res), _lib.stream_ptr())
        _lib.check(rc, "sync_beam_search")
        # (columns behind a hypothesis' length are not written by the call: compare what it defines)
        for b in range(B):
            for h in range(W):
                n = ntok[b, h] if h < nhyp[b] else 0
                tokens[b, h, n:], frames[b, h, n:], tlogp[b, h, n:] = 0, 0, 0.0
        return nbytes, tokens, frames, tlogp, ntok, nhyp, logp

    # ---- the expansion search
    null, allnull = expansion(None), expansion(ctypes.byref(empty))
    assert null[0] == allnull[0] > 0 and null[4] == allnull[4] > 0
    for a, b in zip(null[1:4], allnull[1:4]):
        assert np.array_equal(a, b)
    seqs, score = decode.beam_search_rows(m, E1, B, T, P, lens, W, EM)
    assert decode.beam_search_batch.last_expansions == null[4]
    assert np.array_equal(score.numpy(), null[3])
    assert sum(len(s) for s in seqs) > 0
    for b in range(B):
        assert np.array_equal(seqs[b], null[1][b, :null[2][b]].astype(np.int64)), b

    # ---- the frame-synchronous search
    null, allnull = synchronous(None), synchronous(ctypes.byref(empty))
    assert null[0] == allnull[0] > 0
    for a, b in zip(null[1:], allnull[1:]):
        assert np.array_equal(a, b)
    want = decode.sync_beam_search_nbest_rows(m, E1, B, T, P, lens, W)
    got = decode._nbest_results(*null[1:])
    assert len(want) == len(got) == B
    for g, w in zip(got, want):
        assert len(g) == len(w) >= 1
        assert np.array_equal(g.logp, w.logp)
        for i in range(len(g)):
            assert np.array_equal(g.tokens[i], w.tokens[i]) and np.array_equal(g.frames[i], w.frames[i])
            assert np.array_equal(g.token_logp[i], w.token_logp[i])
    assert sum(len(g.tokens[0]) for g in got) > 0
