"""CPU: the frame-synchronous beam search's oracle (tests/sync_beam_ref.py) against a brute-force sum over paths and
against the greedy oracle, and the argument rules of the native and Python entry points (csrc/decode_sync.hip,
decode.sync_beam_search*): everything that needs no device."""
import ctypes
import itertools
import math

import numpy as np
import pytest
import torch

import sync_beam_ref as S
from oracle import models_ref as M

CFG = dict(vocab_embed_size=16, vocab_size=40, input_size=24, enc_hidden_size=32, enc_layers=2,
           enc_proj_size=24, dec_hidden_size=32, dec_layers=2, dec_proj_size=24, joint_size=32)


def _table_model(V, seed):
    """lp(t, sequence so far): a fixed log-softmax row per (frame, sequence), drawn on first use.  The search's state is
    the sequence before the last token, as a row of the engine carries it."""
    rng = np.random.default_rng(seed)
    rows = {}

    def lp(t, seq):
        if (t, seq) not in rows:
            z = rng.normal(size=V) * 2.0
            rows[(t, seq)] = (z - (z.max() + math.log(np.exp(z - z.max()).sum()))).tolist()
        return rows[(t, seq)]

    def expand(t, tok, state):
        seq = state if tok < 0 else state + (tok,)
        return lp(t, seq), seq

    return lp, expand


def test_unpruned_search_sums_every_one_symbol_per_frame_path():
    V, T, W = 3, 3, 32
    lp, expand = _table_model(V, 5)
    beam, info = S.search_core(T, W, expand, (), -1, blank=0)
    brute = {}
    for path in itertools.product(range(V), repeat=T):
        seq, total = (), 0.0
        for t, k in enumerate(path):
            total += lp(t, seq)[k]
            if k != 0:
                seq = seq + (k,)
        brute.setdefault(seq, []).append(total)
    assert len(brute) == 15 and len(beam) == 15
    assert info["margin"] == float("inf")            # nothing was pruned
    assert info["merges"] == (9 - 7) + (21 - 15)     # candidates minus distinct sequences on frames 1 and 2
    got = {tuple(h["tokens"]): h for h in beam}
    assert set(got) == set(brute)
    for seq, terms in brute.items():
        m = max(terms)
        want = m + math.log(sum(math.exp(x - m) for x in terms))
        assert abs(got[seq]["logp"] - want) <= 1e-12, (seq, got[seq]["logp"], want)
        h = got[seq]
        assert len(h["frames"]) == len(h["token_logp"]) == len(seq)
        # the detail is that of the earliest creation: token u on the first frame it can stand on, frame u
        assert h["frames"] == list(range(len(seq)))
        for u, (f, l) in enumerate(zip(h["frames"], h["token_logp"])):
            assert l == lp(f, seq[:u])[seq[u]]
    logps = [h["logp"] for h in beam]
    assert logps == sorted(logps, reverse=True)
    assert abs(math.log(sum(math.exp(x) for x in logps))) <= 1e-12       # the beam holds all the mass


def test_width_one_is_the_greedy_search_without_its_blanks():
    # the blank raised by 2, not 3: the greedy path then holds blanks and tokens (2 .. 4 tokens in 6 frames)
    sd = S.sharpened(M.make_state_dict(CFG, 2), blank_bias=2.0)
    xs, _, xlen, _ = M.make_batch(CFG, 3, 4, 12, 4, ragged=False)
    want, score = M.greedy_decode(sd, xs, xlen)
    res, infos = S.search(sd, xs, xlen, W=1)
    n_tokens = 0
    for b, (r, info) in enumerate(zip(res, infos)):
        assert len(r) == 1 and info["merges"] == 0
        toks = [int(k) for k in want[b] if k != M.NUL]
        assert r[0]["tokens"] == toks, (b, r[0]["tokens"], toks)
        assert r[0]["frames"] == [t for t, k in enumerate(want[b]) if k != M.NUL]
        np.testing.assert_allclose(-r[0]["logp"], float(score[b]), rtol=1e-5, atol=1e-5)
        n_tokens += len(toks)
    assert n_tokens > 0


def test_new_symbols_are_declared_and_exported(hip_lib):
    from search_abi import assert_search_surface, make_net, make_opts
    assert_search_surface(hip_lib, {"edgedict_sync_beam_workspace_bytes", "edgedict_sync_beam_result_bytes",
                                    "edgedict_sync_beam_search"})
    f = hip_lib.edgedict_sync_beam_workspace_bytes
    assert f.restype is ctypes.c_size_t
    net = ctypes.byref(make_net())                  # fp32, J 32, V 40, E 16, L 2, H 32, P2 24
    assert f(net, 2, 9, 0, None) == 0 and f(net, 2, 9, 33, None) == 0 and f(net, 2, 0, 4, None) == 0
    assert f(None, 2, 9, 4, None) == 0
    n = f(net, 2, 9, 4, None)
    assert f(net, 2, 9, 4, ctypes.byref(make_opts())) == n
    # both state buffers of B W rows, and T W tree nodes of 16 bytes per utterance
    assert n >= 4 * (2 * 4) * 2 * 32 * 4 + 2 * (9 * 4) * 16 and n % 256 == 0
    assert f(net, 2, 9, 10, None) > n
    g = hip_lib.edgedict_sync_beam_result_bytes
    assert g.restype is ctypes.c_size_t
    assert g(0, 4, 9) == 0 and g(2, 0, 9) == 0 and g(2, 4, 9) >= 2 * 4 * 9 * 16


def test_native_argument_errors_come_before_any_launch(hip_lib):
    """W = 0 / 33, T = 0, a null pointer, a bad dtype, blank / bos or a length out of range: -1 with a message, and no
    device needed to get it."""
    buf = ctypes.create_string_buffer(256)
    fake = ctypes.cast(buf, ctypes.c_void_p)
    lens = (ctypes.c_int32 * 2)(5, 3)
    layers = (ctypes.c_void_p * 2)(fake.value, fake.value)
    from search_abi import NET_POINTERS, make_net
    names = ("net", "E1", "lens") + NET_POINTERS + ("tokens", "frames", "tlp", "ntok", "nhyp", "logp", "ws", "result")

    def run(dtype=0, T=5, W=4, blank=0, bos=2, **kw):
        a = {n: fake for n in names}
        a.update(lens=lens, w_ih=layers, w_hh=layers, b_ih=layers, b_hh=layers)
        a.update(kw)
        net = make_net(dtype=dtype, blank=blank, bos=bos, **{n: a[n] for n in NET_POINTERS})
        return hip_lib.edgedict_sync_beam_search(
            a["net"] and ctypes.byref(net), a["E1"], ctypes.c_longlong(5 * 32), ctypes.c_longlong(32), 2, T, a["lens"], W,
            a["tokens"], a["frames"], a["tlp"], 5, a["ntok"], a["nhyp"], a["logp"], None, a["ws"], a["result"], None)

    for name in names:
        assert run(**{name: None}) == -1, name
        assert b"null pointer" in hip_lib.edgedict_last_error(), name
    holes = (ctypes.c_void_p * 2)(fake.value, None)
    assert run(w_hh=holes) == -1 and b"null pointer" in hip_lib.edgedict_last_error()
    for kw, word in ((dict(W=0), b"W = 0"), (dict(W=33), b"W = 33"), (dict(T=0), b"T = 0"), (dict(T=-3), b"T = -3"),
                     (dict(dtype=7), b"dtype"), (dict(blank=40), b"blank"), (dict(bos=-1), b"blank/bos"),
                     (dict(lens=(ctypes.c_int32 * 2)(5, 6)), b"lens[1] = 6"),
                     (dict(lens=(ctypes.c_int32 * 2)(-1, 3)), b"lens[0] = -1")):
        assert run(**kw) == -1, kw
        assert word in hip_lib.edgedict_last_error(), (kw, hip_lib.edgedict_last_error())


def test_python_entry_points_refuse_bad_widths_and_cpu_tensors():
    from edgedict_amd import decode
    from edgedict_amd.models import Transducer
    m = Transducer(enc_dropout=0.0, dec_dropout=0.0, output_loss=False, **CFG).eval()
    xs = torch.zeros(2, 8, CFG["input_size"])
    enc = torch.zeros(2, 4, CFG["enc_proj_size"])
    e1 = torch.zeros(8, CFG["joint_size"])
    calls = [lambda W: m.sync_beam_search(xs, None, W), lambda W: m.sync_beam_search_nbest(xs, None, W),
             lambda W: decode.sync_beam_search(m, xs, None, W), lambda W: decode.sync_beam_search_nbest(m, xs, None, W),
             lambda W: decode.sync_beam_search_enc(m, enc, None, W),
             lambda W: decode.sync_beam_search_nbest_enc(m, enc, None, W),
             lambda W: decode.sync_beam_search_rows(m, e1, 2, 4, CFG["enc_proj_size"], None, W),
             lambda W: decode.sync_beam_search_nbest_rows(m, e1, 2, 4, CFG["enc_proj_size"], None, W)]
    for call in calls:
        for W in (0, -1, 33):
            with pytest.raises(ValueError, match="outside \\[1, 32\\]"):
                call(W)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(4)
    # the search takes none of the best-first search's options
    for kw in (dict(lm=None), dict(bias=None), dict(prefix=False), dict(max_expansions=40)):
        with pytest.raises(TypeError):
            decode.sync_beam_search(m, xs, None, 4, **kw)
