"""Host: the phrase automaton of edgedict_amd.bias.ContextGraph against the brute-force definition of
tests/bias_ref.py (the state is the longest suffix that is a trie path; held / pend by walking the trie), the device
table export, the argument rules and the ctypes mirror.  Nothing here needs a GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
from bias_ref import BruteBias                                       # noqa: E402

CFG = dict(vocab_embed_size=16, vocab_size=40, input_size=24, enc_hidden_size=32, enc_layers=2,
           enc_proj_size=24, dec_hidden_size=32, dec_layers=2, dec_proj_size=24, joint_size=32)
BLANK, BOS = 0, 2


def _random_set(rng, V):
    """A phrase list over a small alphabet (so that phrases overlap): random phrases plus prefixes, suffixes and inner
    parts of them, repeated tokens, single-token phrases; per-phrase boosts for every other set."""
    alphabet = [k for k in rng.choice(np.arange(3, V), size=int(rng.integers(2, 6)), replace=False)]
    n = int(rng.integers(1, 7))
    phrases = []
    for _ in range(n):
        L = int(rng.integers(1, 6))
        phrases.append([int(alphabet[i]) for i in rng.integers(0, len(alphabet), size=L)])
    base = phrases[int(rng.integers(0, n))]
    if len(base) >= 2:
        phrases.append(base[:-1])                       # a prefix
        phrases.append(base[1:])                        # a suffix
    if len(base) >= 3:
        phrases.append(base[1:-1])                      # an inner part
    phrases.append([int(alphabet[0])])                  # a single token
    phrases.append([int(alphabet[0])] * 3)              # a repeated token
    boost = float(rng.choice([0.0, 0.5, 1.25, 3.0]))
    pb = None
    if rng.integers(0, 2):
        pb = [None if rng.integers(0, 3) == 0 else float(rng.choice([0.0, 0.25, 1.0, 2.5])) for _ in phrases]
    return alphabet, phrases, boost, pb


def test_goto_delta_and_score_match_the_brute_force_definition():
    from edgedict_amd.bias import ContextGraph
    rng = np.random.default_rng(0)
    V = 24
    for it in range(300):
        alphabet, phrases, boost, pb = _random_set(rng, V)
        g = ContextGraph(phrases, boost, V, blank=BLANK, bos=BOS, phrase_boosts=pb)
        ref = BruteBias(phrases, boost, pb)
        assert g.n_states == len(ref.paths)
        # random walks over the alphabet plus strangers: the state after every prefix, every increment, the total
        for _ in range(4):
            toks = [int(rng.choice(alphabet)) if rng.integers(0, 6) else int(rng.integers(3, V))
                    for _ in range(int(rng.integers(1, 14)))]
            s, path_of = 0, {0: ()}
            for i, k in enumerate(toks):
                want_path = ref.state(toks[:i + 1])
                d = g.delta(s, k)
                assert d == ref.delta(toks[:i], k), (phrases, pb, toks, i)
                s = g.goto(s, k)
                assert g.held[s] == ref.held_pend(want_path)[0] and g.pend[s] == ref.held_pend(want_path)[1]
                assert path_of.setdefault(s, want_path) == want_path       # one state id per trie path
            assert g.score(toks) == ref.score(toks)
        for p, b in zip(ref.phrases, ref.boosts):
            assert g.score(p) >= b * len(p) - 1e-12                         # a whole phrase banks at least its own


def test_partial_match_gives_back_and_completed_phrase_keeps():
    from edgedict_amd.bias import ContextGraph
    g = ContextGraph([[5, 6, 7]], 1.5, 40)
    assert g.score([5, 6]) == 3.0
    assert g.score([5, 6, 9]) == 0.0 and g.delta(g.goto(g.goto(0, 5), 6), 9) == -3.0
    assert g.score([5, 6, 7]) == 4.5 and g.score([5, 6, 7, 9]) == 4.5
    assert g.score([5, 5, 6, 7]) == 4.5
    # no output links: [6] inside the broken partial match [5, 6, x] is not credited
    g2 = ContextGraph([[5, 6, 7], [6]], 1.0, 40)
    assert g2.score([6]) == 1.0 and g2.score([5, 6, 9]) == 0.0
    # a shared edge takes the largest boost
    g3 = ContextGraph([[5, 6], [5, 7]], 1.0, 40, phrase_boosts=[0.5, 2.0])
    assert g3.score([5]) == 2.0 and g3.score([5, 6]) == 2.5 and g3.score([5, 7]) == 4.0


def test_device_table_export_round_trips():
    """For every state and token the resolved goto is root_next plus the exceptions, rows are sorted, hold no
    default entry, and every target is a state."""
    from edgedict_amd.bias import ContextGraph
    rng = np.random.default_rng(1)
    V = 16
    for it in range(60):
        alphabet, phrases, boost, pb = _random_set(rng, V)
        g = ContextGraph(phrases, boost, V, phrase_boosts=pb)
        ref = BruteBias(phrases, boost, pb)
        assert g.root_next.shape == (V,) and g.row_ptr.shape == (g.n_states + 1,)
        assert g.row_ptr[0] == 0 and g.row_ptr[-1] == g.exc_tok.size == g.exc_next.size
        assert g.row_ptr[1] == 0                                         # the root's row is empty
        assert ((g.exc_next >= 0) & (g.exc_next < g.n_states)).all() and ((g.root_next >= 0) &
                                                                          (g.root_next < g.n_states)).all()
        # the trie path of every state id, breadth first from the root through the exported tables only
        path = {0: ()}
        frontier = [0]
        while frontier:
            nxt = []
            for s in frontier:
                lo, hi = g.row_ptr[s], g.row_ptr[s + 1]
                row = dict(zip(g.exc_tok[lo:hi].tolist(), g.exc_next[lo:hi].tolist()))
                assert list(row) == sorted(row) and len(row) == hi - lo
                for k in range(V):
                    n = row.get(k, int(g.root_next[k]))
                    assert k not in row or row[k] != g.root_next[k]
                    assert n == g.goto(s, k)
                    want = ref.state(path[s] + (k,))
                    if n in path:
                        assert path[n] == want
                    else:
                        path[n] = want
                        nxt.append(n)
            frontier = nxt
        assert len(path) == g.n_states


def test_a_large_list_has_short_rows():
    from edgedict_amd.bias import ContextGraph
    rng = np.random.default_rng(2)
    phrases = [[int(k) for k in rng.integers(4, 4000, size=int(rng.integers(2, 5)))] for _ in range(1000)]
    g = ContextGraph(phrases, 1.0, 4096)
    assert g.n_states > 2000
    assert np.diff(g.row_ptr).max() <= 8 and g.exc_tok.size < 2 * g.n_states


def test_argument_errors():
    from edgedict_amd.bias import ContextGraph
    for bad, match in (([[]], "empty"), ([[5, 40]], "outside"), ([[-1]], "outside"), ([[5, BLANK]], "blank"),
                       ([[BOS, 5]], "BOS")):
        with pytest.raises(ValueError, match=match):
            ContextGraph(bad, 1.0, 40, blank=BLANK, bos=BOS)
    with pytest.raises(ValueError, match="boost"):
        ContextGraph([[5]], -0.5, 40)
    with pytest.raises(ValueError, match="boost"):
        ContextGraph([[5], [6]], 1.0, 40, phrase_boosts=[1.0, -2.0])
    with pytest.raises(ValueError, match="phrase_boosts"):
        ContextGraph([[5], [6]], 1.0, 40, phrase_boosts=[1.0])
    g = ContextGraph([], 1.0, 40)
    assert g.empty and g.n_states == 1 and g.score([5, 6]) == 0.0


def test_from_text_uses_the_tokenizer_object():
    from edgedict_amd.bias import ContextGraph

    class Enc:
        def __init__(self, ids):
            self.ids = ids

    class Inner:
        def encode(self, text):
            return Enc([4 + ord(c) - ord("a") for c in text])

    class Tok:
        tokenizer = Inner()
        vocab_size = 40

    g = ContextGraph.from_text(["ab", "abc"], Tok(), 2.0)
    assert g.V == 40 and g.phrases == [[4, 5], [4, 5, 6]]
    assert g.score([4, 5, 6]) == 6.0
    h = ContextGraph.from_text(["ba"], Inner(), 1.0, vocab_size=40)
    assert h.phrases == [[5, 4]]


def _model():
    from edgedict_amd.models import Transducer
    return Transducer(enc_dropout=0.0, dec_dropout=0.0, output_loss=False, **CFG).eval()


def test_python_argument_errors_come_before_any_launch():
    """CPU tensors: anything that got as far as a launch would raise RuntimeError (no CPU fallback), not ValueError."""
    from edgedict_amd import decode
    from edgedict_amd.bias import ContextGraph
    from edgedict_amd.flags import make_flags
    from edgedict_amd.stream import BatchedStreamBeamDecoder
    m = _model()
    g = ContextGraph([[5, 6]], 1.0, 40)
    other = ContextGraph([[5, 6]], 1.0, 41)
    xs = torch.zeros(1, 5, CFG["input_size"])
    enc = torch.zeros(1, 5, CFG["enc_proj_size"])
    rows = torch.zeros(5, CFG["joint_size"])
    with pytest.raises(ValueError, match="prefix"):
        m.beam_search(xs, None, W=2, prefix=True, bias=g)
    with pytest.raises(ValueError, match="vocabulary"):
        m.beam_search(xs, None, W=2, bias=other)
    with pytest.raises(ValueError, match="ContextGraph"):
        m.beam_search(xs, None, W=2, bias=[[5, 6]])
    with pytest.raises(ValueError, match="vocabulary"):
        m.beam_search_nbest(xs, None, W=2, bias=other)
    with pytest.raises(ValueError, match="prefix"):
        decode.beam_search_enc(m, enc, None, W=2, prefix=True, bias=g)
    with pytest.raises(ValueError, match="vocabulary"):
        decode.beam_search_rows(m, rows, 1, 5, CFG["enc_proj_size"], W=2, bias=other)
    with pytest.raises(ValueError, match="vocabulary"):
        decode.beam_search_nbest_enc(m, enc, None, W=2, bias=other)
    with pytest.raises(ValueError, match="prefix"):
        decode.beam_search_nbest_rows(m, rows, 1, 5, CFG["enc_proj_size"], W=2, prefix=True, bias=g)
    for kw in (dict(bias=other), dict(bias=g, prefix=True), dict(bias=object())):
        with pytest.raises(ValueError):
            decode.StreamingBeamSearch(m, 2, W=2, **kw)
        with pytest.raises(ValueError):
            BatchedStreamBeamDecoder(m, make_flags("E6D2"), 2, W=2, dither=0, **kw)


def test_ctypes_mirrors_have_the_header_struct_sizes(hip_lib):
    from edgedict_amd.bias import BeamBias
    from edgedict_amd.lm import BeamLM
    assert ctypes.sizeof(BeamBias) == hip_lib.edgedict_beam_bias_struct_bytes()
    assert ctypes.sizeof(BeamLM) == hip_lib.edgedict_beam_lm_struct_bytes() == 104       # edgedict_beam_lm_t is unchanged


def test_native_bias_errors_are_status_codes_and_sizes_grow(hip_lib):
    """edgedict_beam_search validates opts->bias before it touches the device (the device pointers below are never
    dereferenced); without a list the size queries equal the plain ones."""
    from edgedict_amd.bias import BeamBias
    from search_abi import make_net, make_opts
    fake = ctypes.c_void_p(256)
    arr = (ctypes.c_void_p * 1)(256)
    bias = BeamBias()
    bias.S, bias.V, bias.n_exc = 3, 41, 0
    bias.root_next = bias.held = bias.pend = bias.row_ptr = bias.exc_tok = bias.exc_next = 256
    opts = ctypes.byref(make_opts(bias=bias))
    lens = np.array([3], dtype=np.int32)
    toks = np.zeros(64, dtype=np.int32)
    ntok = np.zeros(1, dtype=np.int32)
    score = np.zeros(1, dtype=np.float64)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def call(V, prefix):
        net = make_net(fake, V=V, L=1, w_ih=arr, w_hh=arr, b_ih=arr, b_hh=arr)
        return hip_lib.edgedict_beam_search(
            ctypes.byref(net), fake, ctypes.c_longlong(96), ctypes.c_longlong(32), 1, 3, vp(lens), 2, 16, prefix,
            vp(toks), 64, vp(ntok), vp(score), None, opts, fake, None)

    assert call(40, 0) == -1
    assert b"vocabulary" in hip_lib.edgedict_last_error()
    assert call(41, 1) == -1
    assert b"prefix" in hip_lib.edgedict_last_error()
    bias.held = 0
    assert call(41, 0) == -1
    assert b"null bias" in hip_lib.edgedict_last_error()
    net, empty = ctypes.byref(make_net(dtype=1)), ctypes.byref(make_opts())
    plain = hip_lib.edgedict_beam_workspace_bytes(net, 4, 10, 4, 32, 0, None)
    assert hip_lib.edgedict_beam_workspace_bytes(net, 4, 10, 4, 32, 0, empty) == plain > 0
    assert hip_lib.edgedict_beam_workspace_bytes(net, 4, 10, 4, 32, 0, opts) > plain
    st = hip_lib.edgedict_beam_stream_state_bytes(None, 4, 2, 32, 4, 256)
    ws = hip_lib.edgedict_beam_stream_workspace_bytes(net, 4, 4, 32, 256, None)
    assert hip_lib.edgedict_beam_stream_state_bytes(empty, 4, 2, 32, 4, 256) == st > 0
    assert hip_lib.edgedict_beam_stream_state_bytes(opts, 4, 2, 32, 4, 256) > st
    assert hip_lib.edgedict_beam_stream_workspace_bytes(net, 4, 4, 32, 256, empty) == ws > 0
    assert hip_lib.edgedict_beam_stream_workspace_bytes(net, 4, 4, 32, 256, opts) > ws
