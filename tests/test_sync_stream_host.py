"""CPU: the streaming frame-synchronous beam search's oracle (tests/sync_stream_ref.py) against the offline oracle
(tests/sync_beam_ref.search_core) over every split of the frames into chunks, its commit rule, and the argument rules of
the native and Python entry points (csrc/decode_sync.hip ``edgedict_sync_stream_*``, decode.StreamingSyncBeamSearch,
stream.BatchedStreamSyncBeamDecoder): everything that needs no device."""
import ctypes
import itertools

import pytest

import sync_beam_ref as S
import sync_stream_ref as R
from edgedict_amd.decode import StreamingSyncBeamSearch
from edgedict_amd.stream import BatchedStreamSyncBeamDecoder
from test_sync_beam_host import CFG, _table_model


def _splits(T):
    """Every composition of T: all ways to cut T frames into chunks."""
    for cuts in itertools.product((0, 1), repeat=T - 1):
        out, n = [], 1
        for c in cuts:
            if c:
                out.append(n)
                n = 0
            n += 1
        yield out + [n]


def _prefix_of(log, hyp):
    n = len(log)
    return (hyp["tokens"][:n] == [k for k, _, _ in log] and hyp["frames"][:n] == [f for _, f, _ in log]
            and hyp["token_logp"][:n] == [lp for _, _, lp in log])


# (W, seed, T).  (2, 5, 7): a non-empty commit, one merge, and - measured on the oracle, asserted below - a commit that is
# strictly shorter than the beam's common token prefix
CASES = [(2, 5, 7), (2, 4, 6), (4, 5, 6), (4, 11, 5), (32, 5, 3), (32, 7, 4)]


@pytest.mark.parametrize("W,seed,T", CASES)
def test_chunked_oracle_equals_the_offline_oracle_for_every_split(W, seed, T):
    V = 3
    offline = {}
    for n in range(1, T + 1):
        _, expand = _table_model(V, seed)
        offline[n] = S.search_core(n, W, expand, (), -1, blank=0)[0]
    n_splits = 0
    for split in _splits(T):
        _, expand = _table_model(V, seed)           # the table draws rows on first use: same seed, same order of use
        st = R.StreamSearch(W, expand, (), -1, blank=0)
        logs, done = [], 0
        for n in split:
            before = list(st.log)
            new = st.advance(n)
            done += n
            assert st.log[:len(before)] == before and st.log[len(before):] == new      # the log only grows
            beam = st.beam()
            assert beam == offline[done], (split, done)
            logs.append(list(st.log))
            for log in logs:                        # every boundary's log is a prefix of every later hypothesis
                assert all(_prefix_of(log, h) for h in beam), (split, done, log)
            assert len(st.log) <= R.common_token_prefix(beam)
            assert st.live_nodes() <= W * done
        n_splits += 1
    assert n_splits == 2 ** (T - 1)


def test_the_table_draws_do_not_depend_on_the_chunking():
    """The comparison above needs lp(t, seq) to be the same function for every split: the table model draws a row on
    first use, and both searches ask for (frame, sequence) pairs in the same order."""
    _, e1 = _table_model(3, 5)
    _, e2 = _table_model(3, 5)
    a = S.search_core(6, 4, e1, (), -1, blank=0)[0]
    st = R.StreamSearch(4, e2, (), -1, blank=0)
    for n in (1, 2, 3):
        st.advance(n)
    assert st.beam() == a


def test_commits_happen_and_can_lag_the_common_token_prefix():
    """W = 2, seed 5, one-frame chunks: tokens are committed, and at some boundary the beam agrees on more tokens than
    are committed, because the agreed token stands in two nodes - a sequence that was pruned and created again has a
    second chain.  The commit is the TREE's common ancestor."""
    W, seed, T = CASES[0]
    _, expand = _table_model(3, seed)
    st = R.StreamSearch(W, expand, (), -1, blank=0)
    committed_any = lagged = False
    for _ in range(T):
        st.advance(1)
        beam = st.beam()
        n_tok, n_log = R.common_token_prefix(beam), len(st.log)
        committed_any |= n_log > 0
        if n_log < n_tok:
            lagged = True
            # the first uncommitted token is the same in every hypothesis, but not the same node
            firsts = {st._path(h.node)[0] for h in st.rows}
            assert len(firsts) > 1
            assert len({st.tree[nd][1] for nd in firsts}) == 1
    assert committed_any and lagged
    assert st.merges >= 1


# ------------------------------------------------------------------------------------------- the native entry points
NAMES = {"edgedict_sync_stream_state_bytes", "edgedict_sync_stream_workspace_bytes", "edgedict_sync_stream_result_bytes",
         "edgedict_sync_stream_reset", "edgedict_sync_stream_advance", "edgedict_sync_stream_read"}


def test_new_symbols_are_declared_and_exported(hip_lib):
    from search_abi import assert_search_surface, make_net, make_opts
    assert_search_surface(hip_lib, NAMES)
    assert hip_lib.edgedict_abi_version() == 2
    empty = ctypes.byref(make_opts())
    f = hip_lib.edgedict_sync_stream_state_bytes             # opts, S, L, H, W, NC
    assert f.restype is ctypes.c_size_t
    n = f(None, 3, 2, 32, 4, 64)
    assert f(empty, 3, 2, 32, 4, 64) == n
    # both state buffers of S W rows (h and c), and NC nodes of 16 bytes per stream
    assert n >= 4 * (3 * 4) * 2 * 32 * 4 + 3 * 64 * 16 and n % 256 == 0
    assert f(None, 3, 2, 32, 10, 64) > n and f(None, 5, 2, 32, 4, 64) > n and f(None, 3, 2, 32, 4, 640) > n
    for bad in ((0, 2, 32, 4, 64), (3, 2, 32, 0, 64), (3, 2, 32, 33, 64), (3, 2, 30, 4, 64), (3, 2, 32, 4, 3),
                (3, 0, 32, 4, 64)):
        assert f(None, *bad) == 0, bad
    g = hip_lib.edgedict_sync_stream_workspace_bytes         # net, S, W, NC, opts
    assert g.restype is ctypes.c_size_t
    net = ctypes.byref(make_net())                           # fp32, J 32, V 40, E 16, L 2, H 32, P2 24
    m = g(net, 3, 4, 64, None)
    assert m > 0 and m % 256 == 0 and g(net, 3, 4, 64, empty) == m
    assert g(net, 3, 10, 64, None) > m and g(net, 3, 4, 640, None) > m and g(net, 5, 4, 64, None) > m
    assert g(net, 3, 0, 64, None) == 0 and g(net, 3, 33, 64, None) == 0 and g(net, 3, 4, 3, None) == 0
    assert g(ctypes.byref(make_net(dtype=7)), 3, 4, 64, None) == 0
    assert g(net, 0, 4, 64, None) == 0 and g(None, 3, 4, 64, None) == 0
    r = hip_lib.edgedict_sync_stream_result_bytes
    assert r.restype is ctypes.c_size_t
    assert r(0, 4, 9) == 0 and r(2, 0, 9) == 0 and r(2, 33, 9) == 0 and r(2, 4, -1) == 0
    assert r(2, 4, 9) >= 2 * 4 * 9 * 16 and r(3, 4, 9) > r(2, 4, 9) and r(2, 10, 9) > r(2, 4, 9)


def _fake():
    buf = ctypes.create_string_buffer(4096)
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def test_native_advance_argument_errors_come_before_any_launch(hip_lib):
    buf, fake = _fake()
    layers = (ctypes.c_void_p * 2)(fake.value, fake.value)
    from search_abi import NET_POINTERS, make_net
    names = ("net", "E1", "nf") + NET_POINTERS + ("live", "parity", "commit", "state", "ws")

    def run(dtype=0, S=2, T=5, W=4, NC=64, H=32, blank=0, bos=2, emb_dtype=0, live_v=(0, 0), nf_v=(5, 3), parity_v=0,
            max_commit=64, **kw):
        a = {n: fake for n in names}
        a.update(nf=(ctypes.c_int32 * 2)(*nf_v), live=(ctypes.c_int32 * 2)(*live_v),
                 parity=ctypes.pointer(ctypes.c_int32(parity_v)),
                 w_ih=layers, w_hh=layers, b_ih=layers, b_hh=layers)
        a.update(kw)
        net = make_net(dtype=dtype, H=H, blank=blank, bos=bos, emb_dtype=emb_dtype, **{n: a[n] for n in NET_POINTERS})
        return hip_lib.edgedict_sync_stream_advance(
            a["net"] and ctypes.byref(net), a["E1"], ctypes.c_longlong(5 * 32), ctypes.c_longlong(32), S, T, a["nf"], W,
            NC, a["live"], a["parity"], a["commit"], max_commit, None, a["state"], a["ws"], None)

    for name in names:
        assert run(**{name: None}) == -1, name
        assert b"null pointer" in hip_lib.edgedict_last_error(), name
    holes = (ctypes.c_void_p * 2)(fake.value, None)
    for which in ("w_ih", "w_hh", "b_ih", "b_hh"):
        assert run(**{which: holes}) == -1 and b"null pointer (layer 1)" in hip_lib.edgedict_last_error()
    for kw, word in ((dict(W=0), b"W = 0"), (dict(W=33), b"W = 33"), (dict(S=0), b"S = 0"), (dict(S=-2), b"S = -2"),
                     (dict(NC=3), b"node_capacity = 3 is too small"), (dict(dtype=7), b"bad dtype"),
                     (dict(emb_dtype=5), b"embedding dtype"), (dict(blank=40), b"blank"), (dict(bos=-1), b"blank/bos"),
                     (dict(nf_v=(5, 6)), b"n_frames[1] = 6"), (dict(nf_v=(-1, 3)), b"n_frames[0] = -1"),
                     (dict(H=30), b"multiple of 4"), (dict(parity_v=2), b"parity"),
                     (dict(live_v=(0, 60)), b"node_capacity is 64"), (dict(live_v=(0, 53)), b"stream 1 may need 65"),
                     (dict(max_commit=4), b"max_commit = 4")):
        assert run(**kw) == -1, kw
        assert word in hip_lib.edgedict_last_error(), (kw, hip_lib.edgedict_last_error())


def test_native_reset_and_read_argument_errors_come_before_any_launch(hip_lib):
    buf, fake = _fake()

    def reset(S=2, L=2, H=32, W=4, NC=64, bos=2, state=fake):
        return hip_lib.edgedict_sync_stream_reset(None, S, L, H, W, NC, bos, None, 0, state, None)

    names = ("state", "result", "tokens", "ntok", "nhyp", "logp")        # (frames and token_logp are nullable)

    def read(S=2, L=2, H=32, W=4, NC=64, MT=8, **kw):
        a = {n: fake for n in names + ("frames", "tlp")}
        a.update(kw)
        return hip_lib.edgedict_sync_stream_read(S, L, H, W, NC, a["state"], a["result"], a["tokens"], a["frames"],
                                                 a["tlp"], MT, a["ntok"], a["nhyp"], a["logp"], None, None, None)

    for call, what in ((reset, b"sync_stream_reset"), (read, b"sync_stream_read")):
        for kw, word in ((dict(W=0), b"W = 0"), (dict(W=33), b"W = 33"), (dict(S=0), b"S = 0"),
                         (dict(NC=3), b"node_capacity = 3 is too small"), (dict(H=30), b"multiple of 4"),
                         (dict(state=None), b"null pointer")):
            assert call(**kw) == -1, (what, kw)
            msg = hip_lib.edgedict_last_error()
            assert word in msg and msg.startswith(what), (what, kw, msg)
    assert reset(bos=-1) == -1 and b"bos" in hip_lib.edgedict_last_error()
    assert read(MT=-1) == -1 and b"max_tokens" in hip_lib.edgedict_last_error()
    for name in names:
        assert read(**{name: None}) == -1 and b"null pointer" in hip_lib.edgedict_last_error(), name


# ------------------------------------------------------------------------------------------- the Python entry points
def test_python_entry_points_refuse_bad_widths_cpu_models_and_foreign_keywords():
    from edgedict_amd.flags import make_flags
    from edgedict_amd.models import Transducer
    m = Transducer(enc_dropout=0.0, dec_dropout=0.0, output_loss=False, **CFG).eval()
    flags = make_flags("E6D2")
    calls = [lambda **kw: StreamingSyncBeamSearch(m, 2, **kw),
             lambda **kw: BatchedStreamSyncBeamDecoder(m, flags, 2, dither=0, **kw)]
    for call in calls:
        for W in (0, -1, 33):
            with pytest.raises(ValueError, match="outside \\[1, 32\\]"):
                call(W=W)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(W=4)
        for kw in (dict(lm=None), dict(bias=None), dict(prefix=False), dict(max_expansions=40)):
            with pytest.raises(TypeError):
                call(W=4, **kw)
    with pytest.raises(ValueError, match="n_streams"):
        StreamingSyncBeamSearch(m, 0, W=4)
    with pytest.raises(ValueError, match="node_capacity"):
        StreamingSyncBeamSearch(m, 2, W=4, node_capacity=3)
