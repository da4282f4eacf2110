"""CPU: the structs the native searches take (include/edgedict_hip.h ``edgedict_search_net_t`` /
``edgedict_search_opts_t``) against their ctypes mirrors (edgedict_amd/decode.py): sizes, the placement of every shape
field, and the refusals that come with the struct calling convention - internal-LM estimation in the expansion searches,
a partly null set of detail pointers.  Every call fails an argument check before the device is touched: the device
pointers are fake."""
import ctypes

import numpy as np

from search_abi import fake_pointer, make_net, make_opts

# pairwise distinct, so that a field read from another field's place is seen by its value
DIMS = dict(J=32, V=40, E=16, L=2, H=36, P2=24)


def test_ctypes_mirrors_have_the_header_struct_sizes(hip_lib):
    from edgedict_amd.decode import SearchNetStruct, SearchOpts
    f = hip_lib.edgedict_search_struct_bytes
    assert f.restype is ctypes.c_size_t
    assert ctypes.sizeof(SearchNetStruct) == f(0) and ctypes.sizeof(SearchOpts) == f(1) and f(2) == 0
    assert hip_lib.edgedict_beam_lm_struct_bytes() == 104          # edgedict_beam_lm_t is unchanged


def _lm(fake, V, H=32):
    from edgedict_amd.lm import BeamLM
    lm = BeamLM()
    lm.L, lm.E, lm.H, lm.V = 2, 16, H, V
    lm.emb, lm.emb_dtype, lm.Wo, lm.bo = fake.value, 0, fake.value, fake.value
    lm.w_ih = lm.w_hh = lm.b_ih = lm.b_hh = fake.value
    lm.bos, lm.weight, lm.length_bonus = 1, 0.5, 0.0
    return lm


class _Calls:
    """The two offline searches over a net of DIMS (with overrides) and fake buffers, B = 2, T = 5."""

    def __init__(self, lib):
        self.lib = lib
        self.buf, self.fake = fake_pointer()
        self.lens = (ctypes.c_int32 * 2)(5, 3)

    def net(self, **kw):
        return make_net(self.fake, **{**DIMS, **kw})

    def beam(self, net, opts=None, W=4, EM=16, nbest=False):
        f, ll = self.fake, ctypes.c_longlong
        o = None if opts is None else ctypes.byref(opts)
        if nbest:
            return self.lib.edgedict_beam_search_nbest(ctypes.byref(net), f, ll(5 * 32), ll(32), 2, 5, self.lens, W, EM, 0,
                                                       f, f, f, 81, f, f, f, None, o, f, f, f, None)
        return self.lib.edgedict_beam_search(ctypes.byref(net), f, ll(5 * 32), ll(32), 2, 5, self.lens, W, EM, 0, f, 81,
                                             f, f, None, o, f, None)

    def sync(self, net, opts=None, W=4):
        f, ll = self.fake, ctypes.c_longlong
        return self.lib.edgedict_sync_beam_search(ctypes.byref(net), f, ll(5 * 32), ll(32), 2, 5, self.lens, W, f, f, f,
                                                  5, f, f, f, None if opts is None else ctypes.byref(opts), f, f, None)

    def error(self):
        return self.lib.edgedict_last_error()


def test_every_shape_field_lands_where_the_library_reads_it(hip_lib):
    """A mis-mirrored struct shows up as a check that fires for the wrong value, or not at all.  Where the message
    prints the value it must be the one put into that field; where it prints none (``bad shape``, ``blank/bos``: the
    texts other tests match) the check must turn exactly at the field's boundary."""
    c = _Calls(hip_lib)
    lm = _lm(c.fake, V=41)
    for call, what in ((c.beam, b"beam_search"), (c.sync, b"sync_beam_search")):
        # V: an LM of another vocabulary names both
        assert call(c.net(), make_opts(lm=lm)) == -1
        assert c.error().startswith(what) and b"ntoken = 41" in c.error() and b"V = 40" in c.error(), c.error()
        # blank and bos against V: V - 1 passes this check (and is stopped by the LM's behind it), V is refused
        for field in ("blank", "bos"):
            assert call(c.net(**{field: 39}), make_opts(lm=lm)) == -1 and b"ntoken = 41" in c.error(), (field, c.error())
            assert call(c.net(**{field: 40})) == -1 and b"blank/bos outside the vocabulary" in c.error(), (field, c.error())
            assert call(c.net(**{field: -1})) == -1 and b"blank/bos outside the vocabulary" in c.error(), (field, c.error())
        # every shape field: 0 is a bad shape, the value of DIMS is not
        for field in DIMS:
            assert call(c.net(**{field: 0})) == -1 and b"bad shape" in c.error(), (field, c.error())
        # dtype and the embedding's dtype are two fields
        assert call(c.net(dtype=7)) == -1 and b"bad dtype" in c.error()
        assert call(c.net(dtype=1), make_opts(lm=lm)) == -1 and b"ntoken = 41" in c.error()
    # the frame-synchronous search alone: H must be a multiple of 4 (36 is, 38 is not - and no other field is 38)
    assert c.sync(c.net(H=38)) == -1 and b"bad shape (H must be a multiple of 4)" in c.error()
    assert c.sync(c.net(), make_opts(lm=_lm(c.fake, V=40, H=38))) == -1
    assert b"the LM's hidden width H = 38 must be a multiple of 4" in c.error()
    assert c.sync(c.net(emb_dtype=5)) == -1 and b"bad embedding dtype" in c.error()
    assert c.sync(c.net(), W=33) == -1 and b"W = 33 outside [1, 32]" in c.error()
    # L counts the layer pointers that are looked at: the third entry of an array [2] is never read
    holes = (ctypes.c_void_p * 3)(c.fake.value, c.fake.value, None)
    assert c.sync(c.net(w_hh=holes), make_opts(lm=lm)) == -1 and b"ntoken = 41" in c.error()
    assert c.sync(c.net(w_hh=holes, L=3)) == -1 and b"null pointer (layer 2)" in c.error()
    # max_expansions against W: the expansion search's own shape rule, read beside the struct
    assert c.beam(c.net(), W=4, EM=3) == -1 and b"bad shape (max_expansions must be >= W)" in c.error()


def test_null_net_and_null_net_pointers_are_refused(hip_lib):
    from search_abi import NET_POINTERS
    c = _Calls(hip_lib)
    for call in (c.beam, c.sync):
        for name in NET_POINTERS:
            assert call(c.net(**{name: None})) == -1 and b"null pointer" in c.error(), name
    f, ll = c.fake, ctypes.c_longlong
    assert hip_lib.edgedict_beam_search(None, f, ll(160), ll(32), 2, 5, c.lens, 4, 16, 0, f, 81, f, f, None, None, f,
                                        None) == -1 and b"beam_search: null pointer" in c.error()
    assert hip_lib.edgedict_sync_beam_search(None, f, ll(160), ll(32), 2, 5, c.lens, 4, f, f, f, 5, f, f, f, None, f, f,
                                             None) == -1 and b"sync_beam_search: null pointer" in c.error()


def _stream_advance(c, net, opts=None, detail=(None, None, None, None)):
    f, ll = c.fake, ctypes.c_longlong
    nf = (ctypes.c_int32 * 2)(5, 3)
    commit, ncommit = np.zeros((2, 64), dtype=np.int32), np.zeros(2, dtype=np.int32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    return c.lib.edgedict_beam_stream_advance(ctypes.byref(net), f, ll(5 * 32), ll(32), 2, nf, 4, 16, 64, vp(commit),
                                              vp(ncommit), None, None if opts is None else ctypes.byref(opts), f, f,
                                              *detail, None)


def test_expansion_searches_refuse_internal_lm_estimation(hip_lib):
    """opts->ilm_weight is the frame-synchronous search's: the expansion searches say so before anything else."""
    c = _Calls(hip_lib)
    w = ctypes.c_double(0.3)
    opts = make_opts(ilm_weight=w)
    for call, what in ((lambda: c.beam(c.net(), opts), b"beam_search:"),
                       (lambda: c.beam(c.net(), opts, nbest=True), b"beam_search_nbest:"),
                       (lambda: _stream_advance(c, c.net(), opts), b"beam_stream_advance:")):
        assert call() == -1
        assert c.error().startswith(what) and b"ilm_weight is not supported" in c.error(), c.error()
    assert hip_lib.edgedict_beam_stream_reset(ctypes.byref(opts), 2, 2, 36, 4, 64, 2, None, 0, c.fake, None, None) == -1
    assert b"beam_stream_reset: ilm_weight is not supported" in c.error()
    # with the weight gone the same calls get past it: to the LM's vocabulary check
    lm = _lm(c.fake, V=41)
    assert c.beam(c.net(), make_opts(lm=lm)) == -1 and b"ntoken = 41" in c.error()
    assert _stream_advance(c, c.net(), make_opts(lm=lm)) == -1 and b"ntoken = 41" in c.error()


def test_a_partly_null_detail_set_is_refused(hip_lib):
    """The streaming expansion search's detail - second state, second workspace, the two commit buffers - is all or
    nothing.  (The reset has one detail pointer, its state: there is no partly null set to give it.)"""
    c = _Calls(hip_lib)
    f = c.fake
    lm = _lm(f, V=41)
    for k in range(1, 15):          # every proper, non-empty subset of the four
        detail = tuple(f if k >> i & 1 else None for i in range(4))
        assert _stream_advance(c, c.net(), None, detail) == -1
        assert b"beam_stream_advance_detail: null pointer" in c.error(), (detail, c.error())
    # none, or all four, pass this check: the next one to fire is the LM's
    for detail in ((None,) * 4, (f,) * 4):
        assert _stream_advance(c, c.net(), make_opts(lm=lm), detail) == -1 and b"ntoken = 41" in c.error()
    # the reset's: a null state is refused with or without the detail's
    for dstate in (None, f):
        assert hip_lib.edgedict_beam_stream_reset(None, 2, 2, 36, 4, 64, 2, None, 0, None, dstate, None) == -1
        assert b"beam_stream_reset: null state" in c.error()


def test_calls_written_for_abi_version_1_get_a_status_not_a_fault(hip_lib):
    """A binding that still passes the network positionally puts a dtype code or a stream count where ``net`` / ``opts``
    stand now.  An address below 4096 is no object: refused (size queries: 0) before it is read."""
    c = _Calls(hip_lib)
    f, ll = c.fake, ctypes.c_longlong
    layers = (ctypes.c_void_p * 2)(f.value, f.value)
    # the size queries, with the argument lists of version 1
    assert hip_lib.edgedict_beam_workspace_bytes(1, 4, 10, 32, 40, 16, 2, 32, 24, 4, 32, 0) == 0
    assert hip_lib.edgedict_beam_stream_state_bytes(1, 4, 32, 40, 16, 2, 32, 24, 4, 32, 256) == 0
    assert hip_lib.edgedict_beam_stream_workspace_bytes(1, 4, 32, 40, 16, 2, 32, 24, 4, 32, 256) == 0
    assert hip_lib.edgedict_sync_beam_workspace_bytes(0, 2, 9, 32, 40, 16, 2, 32, 24, 4) == 0
    assert hip_lib.edgedict_sync_stream_state_bytes(3, 2, 32, 4, 64) == 0
    assert hip_lib.edgedict_sync_stream_workspace_bytes(1, 3, 32, 40, 16, 2, 32, 24, 4, 64) == 0
    # the searches and the advances: dtype = 1 (bf16) or an unknown code in net's place
    net_v1 = (32, f, ll(56), f, 24, f, f, 40, f, 0, 16, 2, layers, layers, layers, layers, 32, f, f, 0, 2)
    for dtype in (1, 7):
        for name, rc in (
                (b"beam_search", hip_lib.edgedict_beam_search(dtype, f, ll(160), ll(32), 2, 5, c.lens, *net_v1, 4, 16, 0, f,
                                                              81, f, f, None, f, None)),
                (b"sync_beam_search", hip_lib.edgedict_sync_beam_search(dtype, f, ll(160), ll(32), 2, 5, c.lens, *net_v1, 4,
                                                                        f, f, f, 5, f, f, f, f, f, None)),
                (b"sync_stream_advance", hip_lib.edgedict_sync_stream_advance(dtype, f, ll(160), ll(32), 2, 5, c.lens,
                                                                              *net_v1, 4, 64, f, f, f, 64, f, f, None))):
            assert rc == -1, (name, dtype)
    assert b"is not a pointer" in c.error()
    # the resets: the stream count in opts' place
    assert hip_lib.edgedict_sync_stream_reset(2, 2, 32, 4, 64, 2, None, 0, f, None) == -1
    assert b"sync_stream_reset: opts is not a pointer" in c.error()
    assert hip_lib.edgedict_beam_stream_reset(2, 2, 32, 4, 64, 2, None, 0, f, None) == -1
    assert b"beam_stream_reset: opts is not a pointer" in c.error()
