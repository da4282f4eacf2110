"""ctypes helpers of the host tests that call the native searches directly (include/edgedict_hip.h): an
``edgedict_search_net_t`` of given shapes over fake pointers, and an ``edgedict_search_opts_t``."""
import ctypes

from edgedict_amd.decode import SearchNetStruct, SearchOpts

NET_POINTERS = ("W1d", "b1", "W2", "b2", "emb", "w_ih", "w_hh", "b_ih", "b_hh", "Wp", "bp")


def fake_pointer(nbytes=256):
    """(buffer, void*) - host memory standing in for device pointers that no argument check dereferences.  Its first
    words are non-zero, so that it also serves as a HOST array [L] of layer pointers."""
    buf = ctypes.create_string_buffer(b"\x01" * nbytes, nbytes)
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def make_net(fake=None, dtype=0, J=32, V=40, E=16, L=2, H=32, P2=24, blank=0, bos=2, emb_dtype=0, ldw1=56, **pointers):
    """An ``edgedict_search_net_t`` of these shapes whose pointers are all ``fake`` (None: null), except those given by
    name.  The size queries read the shapes alone."""
    n = SearchNetStruct(dtype=dtype, J=J, ldw1=ldw1, P2=P2, V=V, emb_dtype=emb_dtype, E=E, L=L, H=H, blank=blank, bos=bos)
    for name in NET_POINTERS:
        p = pointers.get(name, fake)
        setattr(n, name, p if p is None or isinstance(p, (int, ctypes.c_void_p)) else ctypes.cast(p, ctypes.c_void_p))
    return n


def make_opts(lm=None, bias=None, ilm_weight=None):
    """An ``edgedict_search_opts_t`` naming these ctypes objects (a BeamLM, a BeamBias, a c_double); all None gives the
    struct with three null members, NOT a null pointer.  Keep the arguments alive while it is in use."""
    addr = lambda x: None if x is None else ctypes.addressof(x)
    return SearchOpts(lm=addr(lm), bias=addr(bias), ilm_weight=addr(ilm_weight))


# the searches' whole native surface: one exported function per operation, features are opts members
SEARCH_ENTRY_POINTS = {
    "edgedict_search_struct_bytes",
    "edgedict_beam_workspace_bytes", "edgedict_beam_detail_bytes", "edgedict_beam_nbest_result_bytes",
    "edgedict_beam_search", "edgedict_beam_search_nbest",
    "edgedict_beam_stream_state_bytes", "edgedict_beam_stream_workspace_bytes",
    "edgedict_beam_stream_detail_state_bytes", "edgedict_beam_stream_detail_workspace_bytes",
    "edgedict_beam_stream_reset", "edgedict_beam_stream_advance", "edgedict_beam_stream_read",
    "edgedict_beam_stream_read_nbest",
    "edgedict_sync_beam_workspace_bytes", "edgedict_sync_beam_result_bytes", "edgedict_sync_beam_search",
    "edgedict_sync_stream_state_bytes", "edgedict_sync_stream_workspace_bytes", "edgedict_sync_stream_result_bytes",
    "edgedict_sync_stream_reset", "edgedict_sync_stream_advance", "edgedict_sync_stream_read",
}
DELETED_SUFFIXES = ("_lm", "_bias", "_nbest_bias", "_detail", "_detail_bias", "_fusion", "_ilme")


def assert_search_surface(lib, names):
    """``names`` (of SEARCH_ENTRY_POINTS) are declared and exported, and no search entry point carries a feature suffix."""
    from edgedict_amd import _lib
    declared = set(_lib.declared_symbols())
    assert names <= SEARCH_ENTRY_POINTS and names <= declared
    for name in names:
        assert hasattr(lib, name), name
    searches = {n for n in declared if n.startswith(("edgedict_beam_", "edgedict_sync_"))}
    assert searches | {"edgedict_search_struct_bytes"} == SEARCH_ENTRY_POINTS | {"edgedict_beam_lm_struct_bytes",
                                                                                "edgedict_beam_bias_struct_bytes"}
    assert not [n for n in searches if n.endswith(DELETED_SUFFIXES)]
