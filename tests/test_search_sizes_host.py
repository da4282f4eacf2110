"""CPU: every size query of the search layer (csrc/decode.hip) returns the bytes recorded from the build of commit
efb6be6, the last one before the host code was restructured around shared structs: workspace and state layouts are part
of what callers allocate, so a refactor of the layout code must not move them.  Exact equality, no GPU.

``python tests/test_search_sizes_host.py > tests/golden/search_sizes.json`` rewrites the record from whatever library is
built - only do that on purpose, for a change that is meant to move a layout."""
import ctypes
import itertools
import json
import os
import sys

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "search_sizes.json")

# J, V, E, L, H, P2 of the transducer; (L, E, H) of the fusion LM; B/S, T, W, max_expansions, node_capacity
SHAPES = {
    "tiny": dict(net=(32, 40, 16, 2, 32, 24), lm=(2, 16, 32), B=3, T=7, W=2, EM=16, NC=64),
    "E6D2": dict(net=(640, 1024, 64, 2, 256, 256), lm=(2, 64, 1024), B=64, T=40, W=10, EM=80, NC=3584),
}


def _lm(V, shape):
    from edgedict_amd.lm import BeamLM
    lm = BeamLM()
    lm.L, lm.E, lm.H = shape
    lm.V = V
    return lm


def _rows(lib):
    """[(key, bytes)] over both dtypes x both shapes x (prefix 0/1 where it applies) x (without / with an LM)."""
    from search_abi import make_net, make_opts
    out = []
    for dt, (name, sh) in itertools.product((0, 1), SHAPES.items()):
        J, V, E, L, H, P2 = sh["net"]
        B, T, W, EM, NC = sh["B"], sh["T"], sh["W"], sh["EM"], sh["NC"]
        out.append(("greedy_workspace dtype=%d %s" % (dt, name),
                    lib.edgedict_greedy_workspace_bytes(dt, B, J, V, E, L, H, P2)))
        net = ctypes.byref(make_net(dtype=dt, J=J, V=V, E=E, L=L, H=H, P2=P2))
        for with_lm in (0, 1):         # (the keys keep the names the record was made under: _lm = with an LM in opts)
            lm = _lm(V, sh["lm"])
            opts = ctypes.byref(make_opts(lm=lm)) if with_lm else None
            sfx = "_lm" if with_lm else ""
            for prefix in (0, 1):
                out.append(("beam_workspace%s dtype=%d %s prefix=%d" % (sfx, dt, name, prefix),
                            lib.edgedict_beam_workspace_bytes(net, B, T, W, EM, prefix, opts)))
            out.append(("beam_stream_state%s dtype=%d %s" % (sfx, dt, name),
                        lib.edgedict_beam_stream_state_bytes(opts, B, L, H, W, NC)))
            out.append(("beam_stream_workspace%s dtype=%d %s" % (sfx, dt, name),
                        lib.edgedict_beam_stream_workspace_bytes(net, B, W, EM, NC, opts)))
    return out


def test_size_queries_return_the_recorded_bytes(hip_lib):
    with open(GOLDEN) as f:
        golden = json.load(f)
    rows = _rows(hip_lib)
    assert [k for k, _ in rows] == list(golden["bytes"])
    for key, got in rows:
        assert got == golden["bytes"][key] and got > 0, (key, got, golden["bytes"][key])


def test_lm_forms_without_an_lm_equal_the_plain_queries(hip_lib):
    """opts with three null members is the null opts; ILME, which these searches do not have, sizes nothing."""
    from search_abi import make_net, make_opts
    empty, ilm = ctypes.byref(make_opts()), ctypes.c_double(0.5)
    for dt, sh in itertools.product((0, 1), SHAPES.values()):
        J, V, E, L, H, P2 = sh["net"]
        B, T, W, EM, NC = sh["B"], sh["T"], sh["W"], sh["EM"], sh["NC"]
        net = ctypes.byref(make_net(dtype=dt, J=J, V=V, E=E, L=L, H=H, P2=P2))
        for prefix in (0, 1):
            a = (net, B, T, W, EM, prefix)
            assert hip_lib.edgedict_beam_workspace_bytes(*a, empty) == hip_lib.edgedict_beam_workspace_bytes(*a, None) > 0
        f, g = hip_lib.edgedict_beam_stream_state_bytes, hip_lib.edgedict_beam_stream_workspace_bytes
        assert f(empty, B, L, H, W, NC) == f(None, B, L, H, W, NC) > 0
        assert g(net, B, W, EM, NC, empty) == g(net, B, W, EM, NC, None) > 0
        with_ilm = ctypes.byref(make_opts(ilm_weight=ilm))
        assert hip_lib.edgedict_beam_workspace_bytes(net, B, T, W, EM, 0, with_ilm) == 0
        assert f(with_ilm, B, L, H, W, NC) == 0 and g(net, B, W, EM, NC, with_ilm) == 0
        assert hip_lib.edgedict_beam_workspace_bytes(None, B, T, W, EM, 0, None) == 0 and g(None, B, W, EM, NC, None) == 0


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from edgedict_amd import _lib
    json.dump({"recorded_from": "the library built from commit efb6be6 (parent of the shared-structs refactor of "
                                "csrc/decode.hip), by tests/test_search_sizes_host.py run as a script",
               "bytes": dict(_rows(_lib.load()))}, sys.stdout, indent=1)
    sys.stdout.write("\n")
