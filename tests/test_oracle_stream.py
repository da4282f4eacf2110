"""CPU: the streaming-loop oracle (oracle/stream_ref.py) reproduces tests/golden/stream.npz - texts
returned by the REFERENCE's own PytorchStreamDecoder.reset/decode (rnnt/stream.py:78-120), executed
by oracle/make_golden_stream.py on the reference Transducer's sub-modules - and tests/golden/stream_geometry.npz, the
same loop at the chunk geometries of make_golden_stream.GEOMETRIES (1, 3, 13, 23, 24 stacked frames per chunk)."""
import os

import numpy as np
import pytest
import torch

from oracle.make_golden_stream import (CASES, GEOMETRIES, GEOMETRY_CASES, HOP, WIN, StubVocab, case_wave, geometry_flags, ids_of,
                                       state_dict)
from oracle.stream_ref import StreamOracle

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stream.npz"))
GOLD_GEOMETRY = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stream_geometry.npz"))


@pytest.mark.parametrize("name", ["small", "small_multi", "E6D2"])
def test_stream_oracle_reproduces_reference_texts(name):
    from edgedict_amd.flags import make_flags
    cfg, wseed, xseed, S, n_chunks, resets, bias = CASES[name]
    assert list(GOLD[name + "_cfg"]) == [wseed, xseed, S, n_chunks]
    flags = make_flags("E6D2")
    sd = state_dict(cfg, wseed, bias)
    g = torch.Generator(device="cpu").manual_seed(xseed)
    wave = 0.1 * torch.randn(S, WIN + n_chunks * HOP, generator=g)
    oracles = [StreamOracle(sd, flags) for _ in range(S)]
    texts = GOLD[name + "_texts"]
    vocab = StubVocab()
    for c in range(n_chunks):
        for s in resets.get(c, []):
            oracles[s].reset()
        for s in range(S):
            ids = [t for t in oracles[s].decode(wave[s:s + 1, c * HOP:c * HOP + WIN].clone()) if t != 0]
            assert ids == ids_of(str(texts[s, c])), (c, s)
            assert "".join(vocab.id_to_token(t).replace("</w>", " ") for t in ids) == str(texts[s, c])


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_geometry_table_is_what_the_feature_oracle_and_the_engine_give(name):
    """win / hop of the table are the reference's chunk formula (stream.chunk_geometry restates it), T0 x I0 what
    oracle.features_ref stacks from one chunk, T_out what the oracle encoder returns for it."""
    from edgedict_amd.stream import chunk_geometry
    from oracle import features_ref as Fr
    geo = GEOMETRIES[name]
    f = geometry_flags(name)
    assert (f.hop_length, f.downsample, f.win_length, f.n_fft, f.feature_size) == (geo.hop_length, geo.downsample, 320, 512, 80)
    assert chunk_geometry(f, geo.step_n_frame) == (geo.win, geo.hop)
    xs = Fr.stacked_features(torch.zeros(1, geo.win), f.downsample, False, win_length=f.win_length, hop_length=f.hop_length,
                             n_fft=f.n_fft, n_filt=f.feature_size)
    assert tuple(xs.shape) == (1, geo.T0, geo.I0)
    assert geo.T_out == (geo.T0 + 1) // 2


def test_geometry_cases_cover_every_geometry_and_both_input_widths():
    assert {c.geometry for c in GEOMETRY_CASES.values()} == set(GEOMETRIES) - {"native"}
    assert set(GOLD_GEOMETRY.files) == {n + k for n in GEOMETRY_CASES for k in ("_texts", "_cfg")}
    rel = {(c.cfg["input_size"] > c.cfg["enc_hidden_size"]) for c in GEOMETRY_CASES.values()}
    assert rel == {True, False}                                     # I0 < H (narrow at H = 96) and I0 > H
    assert all(c.cfg["input_size"] == GEOMETRIES[c.geometry].I0 and c.n_chunks <= 8 for c in GEOMETRY_CASES.values())
    assert any(c.S > 1 and c.resets for c in GEOMETRY_CASES.values())


@pytest.mark.parametrize("name", list(GEOMETRY_CASES))
def test_stream_oracle_reproduces_reference_texts_at_other_chunk_geometries(name):
    case = GEOMETRY_CASES[name]
    geo = GEOMETRIES[case.geometry]
    assert list(GOLD_GEOMETRY[name + "_cfg"]) == [case.wseed, case.xseed, case.S, case.n_chunks]
    flags = geometry_flags(case.geometry)
    sd = state_dict(case.cfg, case.wseed, case.bias)
    wave = case_wave(case)
    oracles = [StreamOracle(sd, flags) for _ in range(case.S)]
    texts = GOLD_GEOMETRY[name + "_texts"]
    assert texts.shape == (case.S, case.n_chunks)
    vocab = StubVocab()
    emitted = blanks = 0
    for c in range(case.n_chunks):
        for s in case.resets.get(c, []):
            oracles[s].reset()
        for s in range(case.S):
            full = oracles[s].decode(wave[s:s + 1, c * geo.hop:c * geo.hop + geo.win].clone())
            assert len(full) == geo.T_out
            ids = [t for t in full if t != 0]
            assert ids == ids_of(str(texts[s, c])), (c, s)
            assert "".join(vocab.id_to_token(t).replace("</w>", " ") for t in ids) == str(texts[s, c])
            emitted += len(ids)
            blanks += len(full) - len(ids)
    assert emitted > 0 and blanks > 0


def test_compiled_reference_loops_match_the_reference_checkout():
    """oracle/_ref/*.bin (oracle/ref_lift.py) is what tests/test_reference_loops_gpu.py executes on the GPU box, where
    /root/reference does not exist: here, where it does, the manifest must name the current reference files (a stale
    build would test yesterday's loops) and every piece must load into code that defines the names it promises."""
    import hashlib
    import json
    import os
    import pytest
    from oracle import ref_lift
    if not os.path.isdir(ref_lift.REF):
        pytest.skip("no reference checkout here")
    if not ref_lift.available():
        ref_lift.build(verbose=False)
    man = json.load(open(os.path.join(ref_lift.OUT, "manifest.json")))
    for name, (rel, cls, names) in ref_lift.PIECES.items():
        entry = man["pieces"][name]
        digest = hashlib.sha256(open(os.path.join(ref_lift.REF, rel), "rb").read()).hexdigest()
        assert entry["sha256_of_reference_file"] == digest, name
        ns = ref_lift.load(name, {"torch": __import__("torch")})
        assert all(n in ns for n in names), name
