"""CPU: LM shallow fusion's host side - LMModel's parameter surface (the reference's LMModel, models.py:224-261, whose
state dict cli/train_lm.py saves), the ctypes mirror of edgedict_beam_lm_t, and every argument error raised before
anything is launched (Python ValueError; native status codes)."""
import ctypes

import numpy as np
import pytest
import torch

CFG = dict(vocab_embed_size=16, vocab_size=40, input_size=24, enc_hidden_size=32, enc_layers=2,
           enc_proj_size=24, dec_hidden_size=32, dec_layers=2, dec_proj_size=24, joint_size=32)


def _ref_keyed_sd(ntoken=40, ninp=16, nhid=32, nlayers=2):
    """What torch.save(LMModel(...).state_dict()) holds: nn.Embedding, nn.LSTM, nn.Linear under the reference's names."""
    emb = torch.nn.Embedding(ntoken, ninp)
    rnn = torch.nn.LSTM(ninp, nhid, nlayers, dropout=0.5, batch_first=True)
    dec = torch.nn.Linear(nhid, ntoken)
    sd = {"encoder.weight": emb.weight.detach()}
    sd.update({"rnn." + k: v.detach() for k, v in rnn.state_dict().items()})
    sd.update({"decoder." + k: v.detach() for k, v in dec.state_dict().items()})
    return sd


def test_reference_keyed_state_dict_loads_strictly():
    from edgedict_amd.lm import LMModel
    sd = _ref_keyed_sd()
    lm = LMModel(40, 16, 32, 2)
    lm.load_state_dict(sd, strict=True)
    assert set(lm.state_dict()) == set(sd)
    for k, v in sd.items():
        assert torch.equal(lm.state_dict()[k], v), k
    assert (lm.ntoken, lm.nhid, lm.nlayers, lm.rnn_type) == (40, 32, 2, "LSTM")


def test_init_hidden_shapes():
    from edgedict_amd.lm import LMModel
    h, c = LMModel(40, 16, 32, 3).init_hidden(5)
    assert h.shape == c.shape == (3, 5, 32)
    assert not h.any() and not c.any()


def test_tie_weights_shares_the_tensor():
    from edgedict_amd.lm import LMModel
    lm = LMModel(40, 32, 32, 1, tie_weights=True)
    assert lm.decoder.weight is lm.encoder.weight
    with pytest.raises(ValueError):
        LMModel(40, 16, 32, 1, tie_weights=True)


def test_forward_with_grad_enabled_raises():
    from edgedict_amd.lm import LMModel
    lm = LMModel(40, 16, 32, 1)
    with pytest.raises(NotImplementedError):
        lm(torch.zeros(1, 3, dtype=torch.long), lm.init_hidden(1))


def test_ctypes_mirror_has_the_header_struct_size(hip_lib):
    from edgedict_amd.lm import BeamLM
    assert ctypes.sizeof(BeamLM) == hip_lib.edgedict_beam_lm_struct_bytes()


def _model():
    from edgedict_amd.models import Transducer
    return Transducer(enc_dropout=0.0, dec_dropout=0.0, output_loss=False, **CFG).eval()


def test_python_argument_errors_come_before_any_launch():
    """CPU tensors: anything that got as far as a launch would raise RuntimeError (no CPU fallback), not ValueError."""
    from edgedict_amd import decode
    from edgedict_amd.lm import LMModel
    from edgedict_amd.stream import BatchedStreamBeamDecoder
    from edgedict_amd.flags import make_flags
    m = _model()
    lm = LMModel(40, 16, 32, 2)
    xs = torch.zeros(1, 5, CFG["input_size"])
    with pytest.raises(ValueError, match="lm_weight"):
        m.beam_search(xs, None, W=2, lm=lm)
    with pytest.raises(ValueError, match="prefix"):
        m.beam_search(xs, None, W=2, prefix=True, lm=lm, lm_weight=0.5)
    with pytest.raises(ValueError, match="vocabulary"):
        m.beam_search(xs, None, W=2, lm=LMModel(41, 16, 32, 2), lm_weight=0.5)
    with pytest.raises(ValueError, match="LMModel"):
        m.beam_search(xs, None, W=2, lm=object(), lm_weight=0.5)
    enc = torch.zeros(1, 5, CFG["enc_proj_size"])
    with pytest.raises(ValueError, match="lm_weight"):
        decode.beam_search_enc(m, enc, None, W=2, lm=lm)
    with pytest.raises(ValueError, match="vocabulary"):
        decode.beam_search_rows(m, torch.zeros(5, CFG["joint_size"]), 1, 5, CFG["enc_proj_size"], W=2,
                                lm=LMModel(39, 16, 32, 2), lm_weight=0.5)
    for kw in (dict(lm=lm), dict(lm=lm, lm_weight=0.5, prefix=True), dict(lm=LMModel(64, 16, 32, 1), lm_weight=1.0)):
        with pytest.raises(ValueError):
            decode.StreamingBeamSearch(m, 2, W=2, **kw)
        with pytest.raises(ValueError):
            BatchedStreamBeamDecoder(m, make_flags("E6D2"), 2, W=2, dither=0, **kw)


def test_native_lm_errors_are_status_codes(hip_lib):
    """edgedict_beam_search validates opts->lm before it touches the device: a vocabulary mismatch and prefix = 1 are
    ED_ERR_INVALID with a message (the device pointers below are never dereferenced)."""
    from edgedict_amd.lm import BeamLM
    from search_abi import make_net, make_opts
    fake = ctypes.c_void_p(256)
    arr = (ctypes.c_void_p * 1)(256)
    lm = BeamLM()
    lm.L, lm.E, lm.H, lm.V = 1, 16, 32, 41
    lm.emb, lm.emb_dtype = 256, 0
    lm.w_ih = lm.w_hh = lm.b_ih = lm.b_hh = ctypes.cast(arr, ctypes.c_void_p).value
    lm.Wo, lm.bo, lm.bos, lm.weight, lm.length_bonus = 256, 256, 1, 0.5, 0.0
    opts = ctypes.byref(make_opts(lm=lm))
    lens = np.array([3], dtype=np.int32)
    toks = np.zeros(64, dtype=np.int32)
    ntok = np.zeros(1, dtype=np.int32)
    score = np.zeros(1, dtype=np.float64)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def net(V, dtype=0, L=1):
        return ctypes.byref(make_net(fake, dtype=dtype, V=V, L=L, w_ih=arr, w_hh=arr, b_ih=arr, b_hh=arr))

    def call(V, prefix):
        return hip_lib.edgedict_beam_search(
            net(V), fake, ctypes.c_longlong(96), ctypes.c_longlong(32), 1, 3, vp(lens), 2, 16, prefix, vp(toks), 64,
            vp(ntok), vp(score), None, opts, fake, None)

    assert call(40, 0) == -1
    assert b"ntoken" in hip_lib.edgedict_last_error()
    assert call(41, 1) == -1
    assert b"prefix" in hip_lib.edgedict_last_error()
    nf = np.array([2], dtype=np.int32)
    commit = np.zeros(64, dtype=np.int32)
    rc = hip_lib.edgedict_beam_stream_advance(
        net(40), fake, ctypes.c_longlong(64), ctypes.c_longlong(32), 1, vp(nf), 2, 16, 64, vp(commit), vp(ntok), None,
        opts, fake, fake, None, None, None, None, None)
    assert rc == -1
    assert b"ntoken" in hip_lib.edgedict_last_error()
    # the size queries grow by the LM's state and buffers, and without an LM equal the plain ones
    empty = ctypes.byref(make_opts())
    f = hip_lib.edgedict_beam_workspace_bytes
    plain = f(net(40, 1, 2), 4, 10, 4, 32, 0, None)
    assert f(net(40, 1, 2), 4, 10, 4, 32, 0, empty) == plain > 0
    assert f(net(40, 1, 2), 4, 10, 4, 32, 0, opts) > plain
    g = hip_lib.edgedict_beam_stream_state_bytes
    st = g(None, 4, 2, 32, 4, 256)
    assert g(empty, 4, 2, 32, 4, 256) == st > 0
    assert g(opts, 4, 2, 32, 4, 256) > st
