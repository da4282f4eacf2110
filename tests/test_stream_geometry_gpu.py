"""GPU: the streaming decoders at chunk geometries beyond the native 75 ms chunk (oracle.make_golden_stream.GEOMETRIES).

Every other streaming test runs one chunk: 1320 / 1200 samples, T0 = 2 stacked frames of I0 = 240 features.  Chunk
geometry selects the code a chunk step runs - stream._ChunkPlan (the pre-bound fast path) only for 0 < T0 < 24 and
S <= 4096 (T0 <= 2) or S <= 16 (T0 > 2); Encoder.forward then one of the fused edgedict_stream_encoder_step, the
per-layer LSTM kernels, and from T0 >= 24 in bf16 the layer-pipelined stack with carried (h, c) - and an odd T0 is
zero-padded by the time reduction inside EVERY chunk, which offline decoding does not do.  The geometries:

    name          hop  ds  steps   win / hop     T0 x I0    frames out
    native        200   3    2    1320 / 1200    2 x 240        1
    hop640        160   2    2     800 /  640    3 x 160        2       bench.py's stream_256_hop640(_fp32)
    one_frame     200   3    1     720 /  600    1 x 240        1
    narrow        200   1    2     520 /  400    3 x  80        2       H = 96: I0 < H
    wide          200   4    2    1720 / 1600    2 x 320        1
    long          160   2   12    4000 / 3840   13 x 160        7
    stack_below   160   2   22    7200 / 7040   23 x 160       12
    stack_at      160   2   23    7520 / 7360   24 x 160       12       config.STACK_MIN_FRAMES

fp32 (the parity mode) is token-exact: against the texts the REFERENCE's own decoder loop returned
(tests/golden/stream_geometry.npz, oracle/make_golden_stream.py) and, blanks included, against oracle.stream_ref.

bf16 has no free-running token reference (a near-tie flips a token and the histories part; the picks are judged by the
token-forced replay of tests/test_search_kernels_gpu.py).  Here: the ROUTE is asserted (the plan's ``ok``, calls of
encoder_stack.EncoderStackFn.apply and of models._stream_encoder_step counted around the run); where the plan applies it
is bit-identical to the module path in tokens and every carried state; a stream that repeats another stream's audio and
resets is bit-identical to it; the chunk's stacked features are the float64 front-end's (tests/fbank_ref.py, its bound)
and the plan's bf16 features their rounding; the encoder's rows and carried (h, c) are the bf16-rounded float64 replay's
(tests/stream_enc_ref.py) fed the device's own features and previous state, chunk after chunk, at BF16_TOL = 2e-2 of the
buffer's max (tests/test_stream_encoder_gpu.py; tests/test_stream_enc_chunks_host.py shows on the CPU that the bound is
neither used up by the replay nor slack at these shapes); the per-layer route against the fused one at that test's
bounds.  Routes without an indicator of their own: the per-layer kernels are Encoder.forward's ``else`` branch - taken
exactly when neither counted entry was (T0 < 24 with S beyond the row limit); encoder_stack.last_mode(False) is the stack's
own indicator but keeps the value of the last stack pass of the PROCESS, so the call count decides and last_mode is
asserted to be a stack kind after a stack run and unchanged by a run that must not enter the stack.

Both benched hop640 configurations run at S = 256: a mid-size body (H = 128) in fp32 and bf16, the E6D2 body in fp32.

Measured on an MI355X (printed with -s), 60 tests in 4.3 s, error / max(|ref|, 1e-3) against its bound:
  features, every geometry      linear frame-relative 1.4e-7 .. 2.9e-7 (bound 6.8e-6), log 4.8e-7 (bound 2e-6); the plan's
                                bf16 buffer is the rounding of the fp32 output bit for bit at every geometry
  fused step vs rounded replay  T0 = 1, 2, 3, 23 (native, hop640, one_frame, narrow, wide, stack_below; S = 1 .. 16): the
                                rows equal the replay's bit for bit, h <= 1.2e-5, c <= 8.7e-6 (most 2e-7);
                                T0 = 13 (long): rows 2.2e-3, h 2.7e-4, c 1.5e-4, last row 0 (bound 2e-2)
  stack vs rounded replay       stack_at: rows 1.0e-2, last row 1.1e-2, h 9.3e-3, c 3.1e-3 (bound 2e-2; the stack
                                normalises the fp32 input without the bf16 copy the replay rounds);
                                chunk 0, rows 0..10, stack against fused step: 7.3e-3 (bound 4e-2)
  per-layer vs fused step       S = 17: hop640 6.9e-3, narrow 8.9e-3, long 8.1e-3 of the max (bound 4e-2)
  256 streams vs 16-stream      mid-size body fp32 3072 of 3072 frame tokens, bf16 3050 of 3072 (99.3 %, bound 98 %);
  decoders                      E6D2 body fp32 2048 of 2048
  stack_at ran the launch-persistent forward: last_mode(False) == (1, 16).
"""
import collections
import math
import os

import numpy as np
import pytest
import torch

import fbank_ref as FR
import stream_enc_ref as R
from oracle.make_golden_stream import (CASES, GEOMETRIES, GEOMETRY_CASES, StubVocab, case_wave, geometry_flags, ids_of,
                                       state_dict)
from oracle.stream_ref import StreamOracle

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stream_geometry.npz"))
F32, BF16 = torch.float32, torch.bfloat16
BF16_TOL = 2e-2              # tests/test_stream_encoder_gpu.py
LOG_TOL = 2e-6               # tests/test_fbank_edges_gpu.py: the log output is the correctly rounded log of the linear one
SMALL_CASES = [n for n, c in GEOMETRY_CASES.items() if c.cfg["enc_hidden_size"] < 512]

_MODELS = {}


def _model(key, cfg, wseed, bias, dtype):
    """(Transducer on the device, its state dict): built once per key; the compute dtype is set on every call."""
    if key not in _MODELS:
        from edgedict_amd.models import Transducer
        sd = state_dict(cfg, wseed, bias)
        m = Transducer(enc_dropout=0.0, dec_dropout=0.0, output_loss=False, **cfg)
        m.load_state_dict(sd)
        _MODELS[key] = (m.cuda().eval(), sd)
    m, sd = _MODELS[key]
    m.compute_dtype = dtype
    return m, sd


def _case(name, dtype):
    case = GEOMETRY_CASES[name]
    m, sd = _model(name, case.cfg, case.wseed, case.bias, dtype)
    return case, GEOMETRIES[case.geometry], geometry_flags(case.geometry), m, sd, case_wave(case)


def _mask(S, streams):
    mask = torch.zeros(S, dtype=torch.bool)
    mask[list(streams)] = True
    return mask


# ----------------------------------------------------------------------------------------------- fp32, token-exact
@pytest.mark.parametrize("name", SMALL_CASES)
def test_fp32_single_stream_text_is_the_reference_decoders(hip_lib, name):
    """PytorchStreamDecoder.decode(frame) -> str against the text the REFERENCE's reset / decode returned for the same
    chunks of every stream of the case, across its reset; chunk_geometry gives the table's win / hop."""
    from edgedict_amd.stream import PytorchStreamDecoder, chunk_geometry
    case, geo, flags, m, sd, wave = _case(name, "fp32")
    assert chunk_geometry(flags, geo.step_n_frame) == (geo.win, geo.hop)
    texts = GOLD[name + "_texts"]
    assert texts.shape == (case.S, case.n_chunks)
    dec = PytorchStreamDecoder(flags, transducer=m, tokenizer=StubVocab(), dither=0)
    for s in range(case.S):
        dec.reset()
        for c in range(case.n_chunks):
            if s in case.resets.get(c, []):
                dec.reset()
            got = dec.decode(wave[s:s + 1, c * geo.hop:c * geo.hop + geo.win].clone())
            assert got == str(texts[s, c]), (s, c, got, str(texts[s, c]))
    assert len(dec.encoder_elapsed) == case.S * case.n_chunks


@pytest.mark.parametrize("name", SMALL_CASES)
def test_fp32_batched_streams_emit_the_oracles_ids_frame_by_frame(hip_lib, name):
    """BatchedStreamDecoder with the case's stream count and masked reset: int32 [S, frames out] per chunk, equal to
    StreamOracle's ids frame by frame, blanks included, and without blanks to the reference's texts."""
    from edgedict_amd.stream import BatchedStreamDecoder
    case, geo, flags, m, sd, wave = _case(name, "fp32")
    texts = GOLD[name + "_texts"]
    dec = BatchedStreamDecoder(m, flags, case.S, dither=0)
    oracles = [StreamOracle(sd, flags) for _ in range(case.S)]
    emitted = blanks = 0
    for c in range(case.n_chunks):
        if case.resets.get(c):
            dec.reset(_mask(case.S, case.resets[c]))
            for s in case.resets[c]:
                oracles[s].reset()
        chunk = wave[:, c * geo.hop:c * geo.hop + geo.win]
        got = dec.decode(chunk.cuda().contiguous())
        assert tuple(got.shape) == (case.S, geo.T_out) and got.dtype == torch.int32
        got = got.cpu().numpy()
        for s in range(case.S):
            want = oracles[s].decode(chunk[s:s + 1].clone())
            assert got[s].tolist() == want, (c, s, got[s].tolist(), want)
            assert [t for t in want if t != 0] == ids_of(str(texts[s, c])), (c, s)
            emitted += sum(t != 0 for t in want)
            blanks += sum(t == 0 for t in want)
    assert emitted > 0 and blanks > 0
    assert dec._plan is not None and not dec._plan.ok           # fp32: always the module path


def test_fp32_e6d2_body_at_hop640_reproduces_the_reference_texts(hip_lib):
    """The E6D2 body (6 x 1024) at the benched 40 ms chunk: 3 streams in lock-step and stream 0 through the
    single-stream API, against the reference-executed texts."""
    from edgedict_amd.stream import BatchedStreamDecoder, PytorchStreamDecoder
    case, geo, flags, m, sd, wave = _case("E6D2_hop640", "fp32")
    texts = GOLD["E6D2_hop640_texts"]
    dec = BatchedStreamDecoder(m, flags, case.S, dither=0)
    one = PytorchStreamDecoder(flags, transducer=m, tokenizer=StubVocab(), dither=0)
    assert not case.resets
    for c in range(case.n_chunks):
        chunk = wave[:, c * geo.hop:c * geo.hop + geo.win]
        got = dec.decode(chunk.cuda().contiguous())
        assert tuple(got.shape) == (case.S, geo.T_out)
        got = got.cpu().numpy()
        for s in range(case.S):
            assert [t for t in got[s].tolist() if t != 0] == ids_of(str(texts[s, c])), (c, s)
        assert one.decode(chunk[:1].clone()) == str(texts[0, c]), c


# ----------------------------------------------------------------------------------------------- bf16: the traced runs
# (geometry, streams): 16 / 17 straddles config.STREAM_STEP_MAX_ROWS where T0 > 2
BF16_RUNS = [("native", 4), ("hop640", 1), ("hop640", 16), ("hop640", 17), ("one_frame", 5), ("narrow", 1), ("narrow", 16),
             ("narrow", 17), ("wide", 5), ("long", 1), ("long", 16), ("long", 17), ("stack_below", 3), ("stack_at", 3)]
RESET_CHUNK = 2

Step = collections.namedtuple("Step", "frames h0 c0 tokens h1 c1 pred_h pred_c dec_out plan_ok xs_plan rows_plan")
Trace = collections.namedtuple("Trace", "steps calls mode_before mode_after transform")
_TRACES = {}


def _geometry_model(geometry, dtype):
    """The body a geometry's bf16 runs use: that of its first golden case (narrow: H = 96; stack_below and stack_at: the
    same weights); native: the 'small' case of tests/golden/stream.npz."""
    if geometry == "native":
        cfg, wseed, _, _, _, _, bias = CASES["small"]
        return _model("native", cfg, wseed, bias, dtype)
    name = next(n for n, c in GEOMETRY_CASES.items() if c.geometry == geometry)
    case = GEOMETRY_CASES[name]
    return _model(name, case.cfg, case.wseed, case.bias, dtype)


def _n_chunks(geometry):
    return 3 if geometry.startswith("stack") else 4


def _twin_wave(geometry, S):
    """[S, win + n hop]: one generator per row, so that a longer chunk geometry shares the prefix of every row; rows
    S // 2 .. 2 (S // 2) - 1 repeat rows 0 .. S // 2 - 1."""
    geo = GEOMETRIES[geometry]
    N = geo.win + _n_chunks(geometry) * geo.hop
    rows = [0.1 * torch.randn(N, generator=torch.Generator(device="cpu").manual_seed(500 + s)) for s in range(S)]
    half = S // 2
    for s in range(half):
        rows[half + s] = rows[s].clone()
    return torch.stack(rows)


def _reset_streams(S):
    """Stream 0 and the stream that repeats it (all of S = 1)."""
    return sorted({0, S // 2})


class _Counted:
    """Counts the calls of encoder_stack.EncoderStackFn.apply and models._stream_encoder_step: the two entries of
    Encoder.forward that are not the per-layer kernels."""

    def __enter__(self):
        from edgedict_amd import encoder_stack, models
        self.calls = {"stack": 0, "step": 0}
        self.models, self.fn = models, encoder_stack.EncoderStackFn
        self.step = models._stream_encoder_step
        inner_apply = self.fn.apply

        def stack(*a, **kw):
            self.calls["stack"] += 1
            return inner_apply(*a, **kw)

        def step(*a, **kw):
            self.calls["step"] += 1
            return self.step(*a, **kw)
        self.fn.apply = staticmethod(stack)
        models._stream_encoder_step = step
        return self

    def __exit__(self, *exc):
        del self.fn.apply                      # the inherited classmethod shows again
        self.models._stream_encoder_step = self.step
        return False


def _trace(geometry, S, fast=True):
    """One bf16 run of BatchedStreamDecoder over the chunks of _twin_wave with a masked reset before chunk RESET_CHUNK,
    config.STREAM_FAST_CHUNK = fast: per chunk the frames, the carried encoder state before and after, the tokens, the
    prediction network's state and - where the plan ran - copies of its feature and encoder-row buffers.  Made once."""
    key = (geometry, S, fast)
    if key in _TRACES:
        return _TRACES[key]
    from edgedict_amd import config, encoder_stack
    from edgedict_amd.stream import BatchedStreamDecoder
    geo = GEOMETRIES[geometry]
    m, sd = _geometry_model(geometry, "bf16")
    wave = _twin_wave(geometry, S)
    old = config.STREAM_FAST_CHUNK
    config.STREAM_FAST_CHUNK = fast
    steps = []
    try:
        with _Counted() as counted:
            mode_before = encoder_stack.last_mode(False)
            dec = BatchedStreamDecoder(m, geometry_flags(geometry), S, dither=0)
            for c in range(_n_chunks(geometry)):
                if c == RESET_CHUNK:
                    dec.reset(_mask(S, _reset_streams(S)))
                frames = wave[:, c * geo.hop:c * geo.hop + geo.win].cuda().contiguous()
                h0, c0 = dec.enc_h.clone(), dec.enc_c.clone()
                tokens = dec.decode(frames).cpu()
                torch.cuda.synchronize()
                plan = dec._plan
                ok = plan is not None and plan.ok
                steps.append(Step(frames, h0, c0, tokens, dec.enc_h.clone(), dec.enc_c.clone(), dec.state.h.clone(),
                                  dec.state.c.clone(), dec.state.dec_out.clone(), ok,
                                  plan.xs.clone() if ok else None, plan.rows.clone() if ok else None))
            mode_after = encoder_stack.last_mode(False)
    finally:
        config.STREAM_FAST_CHUNK = old
    _TRACES[key] = Trace(steps, dict(counted.calls), mode_before, mode_after, dec.transform)
    return _TRACES[key]


def _routes(geometry, S):
    """(the plan applies, the stack applies) from the constants of edgedict_amd.config."""
    from edgedict_amd import config
    T0 = GEOMETRIES[geometry].T0
    limit = config.STREAM_STEP_MAX_ROWS_SHORT if T0 <= 2 else config.STREAM_STEP_MAX_ROWS
    return T0 < config.STACK_MIN_FRAMES and S <= limit, T0 >= config.STACK_MIN_FRAMES


_TWINS = {}


def _rows_encoder(geometry):
    """An Encoder WITHOUT the output projection that shares the geometry model's input LayerNorm and LSTM stack: what the
    decoder's encoder call computes before the projection, through the same Encoder.forward routing."""
    if geometry not in _TWINS:
        from edgedict_amd.models import Encoder
        m, _ = _geometry_model(geometry, "bf16")
        lstm = m.encoder.lstm
        red = [i for i, r in enumerate(lstm.reductions) if r == 2]
        twin = Encoder(lstm.lstms[0].input_size, lstm.hidden_size, len(lstm.lstms), 0.0, 8, time_reductions=red, has_proj=False)
        twin.norm, twin.lstm = m.encoder.norm, lstm
        twin.compute_dtype = BF16
        _TWINS[geometry] = twin.cuda().eval()
    return _TWINS[geometry]


def _features(tr, st):
    """The module path's fp32 stacked features of a step's frames (dither is off: the frames are left as they are)."""
    xs, _ = tr.transform(st.frames)
    return xs


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (tuple(a.shape), tuple(b.shape))
    assert bool(torch.isfinite(a).all())
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-3)


# ----------------------------------------------------------------------------------------------- bf16: route, plan, rows
@pytest.mark.parametrize("geometry,S", BF16_RUNS)
def test_bf16_route_is_the_expected_one_and_the_plan_equals_the_module_path(hip_lib, geometry, S):
    """(i) the route: ``dec._plan.ok`` exactly when T0 < STACK_MIN_FRAMES and S <= the row limit of T0; the stack entered
    once per chunk exactly when T0 >= STACK_MIN_FRAMES (stack_at) and never otherwise (stack_below: last_mode(False) is
    what it was before the run); with the plan switched off the fused step is entered once per chunk; with neither
    entry counted (S = 17 at T0 = 3 and 13) the chunk ran on the per-layer kernels, Encoder.forward's ``else`` branch.
    (ii) where the plan applies: tokens, enc_h, enc_c, the prediction network's (h, c) and dec_out are bit-identical
    between plan and module path after every chunk and across the masked reset.  (iii) a stream that repeats another's
    audio and resets has its tokens and states, bit for bit.  (iv) tokens are int32 [S, frames out]."""
    geo, n = GEOMETRIES[geometry], _n_chunks(geometry)
    want_plan, want_stack = _routes(geometry, S)
    tr = _trace(geometry, S, True)
    assert [st.plan_ok for st in tr.steps] == [want_plan] * n
    assert tr.calls == {"stack": n if want_stack else 0, "step": 0}, tr.calls
    if want_stack:
        assert tr.mode_after[0] in (0, 1), tr.mode_after            # a forward kind of the stack
    else:
        assert tr.mode_after == tr.mode_before
    for st in tr.steps:
        assert tuple(st.tokens.shape) == (S, geo.T_out) and st.tokens.dtype == torch.int32
        assert st.h1.dtype == F32 and tuple(st.h1.shape) == tuple(st.h0.shape)
    emitted = sum(int((st.tokens != 0).sum()) for st in tr.steps)
    print("\n[geometry %s S %d] plan %s, calls %s, stack mode %s, %d of %d frame tokens non-blank"
          % (geometry, S, want_plan, tr.calls, tr.mode_after, emitted, n * S * geo.T_out))
    assert emitted > 0
    # the reset did reset: the streams' encoder state entering chunk RESET_CHUNK is zero, the others' is not
    st = tr.steps[RESET_CHUNK]
    hit = _reset_streams(S)
    assert float(st.h0[:, hit].abs().sum()) == 0.0 and float(st.c0[:, hit].abs().sum()) == 0.0
    rest = [s for s in range(S) if s not in hit]
    assert not rest or bool((st.h0[:, rest].abs().sum(dim=(0, 2)) > 0).all())
    if want_plan:
        slow = _trace(geometry, S, False)
        assert not any(s.plan_ok for s in slow.steps)
        assert slow.calls == {"stack": 0, "step": n}, slow.calls
        for c, (a, b) in enumerate(zip(tr.steps, slow.steps)):
            for field in ("tokens", "h1", "c1", "pred_h", "pred_c", "dec_out"):
                assert torch.equal(getattr(a, field), getattr(b, field)), (c, field)
    half = S // 2
    for c, st in enumerate(tr.steps):
        for s in range(half):
            assert torch.equal(st.tokens[s], st.tokens[half + s]), (c, s)
            for field in ("h1", "c1", "pred_h", "pred_c"):
                t = getattr(st, field)
                assert torch.equal(t[:, s], t[:, half + s]), (c, s, field)
            assert torch.equal(st.dec_out[s], st.dec_out[half + s]), (c, s)


def _unstack(x, k, M):
    """[B, T0, k * M] stacked -> [B, M, T0 * k] frames."""
    x = np.asarray(x)
    B, T0, _ = x.shape
    return x.reshape(B, T0, k, M).transpose(0, 3, 1, 2).reshape(B, M, T0 * k)


@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_chunk_features_match_fp64_and_the_plan_writes_their_bf16_rounding(hip_lib, geometry):
    """The stacked features of every chunk of the geometry's first traced run.  Module path, fp32: the linear mel
    energies of the same chunk (the transform's twin with log=False) against tests/fbank_ref.py in the frame-relative
    measure at FBANK_KERNEL_TOL, frames at and past ceil(N / hop) exactly zero, and the log output the decoder consumes
    within LOG_TOL of the logarithm of those energies - metric and bounds of tests/test_fbank_edges_gpu.py, here with the
    truncating stack at N = 520 .. 7520 samples.  Plan: its bf16 ``xs`` buffer equals that fp32 output rounded to bf16,
    bit for bit (stream._ChunkPlan: 'the same rounding')."""
    from edgedict_amd.features import StackedLogFbank
    S = next(s for g, s in BF16_RUNS if g == geometry)
    geo, flags = GEOMETRIES[geometry], geometry_flags(geometry)
    tr = _trace(geometry, S, True)
    k, M = flags.downsample, flags.feature_size
    fb = tr.transform.fbank
    lin = StackedLogFbank(n_frame=k, pad_to_divisible=False, win_length=flags.win_length, hop_length=flags.hop_length,
                          n_fft=flags.n_fft, n_filt=M, dither=0, log=False).cuda()
    live = math.ceil(geo.win / flags.hop_length)
    worst = worst_log = 0.0
    for c, st in enumerate(tr.steps):
        xs = _features(tr, st)
        assert tuple(xs.shape) == (S, geo.T0, geo.I0) and xs.dtype == F32
        xl, _ = lin(st.frames)
        ref = FR.stack64(FR.fbank64(st.frames.cpu(), fb.window, fb.fb, flags.hop_length, flags.n_fft, fb.preemph), k, False)
        assert ref.shape == (S, geo.T0, geo.I0)
        got_lin, ref_lin = _unstack(xl.cpu().numpy(), k, M), _unstack(ref, k, M)
        assert FR.dead_frames_exact(got_lin, ref_lin)
        worst = max(worst, FR.frame_rel_err(got_lin, ref_lin))
        got_log = _unstack(xs.cpu().double().numpy(), k, M)
        n_live = min(live, geo.T0 * k)
        want_log = np.log(got_lin.astype(np.float64) + FR.LOG_FLOOR)
        worst_log = max(worst_log, float(np.abs(got_log[:, :, :n_live] - want_log[:, :, :n_live]).max()))
        assert np.all(got_log[:, :, n_live:] == 0) and np.all(got_lin[:, :, n_live:] == 0)
        if st.plan_ok:
            assert st.xs_plan.dtype == BF16 and tuple(st.xs_plan.shape) == (S, geo.T0, geo.I0)
            assert torch.equal(st.xs_plan.cpu().view(torch.int16), xs.cpu().to(BF16).view(torch.int16)), c
    print("\n[geometry %s S %d] features: linear frame-relative error %.3e (bound %.1e), log %.3e (bound %.1e)"
          % (geometry, S, worst, FR.FBANK_KERNEL_TOL, worst_log, LOG_TOL))
    assert any(st.plan_ok for st in tr.steps) == _routes(geometry, S)[0]
    assert worst <= FR.FBANK_KERNEL_TOL
    assert worst_log <= LOG_TOL


def _replay_checks(geometry, S, tag):
    """Every chunk of the traced run: the rows encoder on the device's own features and previous (h, c) returns the
    decoder's carried state bit for bit (and the plan's row buffer where the plan ran), and rows, last row, h and c are
    within BF16_TOL of the bf16-rounded float64 replay of the same inputs, each on its own scale."""
    geo = GEOMETRIES[geometry]
    tr = _trace(geometry, S, True)
    _, sd = _geometry_model(geometry, "bf16")
    sdk = R.kernel_weights(sd)
    twin = _rows_encoder(geometry)
    worst = {}
    rows_all = []
    for c, st in enumerate(tr.steps):
        xs = _features(tr, st)
        with torch.no_grad():
            rows, (h, cc) = twin(xs, (st.h0, st.c0))
        torch.cuda.synchronize()
        assert tuple(rows.shape) == (S, geo.T_out, twin.lstm.hidden_size)
        assert torch.equal(h, st.h1) and torch.equal(cc, st.c1), "chunk %d: the decoder carried another state" % c
        if st.plan_ok:
            assert torch.equal(rows, st.rows_plan), c
        ref = R.encoder_steps64(sdk, xs.cpu(), (st.h0.cpu(), st.c0.cpu()), (1,), store=BF16)
        assert ref.T_out == geo.T_out
        assert min(t.abs().max().item() for t in (ref.out, ref.out[:, -1], ref.h, ref.c)) > 0.1       # nothing compared is ~0
        for key, a, b in (("rows", rows, ref.out), ("last row", rows[:, -1], ref.out[:, -1]), ("h", h, ref.h), ("c", cc, ref.c)):
            worst[key] = max(worst.get(key, 0.0), _rel(a, b))
        rows_all.append(rows)
    print("\n[geometry %s S %d] %s vs bf16-rounded replay over %d chunks: %s (bound %.0e)"
          % (geometry, S, tag, len(tr.steps), ", ".join("%s %.2e" % kv for kv in worst.items()), BF16_TOL))
    for key, v in worst.items():
        assert v <= BF16_TOL, (geometry, S, key, v)
    return rows_all


@pytest.mark.parametrize("geometry,S", [(g, s) for g, s in BF16_RUNS if GEOMETRIES[g].T0 < 24 and s != 17])
def test_fused_step_route_carries_the_state_of_the_rounded_replay(hip_lib, geometry, S):
    """The fused edgedict_stream_encoder_step at T0 = 1, 2, 3, 13, 23 and I0 = 80 .. 320 inside the decoder: rows, the
    last row on its own (at odd T0 the mean of the last frame and the time reduction's zero pad), and the carried (h, c)
    - the state after the chunk's last real frame - against the replay, chunk after chunk, across the reset."""
    assert _routes(geometry, S) == (True, False)
    _replay_checks(geometry, S, "fused step")


def test_stack_route_on_both_sides_of_the_24_frame_boundary(hip_lib):
    """stack_below (T0 = 23: fused step, odd, padded every chunk) and stack_at (T0 = 24: the layer-pipelined stack with
    carried state), S = 3, 3 chunks, the same weights and the same audio rows: each against the rounded replay at
    BF16_TOL, state after every chunk.  Chunk 0 starts from zeros in both and its first 22 stacked frames are the same
    samples (the 23rd holds the shorter chunk's masked last frame), so the two routes' first 11 rows are each within
    BF16_TOL of ONE replay: they may differ by at most 2 BF16_TOL of its max."""
    assert _routes("stack_below", 3) == (True, False) and _routes("stack_at", 3) == (False, True)
    below = _replay_checks("stack_below", 3, "fused step")
    at = _replay_checks("stack_at", 3, "stack")
    tb, ta = _trace("stack_below", 3), _trace("stack_at", 3)
    assert ta.calls["stack"] == 3 and tb.calls["stack"] == 0
    xb, xa = _features(tb, tb.steps[0]), _features(ta, ta.steps[0])
    assert torch.equal(xb[:, :22], xa[:, :22]) and not torch.equal(xb[:, 22], xa[:, 22])
    d = _rel(at[0][:, :11], below[0][:, :11])
    print("\n[stack boundary] chunk 0, rows 0..10: stack vs fused step %.2e (bound %.0e)" % (d, 2 * BF16_TOL))
    assert d <= 2 * BF16_TOL


@pytest.mark.parametrize("geometry", ["hop640", "narrow", "long"])
def test_per_layer_route_matches_the_fused_step_on_the_same_inputs(hip_lib, geometry):
    """S = 17 at T0 = 3 and 13: one stream beyond config.STREAM_STEP_MAX_ROWS the chunk runs on the per-layer LSTM
    kernels.  Reference: the fused step on the same features and previous state, forced as
    tests/test_stream_gpu.py::test_fused_stream_encoder_step_matches_the_per_layer_path... forces it (the row limit
    lifted), at that test's bounds: 4e-2 of the max, 1e-2 in norm, for rows, h and c, every chunk."""
    from edgedict_amd import config
    S = 17
    assert _routes(geometry, S) == (False, False)
    tr = _trace(geometry, S, True)
    twin = _rows_encoder(geometry)
    worst = 0.0
    for c, st in enumerate(tr.steps):
        xs = _features(tr, st)
        with torch.no_grad(), _Counted() as counted:
            per = twin(xs, (st.h0, st.c0))
        assert counted.calls == {"stack": 0, "step": 0}
        assert torch.equal(per[1][0], st.h1) and torch.equal(per[1][1], st.c1), c
        old = config.STREAM_STEP_MAX_ROWS
        config.STREAM_STEP_MAX_ROWS = 1 << 20
        try:
            with torch.no_grad(), _Counted() as counted:
                fused = twin(xs, (st.h0, st.c0))
        finally:
            config.STREAM_STEP_MAX_ROWS = old
        torch.cuda.synchronize()
        assert counted.calls == {"stack": 0, "step": 1}
        for a, b in ((per[0], fused[0]), (per[1][0], fused[1][0]), (per[1][1], fused[1][1])):
            a, b = a.float(), b.float()
            assert a.shape == b.shape and bool(torch.isfinite(a).all())
            scale = max(b.abs().max().item(), 1e-3)
            worst = max(worst, (a - b).abs().max().item() / scale)
            assert (a - b).abs().max().item() <= 4e-2 * scale, (c, (a - b).abs().max().item(), scale)
            assert (a - b).norm().item() <= 1e-2 * max(b.norm().item(), 1e-6), c
    print("\n[geometry %s S 17] per-layer vs fused step: worst %.2e of the max (bound 4e-2)" % (geometry, worst))


# ----------------------------------------------------------------------------------------------- the benched size: S = 256
BIG_S, GROUP = 256, 16


def _big_setup(name, n_chunks, extra_resets):
    """256 streams: rows 0 .. S0-1 carry the golden case's audio (and resets), the rest seeded noise; the upper 128 repeat
    the lower 128, resets included."""
    case = GEOMETRY_CASES[name]
    geo = GEOMETRIES[case.geometry]
    N = geo.win + n_chunks * geo.hop
    g = torch.Generator(device="cpu").manual_seed(77)
    wave = 0.1 * torch.randn(BIG_S, N, generator=g)
    wave[:case.S] = case_wave(case)[:, :N]
    wave[BIG_S // 2:] = wave[:BIG_S // 2].clone()
    resets = {}
    for src in (case.resets, extra_resets):
        for c, streams in src.items():
            if c < n_chunks:
                resets.setdefault(c, set()).update(streams)
                resets[c].update(s + BIG_S // 2 for s in streams)
    return case, geo, wave, {c: sorted(v) for c, v in resets.items()}


def _run_streams(m, flags, geo, wave, resets, n_chunks, rows=None, states=False):
    """BatchedStreamDecoder over ``rows`` (default: all) of ``wave``: (tokens per chunk [len(rows), T_out] numpy, states
    per chunk or None, the decoder)."""
    from edgedict_amd.stream import BatchedStreamDecoder
    rows = list(range(wave.shape[0])) if rows is None else list(rows)
    dec = BatchedStreamDecoder(m, flags, len(rows), dither=0)
    toks, sts = [], []
    for c in range(n_chunks):
        hit = [i for i, s in enumerate(rows) if s in resets.get(c, [])]
        if hit:
            dec.reset(_mask(len(rows), hit))
        toks.append(dec.decode(wave[rows, c * geo.hop:c * geo.hop + geo.win].cuda().contiguous()).cpu().numpy())
        if states:
            sts.append((dec.enc_h.clone(), dec.enc_c.clone(), dec.state.h.clone(), dec.state.c.clone(), dec.state.dec_out.clone()))
    return toks, sts, dec


def _agreement_with_groups(m, flags, geo, wave, resets, n_chunks, toks, exact):
    same = total = 0
    for g0 in range(0, BIG_S, GROUP):
        small, _, _ = _run_streams(m, flags, geo, wave, resets, n_chunks, rows=range(g0, g0 + GROUP))
        for c in range(n_chunks):
            eq = small[c] == toks[c][g0:g0 + GROUP]
            if exact:
                assert eq.all(), (g0, c, small[c].tolist(), toks[c][g0:g0 + GROUP].tolist())
            same += int(eq.sum())
            total += eq.size
    return same, total


EXTRA_RESETS = {2: [9, 100], 5: [8, 9, 77, 120]}            # never the golden streams


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_256_streams_at_hop640_mid_size_body(hip_lib, dtype):
    """bench.py's stream_256_hop640 shape - 256 streams, 800 / 640-sample chunks of T0 = 3 stacked frames, beyond the
    plan's 16 rows: the module path on the per-layer kernels, an odd frame count padded every chunk - on a mid-size body
    (H = 128, 3 layers, one reduction), 6 chunks, streams 0..4 = the 'hop640_mid' golden with its reset, the upper 128
    streams repeating the lower 128, other streams reset at chunks 2 and 5.
    fp32: streams 0..4 reproduce the reference's texts; streams 0..15 equal StreamOracle frame by frame; every group of 16
    streams equals a 16-stream decoder fed the same rows, token for token; each repeat equals its twin.
    bf16: ``_plan.ok`` is false and neither the stack nor the fused step is entered; each repeat is bitwise equal to its
    twin in tokens and every carried state; agreement with the 16-stream decoders (which DO run the plan and the fused
    step) is printed and must be >= 98 % of the frame tokens, the figure of
    tests/test_stream_gpu.py::test_256_streams_in_lock_step... for the same reason."""
    n_chunks = 6
    case, geo, wave, resets = _big_setup("hop640_mid", n_chunks, EXTRA_RESETS)
    flags = geometry_flags(case.geometry)
    m, sd = _model("hop640_mid", case.cfg, case.wseed, case.bias, dtype)
    with _Counted() as counted:
        toks, sts, dec = _run_streams(m, flags, geo, wave, resets, n_chunks, states=True)
    assert dec._plan is not None and not dec._plan.ok
    assert counted.calls == {"stack": 0, "step": 0}
    assert all(tuple(t.shape) == (BIG_S, geo.T_out) for t in toks)
    half = BIG_S // 2
    for c in range(n_chunks):
        assert np.array_equal(toks[c][:half], toks[c][half:]), c
        if dtype == "bf16":
            h, cc, ph, pc, do = sts[c]
            for t in (h, cc, ph, pc):
                assert torch.equal(t[:, :half], t[:, half:]), c
            assert torch.equal(do[:half], do[half:]), c
    emitted = sum(int((t != 0).sum()) for t in toks)
    assert emitted > 0
    if dtype == "fp32":
        texts = GOLD["hop640_mid_texts"]
        for s in range(case.S):
            for c in range(n_chunks):
                assert [t for t in toks[c][s].tolist() if t != 0] == ids_of(str(texts[s, c])), (c, s)
        oracles = [StreamOracle(sd, flags) for _ in range(GROUP)]
        for c in range(n_chunks):
            for s in range(GROUP):
                if s in resets.get(c, []):
                    oracles[s].reset()
                want = oracles[s].decode(wave[s:s + 1, c * geo.hop:c * geo.hop + geo.win].clone())
                assert toks[c][s].tolist() == want, (c, s)
    same, total = _agreement_with_groups(m, flags, geo, wave, resets, n_chunks, toks, exact=dtype == "fp32")
    print("\n[stream_256_hop640 mid %s] %d of %d frame tokens equal the 16-stream decoders (%d non-blank)"
          % (dtype, same, total, emitted))
    assert same >= 0.98 * total


def test_256_streams_at_hop640_e6d2_body_fp32(hip_lib):
    """bench.py's stream_256_hop640_fp32 under a parity check: the E6D2 body, 256 streams, 4 chunks of 800 / 640 samples.
    Streams 0..2 carry the 'E6D2_hop640' golden and reproduce the reference's texts of its first 4 chunks; every group of
    16 streams equals a 16-stream decoder fed the same rows, token for token; each repeat equals its twin."""
    n_chunks = 4
    case, geo, wave, resets = _big_setup("E6D2_hop640", n_chunks, {2: [9, 100]})
    flags = geometry_flags(case.geometry)
    m, sd = _model("E6D2_hop640", case.cfg, case.wseed, case.bias, "fp32")
    toks, _, dec = _run_streams(m, flags, geo, wave, resets, n_chunks)
    assert dec._plan is not None and not dec._plan.ok
    texts = GOLD["E6D2_hop640_texts"]
    for s in range(case.S):
        for c in range(n_chunks):
            assert [t for t in toks[c][s].tolist() if t != 0] == ids_of(str(texts[s, c])), (c, s)
    for c in range(n_chunks):
        assert tuple(toks[c].shape) == (BIG_S, geo.T_out)
        assert np.array_equal(toks[c][:BIG_S // 2], toks[c][BIG_S // 2:]), c
    same, total = _agreement_with_groups(m, flags, geo, wave, resets, n_chunks, toks, exact=True)
    emitted = sum(int((t != 0).sum()) for t in toks)
    print("\n[stream_256_hop640 E6D2 fp32] %d of %d frame tokens equal the 16-stream decoders (%d non-blank)"
          % (same, total, emitted))
    assert same == total and emitted > 0
