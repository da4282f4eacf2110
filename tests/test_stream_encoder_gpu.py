"""GPU: edgedict_stream_encoder_step (csrc/decode_fused.hip) - the streaming decoder's encoder call, enc_lstm_step<1> for
up to 16 rows and enc_lstm_tile beyond - against the float64 replay of tests/stream_enc_ref.py at the kernels' tile
edges (the cases and what each is there for: stream_enc_ref.CASES).

The call is made directly through ctypes with the test's own state, output and workspace tensors, the arguments built as
models._stream_encoder_step builds them (the weights through WEIGHTS.get(..., bf16)); one test asserts that
Encoder.forward takes this very call.  Every buffer the call writes has a 4 KiB guard behind it, checked after every call.

Bounds: 2e-2 of the buffer's (or the tail's) max for everything judged against the bf16-rounded replay (OUT_TOL[BF16] of
tests/test_lstm_gpu.py); for the step kernels on the operands they actually read, F32_TOL on the fp32 states and one
bf16 rounding on the y rows; no tolerance for the bit-for-bit properties.  tests/test_stream_enc_ref_host.py shows on the
CPU that the replay alone stays inside the first bound and that seven arithmetic errors each overshoot it five times."""
import collections
import ctypes

import pytest
import torch

import stream_enc_ref as R

pytestmark = pytest.mark.gpu

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
BF16_TOL = 2e-2
# fp32 states of a layer against layer_steps64 on the operands the kernels read, error / max(|ref|, 1e-3).  Measured on
# an MI355X over all cases: h 2.52e-7 (H = 544), c 1.96e-7 (K = 40) at the most - fp32 accumulation of exact bf16 products
# and the fast exponentials, nothing else.  The bound is 4 x the largest, rounded up to one significant digit (1.008e-6 ->
# 2e-6): inputs are seeded and the kernels deterministic, the margin is for another summation order or __expf.
F32_TOL = 2e-6
GUARD = 4096
PATTERN = 0xA5

Result = collections.namedtuple("Result", "out h c T_out X_last Y_last")


def _align256(n):
    return (n + 255) // 256 * 256


class _Guarded:
    """``nbytes`` of device memory with GUARD bytes of PATTERN behind them."""

    def __init__(self, nbytes):
        self.nbytes = nbytes
        self.raw = torch.empty(nbytes + GUARD, dtype=torch.uint8, device="cuda")
        self.raw[:nbytes] = 0
        self.raw[nbytes:] = PATTERN

    def view(self, dtype, *shape):
        n = torch.empty(0, dtype=dtype).element_size()
        for s in shape:
            n *= s
        return self.raw[:n].view(dtype).view(*shape)

    def intact(self):
        return bool((self.raw[self.nbytes:] == PATTERN).all())


_ENCODERS = {}


def _encoder(key, cs, sd):
    """models.Encoder (no projection) holding the problem's parameters, built once per case."""
    if key not in _ENCODERS:
        from edgedict_amd.models import Encoder
        enc = Encoder(cs.I0, cs.H, cs.L, 0.0, 8, time_reductions=list(cs.red), has_proj=False)
        enc.load_state_dict({k[len("encoder."):]: v for k, v in sd.items()})
        enc = enc.cuda().eval()
        enc.compute_dtype = BF16
        _ENCODERS[key] = enc
    return _ENCODERS[key]


def _call(enc, x, hid):
    """edgedict_stream_encoder_step on x [B,T,I0] (device, fp32 or bf16) and hid = (h, c) [L,B,H] fp32 or None (zeros).
    The workspace layout is recomputed from the comment in csrc/decode_fused.hip - X at 0, the other activation buffer at
    ``act``, Y at 2 act, act = align256(B T max(I0, H) 2) - and its total must be what the library reports."""
    from edgedict_amd import _lib
    from edgedict_amd.models import WEIGHTS
    lib = _lib.load()
    lstm = enc.lstm
    B, T, I0 = x.shape
    H, L = lstm.hidden_size, len(lstm.lstms)
    assert x.is_cuda and x.is_contiguous() and x.dtype in (F32, BF16)
    T_out = enc.output_frames(T)
    D = max(I0, H)
    act = _align256(B * T * D * 2)
    total = 4 * act + 2 * _align256(B * H * 4) + 2 * _align256(B * T * 4) + _align256(L * B * H * 2)
    assert total == lib.edgedict_stream_encoder_workspace_bytes(B, T, I0, H, L), "the workspace layout changed"
    ws, gout = _Guarded(total), _Guarded(B * T_out * H * 2)
    gh, gc = _Guarded(L * B * H * 4), _Guarded(L * B * H * 4)
    out, h, c = gout.view(BF16, B, T_out, H), gh.view(F32, L, B, H), gc.view(F32, L, B, H)
    if hid is not None:
        h.copy_(hid[0])
        c.copy_(hid[1])
    w_ih = [WEIGHTS.get(m.layer(0)[0], BF16) for m in lstm.lstms]
    w_hh = [WEIGHTS.get(m.layer(0)[1], BF16) for m in lstm.lstms]
    b_ih = [m.layer(0)[2].detach() for m in lstm.lstms]
    b_hh = [m.layer(0)[3].detach() for m in lstm.lstms]
    gam = [p[0].weight.detach() for p in lstm.projs]
    bet = [p[0].bias.detach() for p in lstm.projs]
    assert all(w.dtype == BF16 and w.is_contiguous() for w in w_ih + w_hh)

    def arr(ts):
        return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    red = (ctypes.c_int * L)(*[int(r) for r in lstm.reductions])
    t_out = ctypes.c_int(-1)
    rc = lib.edgedict_stream_encoder_step(
        _lib.ptr(x), _lib.dtype_code(x.dtype), B, T, I0, H, L, _lib.ptr(enc.norm.weight.detach()),
        _lib.ptr(enc.norm.bias.detach()), arr(w_ih), arr(w_hh), arr(b_ih), arr(b_hh), arr(gam), arr(bet), red,
        _lib.ptr(h), _lib.ptr(c), _lib.ptr(out), ctypes.byref(t_out), _lib.ptr(ws.raw), _lib.stream_ptr())
    _lib.check(rc, "stream_encoder_step")
    torch.cuda.synchronize()
    for name, g in (("workspace", ws), ("out", gout), ("h", gh), ("c", gc)):
        assert g.intact(), "the call wrote behind the end of %s" % name
    # the last layer's operands as they lie in the workspace: its input [B, T_l, K_l] in activation buffer (L - 1) % 2
    # (the buffers swap per layer, the last layer's output goes to ``out``), its y rows [B, T_l, H] in Y
    Tl = T
    for r in lstm.reductions[:-1]:
        Tl = (Tl + r - 1) // r
    Kl = I0 if L == 1 else H
    off = ((L - 1) % 2) * act
    X_last = ws.raw[off:off + B * Tl * Kl * 2].view(BF16).view(B, Tl, Kl).clone()
    Y_last = ws.raw[2 * act:2 * act + B * Tl * H * 2].view(BF16).view(B, Tl, H).clone()
    return Result(out.clone(), h.clone(), c.clone(), t_out.value, X_last, Y_last)


_RESULTS = {}


def _result(name):
    """The native call on problem(name), made once; callers leave it unchanged."""
    if name not in _RESULTS:
        sd, x, hid = R.problem(name)
        enc = _encoder(name, R.CASES[name], sd)
        _RESULTS[name] = _call(enc, x.cuda(), None if hid is None else (hid[0].cuda(), hid[1].cuda()))
    return _RESULTS[name]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a[:3], b[:3])) and a.T_out == b.T_out


def _views(t, state, B, H):
    """(label, view) of the output [B,T',H] or of a state [L,B,H]: all of it, the rows of the last partial 64-row tile
    (enc_lstm_tile) and 16-row tile (enc_lstm_step), the last 16-unit block, the last output frame / the last layer."""
    rows = (lambda r0: t[:, r0:]) if state else (lambda r0: t[r0:])
    yield "all", t
    for tile in (64, 16):
        r0 = B - (B % tile or tile)
        yield "rows %d:" % r0, rows(r0)
    yield "units %d:" % (H - 16), t[..., H - 16:]
    if state:
        yield "last layer", t[-1]
    else:
        yield "last frame", t[:, -1]


def _check(name, got, ref, state, B, H, worst):
    """max |got - ref| <= 2e-2 * max(|ref|, 1e-3) on the buffer and on each tail, every one on its own scale."""
    got, ref = got.detach().double().cpu(), ref.detach().double()
    assert got.shape == ref.shape, (name, tuple(got.shape), tuple(ref.shape))
    assert torch.isfinite(got).all(), name
    for (label, a), (_, b) in zip(_views(got, state, B, H), _views(ref, state, B, H)):
        assert a.numel() > 0, (name, label)
        err, scale = (a - b).abs().max().item(), max(b.abs().max().item(), 1e-3)
        worst[name] = max(worst.get(name, 0.0), err / scale)
        assert err <= BF16_TOL * scale, (name, label, err, scale)


def _check_result(tag, got, ref, cs):
    assert got.out.dtype == BF16 and got.h.dtype == got.c.dtype == F32
    assert got.T_out == ref.T_out and tuple(got.out.shape) == (cs.B, ref.T_out, cs.H)
    worst = {}
    _check("out", got.out, ref.out, False, cs.B, cs.H, worst)
    _check("h", got.h, ref.h, True, cs.B, cs.H, worst)
    _check("c", got.c, ref.c, True, cs.B, cs.H, worst)
    print("\nstream encoder %s vs bf16-rounded replay: %s" % (tag, ", ".join("%s %.2e" % kv for kv in worst.items())))


@pytest.mark.parametrize("name", list(R.CASES))
def test_output_and_states_match_the_rounded_replay(hip_lib, name):
    """End to end: the output and every layer's final h and c against the replay that rounds where the call stores bf16,
    whole and tail by tail; finite, bf16 out, fp32 states, the returned T_out.

    Largest error / max(|ref|, 1e-3) measured on an MI355X, over all views (bound 2e-2): in 14 of the 16 cases the bf16
    output equals the rounded replay's bit for bit and the states differ by fp32 rounding (h <= 1.2e-5, c <= 6.6e-6,
    most 2e-7); where a value fell on the other side of a bf16 rounding somewhere upstream: h160 out 8.6e-4, h 2.3e-4,
    c 2.4e-4; deep out 2.3e-3, h 1.6e-3, c 9.1e-4 - the largest."""
    _check_result(name, _result(name), R.replay(name, BF16), R.CASES[name])


@pytest.mark.parametrize("name", list(R.CASES))
def test_step_kernels_on_the_operands_they_read(hip_lib, name):
    """As stored: the LAST layer of every case (the only layer of the T = 1 cases) judged on what its launches read - its
    input X and, for t > 0, its own previous y row, both taken from the workspace after the call, the bf16 rounding of
    the carried h the test passed in (made here, by torch's cast) and the carried c.  layer_steps64 on those; the fp32 h
    and c at F32_TOL of the buffer's max, every y row within one bf16 rounding of the value,
    |y - ref| <= 2^-8 (|ref| + slack) + slack with slack = F32_TOL max|ref|.  No rounding decision upstream enters.

    Largest error / max(|ref|, 1e-3) measured on an MI355X, per case h / c (bound F32_TOL = 2e-6): k8_step 1.3e-7 / 9.8e-8,
    k8_tile 1.7e-7 / 8.1e-8, h32 1.8e-7 / 8.3e-8, k40 1.6e-7 / 2.0e-7, k240 B = 1 .. 130 1.2e-7 .. 2.3e-7 / 1.1e-7 .. 1.3e-7,
    h96 1.6e-7 / 1.2e-7, h160 2.2e-7 / 1.9e-7, k520 1.5e-7 / 9.1e-8, h544 2.5e-7 / 1.3e-7, odd_t 1.4e-7 / 1.1e-7, deep
    2.0e-7 / 1.1e-7; no y row was further than one bf16 rounding from the float64 value in any case."""
    cs = R.CASES[name]
    sd, x, hid = R.problem(name)
    got = _result(name)
    l = cs.L - 1
    q = "encoder.lstm.lstms.%d." % l
    if hid is None:
        hb = c0 = torch.zeros(cs.B, cs.H)
    else:
        hb, c0 = hid[0][l].to(BF16), hid[1][l]
    X, Y = got.X_last.cpu(), got.Y_last.cpu()
    ry, rh, rc = R.layer_steps64(X, sd[q + "weight_ih_l0"], sd[q + "weight_hh_l0"], sd[q + "bias_ih_l0"],
                                 sd[q + "bias_hh_l0"], hb, c0, Y_stored=Y)
    worst = {}
    for key, a, b in (("h", got.h[l], rh), ("c", got.c[l], rc)):
        err, scale = (a.double().cpu() - b).abs().max().item(), max(b.abs().max().item(), 1e-3)
        worst[key] = err / scale
    slack = F32_TOL * max(ry.abs().max().item(), 1e-3)
    over = ((Y.double() - ry).abs() - 2.0 ** -8 * (ry.abs() + slack)).max().item()
    worst["y beyond one rounding"] = max(over, 0.0) / max(ry.abs().max().item(), 1e-3)
    print("\nstream encoder %s layer %d as stored: %s" % (name, l, ", ".join("%s %.2e" % kv for kv in worst.items())))
    assert worst["h"] <= F32_TOL and worst["c"] <= F32_TOL, worst
    assert over <= slack, (over, slack)
    # the last y row IS the bf16 rounding of the fp32 h the kernel returned
    assert torch.equal(Y[:, -1], got.h[l].cpu().to(BF16))


@pytest.mark.parametrize("B", [5, 17])
def test_state_carried_over_three_calls(hip_lib, B):
    """Three consecutive T = 1 calls at (B, 1, 240, 64, 2, []), each fed the state the previous one returned, against the
    replay run the same way; and Encoder.forward on the same chunks returns the same bits without touching the state
    tensors it was given (models._stream_encoder_step clones them).  Measured on an MI355X (bound 2e-2): B = 5 out 0,
    h 2.5e-7, c 1.6e-7 in every call; B = 17 grows over the calls to out 3.4e-4, h 1.0e-4, c 1.1e-4 in the third."""
    cs = R.Case(B, 1, 240, 64, 2, (), True, F32)
    sd, x0, hid = R.make_problem(cs, 100 + B)
    g = torch.Generator(device="cpu").manual_seed(200 + B)
    xs = [x0] + [x0 + 0.5 * torch.randn(x0.shape, generator=g) for _ in range(2)]
    enc = _encoder(("carry", B), cs, sd)
    state, rstate = (hid[0].cuda(), hid[1].cuda()), hid
    for i, x in enumerate(xs):
        got = _call(enc, x.cuda(), state)
        ref = R.encoder_steps64(sd, x, rstate, cs.red, store=BF16)
        _check_result("carry B%d call %d" % (B, i), got, ref, cs)
        keep = (state[0].clone(), state[1].clone())
        with torch.no_grad():
            y, (h, c) = enc(x.cuda(), state)
        torch.cuda.synchronize()
        assert torch.equal(state[0], keep[0]) and torch.equal(state[1], keep[1]), "the caller's state was modified"
        assert torch.equal(y, got.out) and torch.equal(h, got.h) and torch.equal(c, got.c)
        state, rstate = (got.h, got.c), (ref.h, ref.c)


@pytest.mark.parametrize("name", list(R.CASES))
def test_encoder_forward_takes_this_call(hip_lib, monkeypatch, name):
    """Routing: bf16, no_grad and config.STREAM_ENCODER_STEP send Encoder.forward through models._stream_encoder_step at
    every listed shape (the row limit for chunks of more than two frames lifted, as the decoder's own test does), and what
    it returns is the direct call's result bit for bit: the rest of this file tests the path the decoder uses."""
    from edgedict_amd import config, models
    cs = R.CASES[name]
    sd, x, hid = R.problem(name)
    enc = _encoder(name, cs, sd)
    calls = []
    inner = models._stream_encoder_step

    def counted(*a):
        calls.append(1)
        return inner(*a)
    monkeypatch.setattr(models, "_stream_encoder_step", counted)
    monkeypatch.setattr(config, "STREAM_ENCODER_STEP", True)
    monkeypatch.setattr(config, "STREAM_STEP_MAX_ROWS", 1 << 20)
    with torch.no_grad():
        y, (h, c) = enc(x.cuda(), None if hid is None else (hid[0].cuda(), hid[1].cuda()))
    torch.cuda.synchronize()
    assert len(calls) == 1
    got = _result(name)
    assert y.dtype == BF16 and torch.equal(y, got.out) and torch.equal(h, got.h) and torch.equal(c, got.c)


@pytest.mark.parametrize("name", ["k240_b17", "h32", "k240_b130"])
def test_reversed_batch_gives_the_reversed_result_bit_for_bit(hip_lib, name):
    """B = 17, 65, 130: rows and state reversed - every row passes through a clamped partial tile in one of the runs."""
    sd, x, hid = R.problem(name)
    enc = _encoder(name, R.CASES[name], sd)
    fwd = _result(name)
    rev = _call(enc, x.flip(0).contiguous().cuda(), (hid[0].flip(1).contiguous().cuda(), hid[1].flip(1).contiguous().cuda()))
    assert torch.equal(rev.out.flip(0), fwd.out)
    assert torch.equal(rev.h.flip(1), fwd.h) and torch.equal(rev.c.flip(1), fwd.c)


@pytest.mark.parametrize("name", ["h32", "k240_b65"])
def test_every_row_alone_equals_its_row_in_the_batch_bit_for_bit(hip_lib, name):
    """B = 65 goes through enc_lstm_tile, a row alone through enc_lstm_step<1>: the comment above enc_lstm_tile claims the
    two compute the same bits, so a stream's state does not depend on how many streams share its batch.  EVERY row."""
    cs = R.CASES[name]
    sd, x, hid = R.problem(name)
    enc = _encoder(name, cs, sd)
    batch = _result(name)
    xd, hd, cd = x.cuda(), hid[0].cuda(), hid[1].cuda()
    for b in range(cs.B):
        one = _call(enc, xd[b:b + 1].contiguous(), (hd[:, b:b + 1].contiguous(), cd[:, b:b + 1].contiguous()))
        assert torch.equal(one.out, batch.out[b:b + 1]), b
        assert torch.equal(one.h, batch.h[:, b:b + 1]) and torch.equal(one.c, batch.c[:, b:b + 1]), b


@pytest.mark.parametrize("name", ["k240_b16", "h32"])
def test_fp32_input_that_is_bf16_equals_the_bf16_input(hip_lib, name):
    cs = R.CASES[name]
    assert cs.xdtype == F32
    sd, x, hid = R.problem(name)
    enc = _encoder(name, cs, sd)
    xb = x.to(BF16)
    state = (hid[0].cuda(), hid[1].cuda())
    assert _same(_call(enc, xb.float().cuda(), state), _call(enc, xb.cuda(), state))


@pytest.mark.parametrize("name", ["k8_step", "k240_b130"])
def test_nothing_is_written_behind_the_buffers(hip_lib, name):
    """The workspace, out, h and c each with a 4 KiB guard of 0xA5 behind the size the library asks for: untouched (_call
    asserts it for every call of this file; here for one small case and one of the tile kernel, on fresh buffers), and
    the call is deterministic."""
    sd, x, hid = R.problem(name)
    enc = _encoder(name, R.CASES[name], sd)
    again = _call(enc, x.cuda(), (hid[0].cuda(), hid[1].cuda()))
    assert _same(again, _result(name))
