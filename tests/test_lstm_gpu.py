"""GPU: LSTM recurrence kernels (generic fp32/bf16 and the bf16 fragment-order fast path) vs a
plain torch reference of the same cell, forward and backward; further down, the step kernels buffer by buffer, the
weight images and the block's epilogue against float64 (tests/lstm_ref.py) at the kernels' tile edges."""
import pytest
import torch

import lstm_ref as R
from oracle import models_ref as M

pytestmark = pytest.mark.gpu


def _ref_lstm(x, w_ih, w_hh, b_ih, b_hh, h0, c0):
    B, T, _ = x.shape
    H = w_hh.shape[1]
    h, c = h0, c0
    ys = []
    for t in range(T):
        pre = x[:, t] @ w_ih.t() + b_ih + h @ w_hh.t() + b_hh
        i, f, g, o = pre.split(H, 1)
        i, f, g, o = i.sigmoid(), f.sigmoid(), g.tanh(), o.sigmoid()
        c = f * c + i * g
        h = o * c.tanh()
        ys.append(h)
    return torch.stack(ys, 1), h, c


def _run(cd, B, T, I, H, force_generic, seed=0):
    from edgedict_amd import config
    from edgedict_amd.models import _LSTMBlockFn
    g = torch.Generator(device="cpu").manual_seed(seed)
    k = 1.0 / H ** 0.5
    w_ih = ((torch.rand(4 * H, I, generator=g) * 2 - 1) * k).cuda().requires_grad_(True)
    w_hh = ((torch.rand(4 * H, H, generator=g) * 2 - 1) * k).cuda().requires_grad_(True)
    b_ih = ((torch.rand(4 * H, generator=g) * 2 - 1) * k).cuda().requires_grad_(True)
    b_hh = ((torch.rand(4 * H, generator=g) * 2 - 1) * k).cuda().requires_grad_(True)
    x = torch.randn(B, T, I, generator=g).cuda()
    h0 = (0.5 * torch.randn(B, H, generator=g)).cuda()
    c0 = (0.5 * torch.randn(B, H, generator=g)).cuda()
    dy = torch.randn(B, T, H, generator=g).cuda()
    # reference in fp64 on the (possibly bf16-rounded) operands
    xr = x.to(cd).double().requires_grad_(True)
    params = [p.detach().to(cd).double().requires_grad_(True) if p.dim() == 2
              else p.detach().double().requires_grad_(True) for p in (w_ih, w_hh, b_ih, b_hh)]
    yr, hr, cr = _ref_lstm(xr, *params, h0.double(), c0.double())
    (yr * dy.double()).sum().backward()
    config.FORCE_GENERIC_LSTM = force_generic
    try:
        xin = x.to(cd).requires_grad_(True)
        y, hN, cN = _LSTMBlockFn.apply(xin, w_ih, w_hh, b_ih, b_hh, None, None, h0, c0, False, 1, cd)
        (y.float() * dy).sum().backward()
    finally:
        config.FORCE_GENERIC_LSTM = False
    return (y, hN, cN, xin.grad, w_ih.grad, w_hh.grad, b_ih.grad), \
           (yr, hr, cr, xr.grad, params[0].grad, params[1].grad, params[2].grad)


def _close(got, ref, tol):
    ref = ref.float().cuda()
    err = (got.float() - ref).abs().max().item()
    scale = max(ref.abs().max().item(), 1e-3)
    assert err <= tol * scale, (err, scale)


@pytest.mark.parametrize("B,T,I,H", [(3, 5, 24, 32), (16, 7, 64, 64), (64, 4, 256, 256),
                                     (20, 3, 48, 96), (9, 3, 64, 1024), (70, 2, 32, 320)])
def test_fp32_generic_path(hip_lib, B, T, I, H):
    got, ref = _run(torch.float32, B, T, I, H, True)
    for a, b in zip(got, ref):
        _close(a, b, 2e-4)


@pytest.mark.parametrize("force_generic", [True, False])
@pytest.mark.parametrize("B,T,I,H", [(3, 5, 32, 32), (64, 6, 240, 256), (70, 3, 64, 160),
                                     (16, 4, 1024, 1024)])
def test_bf16_paths(hip_lib, force_generic, B, T, I, H):
    got, ref = _run(torch.bfloat16, B, T, I, H, force_generic)
    tols = [2e-2, 2e-2, 2e-2, 4e-2, 4e-2, 4e-2, 4e-2]
    for a, b, tol in zip(got, ref, tols):
        _close(a, b, tol)


def test_bf16_fast_equals_generic_closely(hip_lib):
    fast, _ = _run(torch.bfloat16, 64, 9, 256, 512, False, seed=3)
    gen, _ = _run(torch.bfloat16, 64, 9, 256, 512, True, seed=3)
    for a, b in zip(fast, gen):
        _close(a, b, 1.5e-2)      # same arithmetic, different accumulation split


@pytest.mark.parametrize("B,T,H,with_state", [(64, 9, 1024, True), (37, 12, 256, False), (5, 3, 512, True),
                                              (64, 40, 256, True), (16, 33, 1024, False)])
def test_fp32_launch_persistent_forward_is_bit_identical_to_the_step_kernels(hip_lib, B, T, H, with_state):
    """The exact-f32 recurrence as ONE launch per layer (lstm_fwd_lpw_f32: W_hh slice in registers, c in a register, h
    exchanged through write-through stores and validated gathers) against the launch-per-step kernel it replaces: the
    same MFMA order, the same order of the partial sums, the same cell math - every output (h rows, the h_{t-1} image,
    cell states, final states, the saved gates) must be bit-identical, twice in a row (a stale or torn read would not
    repeat).  This is what carries the token-exactness pinned on the reference's goldens over to the faster path."""
    import os
    from edgedict_amd import encoder_stack, ops
    g = torch.Generator(device="cpu").manual_seed(B + T + H)
    k = 1.0 / H ** 0.5
    w_hh = ((torch.rand(4 * H, H, generator=g) * 2 - 1) * k).cuda()
    G0 = torch.randn(B, T, 4 * H, generator=g).cuda()
    h0 = (0.5 * torch.randn(B, H, generator=g)).cuda() if with_state else None
    c0 = (0.5 * torch.randn(B, H, generator=g)).cuda() if with_state else None

    def run(lpw):
        old = os.environ.get("EDGEDICT_LSTM_F32_LPW")
        os.environ["EDGEDICT_LSTM_F32_LPW"] = "1" if lpw else "0"
        try:
            G = G0.clone()
            out = ops.lstm_forward(G, w_hh, h0, c0)
            torch.cuda.synchronize()
            return (G,) + tuple(out)
        finally:
            if old is None:
                os.environ.pop("EDGEDICT_LSTM_F32_LPW", None)
            else:
                os.environ["EDGEDICT_LSTM_F32_LPW"] = old

    ref = run(False)
    for _ in range(2):
        got = run(True)
        encoder_stack.check_wsr_error()
        for name, a, b in zip(("gates", "Y", "Hprev", "Cst", "hN", "cN"), got, ref):
            assert torch.isfinite(a).all(), name
            assert torch.equal(a, b), (name, (a - b).abs().max().item())


def test_fp32_launch_persistent_forward_on_two_streams_at_once(hip_lib):
    """fp32 mode runs the encoder on the caller's stream and the prediction network on the auxiliary stream, both through
    the launch-persistent kernel, whose workgroups spin until ALL of them are resident: two such launches that each got
    part of the chip wait for each other's CUs until the bounded spins give up (found by the whole suite: E6D2_LARGE in
    fp32, 1 run in ~3; EDGEDICT_LSTM_LPW_NOCHAIN=1 brings it back).  The library chains them - a launch on another stream
    waits for the previous one's event.  Here an encoder-sized and a prediction-network-sized call are queued behind a
    sleeping kernel on two streams, so that both become runnable in the same instant, eight times: results equal to the
    same calls issued alone."""
    from edgedict_amd import encoder_stack, ops, side
    g = torch.Generator(device="cpu").manual_seed(9)
    dev = torch.device("cuda", 0)
    aux = side.stream(dev)
    cur = torch.cuda.current_stream(dev)

    def make(B, T, H):
        w = ((torch.rand(4 * H, H, generator=g) * 2 - 1) / H ** 0.5).cuda()
        return w, torch.randn(B, T, 4 * H, generator=g).cuda()
    wa, Ga = make(64, 40, 1024)          # 256 workgroups: the whole chip
    wb, Gb = make(64, 65, 512)           # 128 workgroups
    ra = ops.lstm_forward(Ga.clone(), wa)[0].clone()
    rb = ops.lstm_forward(Gb.clone(), wb)[0].clone()
    torch.cuda.synchronize()
    for i in range(8):
        ga, gb = Ga.clone(), Gb.clone()
        torch.cuda.synchronize()
        torch.cuda._sleep(40_000_000)            # ~20 ms: the host enqueues both calls meanwhile
        aux.wait_stream(cur)
        order = ("a", "b") if i % 2 == 0 else ("b", "a")
        out = {}
        for which in order:
            if which == "a":
                out["a"] = ops.lstm_forward(ga, wa)[0]
            else:
                with torch.cuda.stream(aux):
                    out["b"] = ops.lstm_forward(gb, wb)[0]
        cur.wait_stream(aux)
        torch.cuda.synchronize()
        encoder_stack.check_wsr_error()
        assert torch.equal(out["a"], ra) and torch.equal(out["b"], rb), i


# ======================================================================================================================
# The step kernels buffer by buffer, the weight images and the block's epilogue against float64 (tests/lstm_ref.py,
# oracle.models_ref) at the kernels' tile edges.  Bounds: the ones above - 2e-4 in fp32 (test_fp32_generic_path), 2e-2 /
# 4e-2 in bf16 for outputs and saved state / gradients (test_bf16_paths) - on the whole buffer AND on every tail alone.
F32, BF16 = torch.float32, torch.bfloat16
OUT_TOL = {F32: 2e-4, BF16: 2e-2}
GRAD_TOL = {F32: 2e-4, BF16: 4e-2}


def _tail_views(t, B, H):
    """(label, view) of a [B,T,H], [B,T,4H] or [B,H] buffer: all of it, the last partial 64-row forward tile and 16-row
    tile, the last (partial) 4-unit forward block and 16-unit backward tile in every gate's column group, the last step."""
    yield "all", t
    for tile in (64, 16):
        r0 = B - (B % tile or tile)
        yield "rows %d:" % r0, t[r0:]
    for tile in (4, 16):
        j0 = H - (H % tile or tile)
        cols = torch.cat([torch.arange(g * H + j0, g * H + H) for g in range(t.shape[-1] // H)])
        yield "units %d:" % j0, t[..., cols]
    if t.dim() == 3:
        yield "last step", t[:, -1]
        yield "first step", t[:, 0]


def _check(name, got, ref, tol, B, H, worst):
    """max |got - ref| <= tol * max(|ref|, 1e-3) on the buffer and on each of its tails, every one on its own scale;
    ``worst[name]`` keeps the largest error / scale seen."""
    got = got.detach().double().cpu()
    ref = ref.detach().double()
    assert got.shape == ref.shape, (name, tuple(got.shape), tuple(ref.shape))
    assert torch.isfinite(got).all(), name
    for (label, a), (_, b) in zip(_tail_views(got, B, H), _tail_views(ref, B, H)):
        err = (a - b).abs().max().item()
        scale = max(b.abs().max().item(), 1e-3)
        worst[name] = max(worst.get(name, 0.0), err / scale)
        assert err <= tol * scale, (name, label, err, scale, tol)


_PROBLEMS = {}


def _step_problem(cd, B, T, H, state):
    """Operands as the kernels see them (W_hh, G_in and dY rounded to the compute dtype, fp32 states) and their float64
    replay; built once per shape."""
    key = (cd, B, T, H, state)
    if key not in _PROBLEMS:
        g = torch.Generator(device="cpu").manual_seed(1000 * H + 10 * B + T)
        w_hh = ((torch.rand(4 * H, H, generator=g) * 2 - 1) / H ** 0.5).to(cd)
        G_in = torch.randn(B, T, 4 * H, generator=g).to(cd)
        h0 = 0.5 * torch.randn(B, H, generator=g) if state else None
        c0 = 0.5 * torch.randn(B, H, generator=g) if state else None
        dY = torch.randn(B, T, H, generator=g).to(cd)
        _PROBLEMS[key] = (w_hh, G_in, h0, c0, dY, R.lstm_steps64(G_in, w_hh, h0, c0, dY))
    return _PROBLEMS[key]


def _run_steps(ops, route, w_hh, G_in, h0, c0, dY):
    """ops.lstm_forward + ops.lstm_backward on fresh device copies, the backward on the forward's own buffers.  "fast":
    the packed images and NO plain W_hh (anything but the fragment-order kernels would refuse); "generic": the plain W_hh
    and its transpose, no image."""
    dev = lambda t: None if t is None else t.cuda()      # noqa: E731
    G, w, h0, c0 = G_in.cuda(), w_hh.cuda(), dev(h0), dev(c0)
    if route == "fast":
        img_f, img_b = ops.lstm_pack_weights(w)
        Y, Hprev, Cst, hN, cN = ops.lstm_forward(G, None, h0, c0, img_f)
    else:
        Y, Hprev, Cst, hN, cN = ops.lstm_forward(G, w, h0, c0)
    gates = G.clone()
    if route == "fast":
        dG = ops.lstm_backward(G, dev(dY), Cst, c0, None, img_b)
    else:
        dG = ops.lstm_backward(G, dev(dY), Cst, c0, w.t().contiguous())
    return gates, Y, Hprev, Cst, hN, cN, dG


# (dtype, route, B, T, H, initial state, EDGEDICT_LSTM_F32_LPW)
STEP_CASES = [
    (F32, "generic", 65, 9, 40, True, None),      # scalar forward AND scalar backward K loops, partial unit tiles, row tails
    (F32, "generic", 17, 3, 8, False, None),      # waves with an empty K slice, the no-state branches
    (F32, "generic", 3, 1, 24, True, None),       # one step
    (F32, "generic", 19, 2, 24, False, None),     # H = 24 with a step t + 1 behind it: the scalar backward loop again
    (F32, "generic", 20, 5, 48, False, None),     # forward scalar (H % 64 != 0), backward f32_product16<1>, clamped batch
    (F32, "generic", 130, 2, 64, True, None),     # forward f32_product16<4> clamped, three forward row tiles
    (F32, "generic", 9, 2, 576, False, None),     # second, partly filled batch of f32_product16<4>
    (F32, "generic", 33, 4, 256, True, "1"),      # the launch-persistent forward itself against float64
    (F32, "generic", 33, 4, 256, True, "0"),
    (F32, "generic", 5, 1, 256, True, None),      # a size the launch-persistent forward owns, declined for T = 1
    (BF16, "generic", 65, 9, 40, True, None),     # a 32-wide K step partly inside H, partial unit tiles
    (BF16, "generic", 17, 3, 8, False, None),
    (BF16, "generic", 1, 1, 24, True, None),
    (BF16, "fast", 65, 9, 32, True, None),        # one k-step: three idle waves
    (BF16, "fast", 17, 1, 160, False, None),      # uneven wave split, one step
    (BF16, "fast", 130, 3, 96, True, None),       # many row tiles, B no multiple of 16
    (BF16, "fast", 5, 2, 544, False, None),       # backward: second, partly filled load batch
    (BF16, "fast", 5, 2, 1056, True, None),       # forward: second, partly filled load batch
]


@pytest.mark.parametrize("cd,route,B,T,H,state,lpw", STEP_CASES)
def test_step_kernels_match_fp64_buffer_by_buffer(hip_lib, monkeypatch, cd, route, B, T, H, state, lpw):
    """ops.lstm_forward / ops.lstm_backward directly: the gates written over G, Y, the h_{t-1} image, the cell states,
    the final states and - from the BPTT run on those very buffers - the pre-activation gradients written over G, each
    against the float64 replay, whole and tail by tail.

    Largest error / max(|ref|, 1e-3) measured on an MI355X, over all cases and views (bounds: fp32 2e-4, bf16 2e-2 and
    4e-2 for dG): fp32 below 3e-7 in every buffer, launch-persistent forward included; bf16 generic gates 2.8e-3,
    Y 2.8e-3, Hprev 3.0e-3, Cst 1.2e-3, hN 1.2e-3, cN 1.2e-3, dG 5.6e-3; bf16 fast gates 2.9e-3, Y 3.2e-3, Hprev 3.1e-3,
    Cst 8.0e-4, hN 3.4e-3, cN 5.7e-4, dG 5.1e-3 - what the replay gives with bf16 rounding at the kernels' stores
    (R.lstm_steps64 / R.lstm_bwd64 with store=bfloat16) and nothing on top."""
    from edgedict_amd import encoder_stack, ops
    if lpw is not None:
        monkeypatch.setenv("EDGEDICT_LSTM_F32_LPW", lpw)
    w_hh, G_in, h0, c0, dY, ref = _step_problem(cd, B, T, H, state)
    gates, Y, Hprev, Cst, hN, cN, dG = _run_steps(ops, route, w_hh, G_in, h0, c0, dY)
    torch.cuda.synchronize()
    if lpw == "1":
        encoder_stack.check_wsr_error()
    assert gates.dtype == Y.dtype == Hprev.dtype == dG.dtype == cd
    assert Cst.dtype == hN.dtype == cN.dtype == F32
    worst = {}
    for name, got, want in (("gates", gates, ref.gates), ("Y", Y, ref.Y), ("Hprev", Hprev, ref.Hprev),
                            ("Cst", Cst, ref.Cst), ("hN", hN, ref.hN), ("cN", cN, ref.cN)):
        _check(name, got, want, OUT_TOL[cd], B, H, worst)
    print("\nlstm steps %s %s B%d T%d H%d state=%d lpw=%s forward: %s"
          % (str(cd)[6:], route, B, T, H, state, lpw, ", ".join("%s %.2e" % kv for kv in worst.items())))
    worst = {}
    _check("dG", dG, ref.dG, GRAD_TOL[cd], B, H, worst)        # (its views include dG[:, 0], the end of the chain)
    print("lstm steps %s %s B%d T%d H%d state=%d lpw=%s backward: dG %.2e" % (str(cd)[6:], route, B, T, H, state, lpw, worst["dG"]))


@pytest.mark.parametrize("cd,route,B,T,H", [(F32, "generic", 5, 3, 24), (BF16, "fast", 5, 3, 32)])
def test_backward_without_dY_leaves_exact_zeros(hip_lib, cd, route, B, T, H):
    """dY = None and the zeroed dc carry: nothing flows, every dG is exactly 0 (and finite: the products of step t + 1
    run on rows of the fragment image past B that nobody wrote)."""
    from edgedict_amd import ops
    w_hh, G_in, h0, c0, _, _ = _step_problem(cd, B, T, H, True)
    dG = _run_steps(ops, route, w_hh, G_in, h0, c0, None)[-1]
    assert dG.dtype == cd and dG.shape == (B, T, 4 * H)
    assert torch.isfinite(dG).all() and bool((dG == 0).all())


def test_entry_points_reject_bad_arguments_before_any_launch(hip_lib):
    from edgedict_amd import ops
    z = lambda *s, dtype=F32: torch.zeros(*s, dtype=dtype, device="cuda")     # noqa: E731
    with pytest.raises(RuntimeError, match="multiple of 8"):
        ops.lstm_forward(z(2, 2, 48), z(48, 12))
    with pytest.raises(RuntimeError, match="multiple of 8"):
        ops.lstm_backward(z(2, 2, 48), None, z(2, 2, 12), None, z(12, 48))
    # the generic route (fp32, or bf16 with H % 32 != 0: an image selects nothing) without the plain matrix
    img = z(4 * 40 * 40, dtype=BF16)
    with pytest.raises(RuntimeError, match="plain W_hh"):
        ops.lstm_forward(z(2, 2, 160), None, None, None, img)
    with pytest.raises(RuntimeError, match="plain W_hh"):
        ops.lstm_forward(z(2, 2, 160, dtype=BF16), None, None, None, img)
    with pytest.raises(RuntimeError, match="plain W_hh"):
        ops.lstm_backward(z(2, 2, 160, dtype=BF16), None, z(2, 2, 40), None, None, img)
    with pytest.raises(RuntimeError, match="null pointer"):
        ops.lstm_forward(z(2, 2, 160), None)
    with pytest.raises(RuntimeError, match="multiple of 32"):
        ops.lstm_pack_weights(z(160, 40))


@pytest.mark.parametrize("src", [F32, BF16])
@pytest.mark.parametrize("H", [32, 96, 160])
def test_weight_images_match_the_layouts_in_the_header_of_lstm_fast(hip_lib, H, src):
    """ops.lstm_pack_weights: both images bit for bit the round-to-nearest-even bf16 cast of W_hh at the places the header
    comment of csrc/lstm_fast.hip gives (R.pack_images: index arithmetic on the CPU); one image on request."""
    from edgedict_amd import ops
    g = torch.Generator(device="cpu").manual_seed(H)
    W = ((torch.rand(4 * H, H, generator=g) * 2 - 1) / H ** 0.5).to(src)
    want_f, want_b = R.pack_images(W)
    bits = lambda t: t.cpu().contiguous().view(torch.int16).flatten()          # noqa: E731
    Wd = W.cuda()
    fwd, bwd = ops.lstm_pack_weights(Wd)
    torch.cuda.synchronize()
    assert fwd.dtype == bwd.dtype == BF16 and fwd.numel() == bwd.numel() == 4 * H * H
    assert torch.equal(bits(fwd), bits(want_f)), "forward image [H/16][4][H/32][64][8]"
    assert torch.equal(bits(bwd), bits(want_b)), "backward image [H/16][4H/32][64][8]"
    f_only, none_b = ops.lstm_pack_weights(Wd, True, False)
    none_f, b_only = ops.lstm_pack_weights(Wd, False, True)
    assert none_b is None and none_f is None
    assert torch.equal(bits(f_only), bits(want_f)) and torch.equal(bits(b_only), bits(want_b))


# (H, B, T, I, initial state, ln, residual, reduce): test_gru_gpu.CASES - what the encoder passes: layer 0 (LN, no
# residual, I != H), layers > 0 (LN + residual, I == H), the reduction layer (reduce 2, odd T ends on a lone frame) - and
# the bare recurrence (no LN)
BLOCK_CASES = [(8, 3, 17, 12, True, False, False, 1),
               (40, 17, 17, 40, False, True, True, 2),
               (40, 130, 1, 24, True, True, False, 2),
               (64, 65, 17, 64, True, True, True, 2),
               (256, 130, 2, 96, False, True, False, 1),
               (256, 1, 17, 256, True, True, True, 1)]


@pytest.mark.parametrize("cd", [F32, BF16])
@pytest.mark.parametrize("H,B,T,I,state,ln,residual,reduce", BLOCK_CASES)
def test_lstm_block_with_epilogue_matches_fp64(hip_lib, cd, H, B, T, I, state, ln, residual, reduce):
    """_LSTMBlockFn whole: input GEMM, step kernels, residual + LayerNorm + TimeReduction epilogue, LN backward, BPTT,
    the in-place accumulating dx GEMM of the residual path, weight-gradient GEMMs and column sums, against
    oracle.models_ref in float64 with autograd, on x and the weight matrices rounded to the compute dtype.

    Largest error / max(|ref|, 1e-3) measured on an MI355X over the six cases: fp32 out 3.5e-7, hN 3.8e-7, cN 3.7e-7,
    dx 1.1e-6, dw_ih 7.3e-7, dw_hh 7.6e-7, db 3.5e-7, dln_w 2.2e-7, dln_b 1.6e-7; bf16 out 5.5e-3, hN 3.1e-3, cN 1.9e-3,
    dx 5.4e-3, dw_ih 4.2e-3, dw_hh 6.3e-3, db 4.8e-3, dln_w 2.4e-3, dln_b 2.0e-8 (a sum of bf16 values in fp32)."""
    from edgedict_amd import models
    from edgedict_amd.models import _LSTMBlockFn
    assert models._lstm_fast(cd, H) == (cd == BF16 and H % 32 == 0)
    g = torch.Generator(device="cpu").manual_seed(H * 7 + B + T)
    k = 1.0 / H ** 0.5
    w_ih = (torch.rand(4 * H, I, generator=g) * 2 - 1) * k
    w_hh = (torch.rand(4 * H, H, generator=g) * 2 - 1) * k
    b_ih = (torch.rand(4 * H, generator=g) * 2 - 1) * k
    b_hh = (torch.rand(4 * H, generator=g) * 2 - 1) * k
    ln_w = 1.0 + 0.2 * torch.randn(H, generator=g)
    ln_b = 0.2 * torch.randn(H, generator=g)
    x = torch.randn(B, T, I, generator=g).to(cd)
    h0 = 0.5 * torch.randn(B, H, generator=g) if state else None
    c0 = 0.5 * torch.randn(B, H, generator=g) if state else None
    Tout = (T + reduce - 1) // reduce if ln else T
    dout = torch.randn(B, Tout, H, generator=g).to(cd)
    x64 = x.double().requires_grad_(True)
    W = [w.to(cd).double().requires_grad_(True) for w in (w_ih, w_hh)]
    Bs = [b.double().requires_grad_(True) for b in (b_ih, b_hh)]
    L = [p.double().requires_grad_(True) for p in (ln_w, ln_b)]
    y64, h64, c64 = M.lstm_layer(x64, W[0], W[1], Bs[0], Bs[1], h0.double() if state else None,
                                 c0.double() if state else None, explicit=True)
    y64.retain_grad()
    out64 = y64
    if ln:
        out64 = M.layer_norm(y64 + x64 if residual else y64, L[0], L[1])
        if reduce == 2:
            out64 = M.time_reduction(out64, 2)
    out64.backward(dout.double())

    dev = [t.cuda().requires_grad_(True) for t in (w_ih, w_hh, b_ih, b_hh, ln_w, ln_b)]
    xin = x.cuda().requires_grad_(True)
    out, hN, cN = _LSTMBlockFn.apply(xin, *dev[:4], dev[4] if ln else None, dev[5] if ln else None,
                                     h0.cuda() if state else None, c0.cuda() if state else None, residual, reduce, cd)
    out.backward(dout.cuda())
    torch.cuda.synchronize()
    assert out.dtype == cd and hN.dtype == F32 and cN.dtype == F32 and xin.grad.dtype == cd
    ot, gt = OUT_TOL[cd], GRAD_TOL[cd]
    worst = {}

    def close(name, got, ref, tol):
        got = got.detach().double().cpu()
        ref = ref.detach().double()
        assert got.shape == ref.shape, (name, tuple(got.shape), tuple(ref.shape))
        assert torch.isfinite(got).all(), name
        err = (got - ref).abs().max().item()
        scale = max(ref.abs().max().item(), 1e-3)
        key = name.split(" ")[0]
        worst[key] = max(worst.get(key, 0.0), err / scale)
        assert err <= tol * scale, (name, err, scale, tol)

    close("out", out, out64, ot)
    close("hN", hN, h64, ot)
    close("cN", cN, c64, ot)
    close("dx", xin.grad, x64.grad, gt)
    for name, p, r in zip(("dw_ih", "dw_hh", "db_ih", "db_hh"), dev[:4], W + Bs):
        close(name, p.grad, r.grad, gt)
    if ln:
        close("dln_w", dev[4].grad, L[0].grad, gt)
        close("dln_b", dev[5].grad, L[1].grad, gt)
    else:
        assert dev[4].grad is None and dev[5].grad is None
    # tails on their own: the last partial 64-row forward tile / 16-row tile, the last partial 16-unit backward tile (its
    # rows of dW_hh and db_hh, one group per gate), the lone last frame of the time reduction
    for tile in (64, 16):
        r0 = B - (B % tile or tile)
        close("out rows %d:" % r0, out[r0:], out64[r0:], ot)
        close("hN rows %d:" % r0, hN[r0:], h64[r0:], ot)
        close("cN rows %d:" % r0, cN[r0:], c64[r0:], ot)
        close("dx rows %d:" % r0, xin.grad[r0:], x64.grad[r0:], gt)
    j0 = H - (H % 16 or 16)
    rows = torch.cat([torch.arange(gate * H + j0, gate * H + H) for gate in range(4)])
    close("dw_hh last unit tile", dev[1].grad[rows.cuda()], W[1].grad[rows], gt)
    close("db_hh last unit tile", dev[3].grad[rows.cuda()], Bs[1].grad[rows], gt)
    if ln and reduce == 2 and T % 2 == 1:
        close("out last frame", out[:, -1], out64[:, -1], ot)
    print("\nlstm block %s H%d B%d T%d I%d: %s" % (str(cd)[6:], H, B, T, I, ", ".join("%s %.2e" % kv for kv in worst.items())))
    # both biases enter the same pre-activation: their gradients are the same column sums of the same dG buffer.  The
    # sums are fp32, accumulated atomically by one workgroup per 64 rows: with at most two of them (B T <= 128) addition
    # commutes and the two results are the same bits; with more, two orders of one n-term fp32 sum differ by at most
    # 2 (n - 1) 2^-24 sum |terms| per column (n = B T; the terms from the float64 replay of this very problem, each with
    # the kernels' own bound on top)
    db_ih, db_hh = dev[2].grad, dev[3].grad
    if B * T <= 128:
        assert torch.equal(db_ih, db_hh)
    else:
        n = B * T
        G_in = (x64 @ W[0].t() + Bs[0] + Bs[1]).detach()
        dG64 = R.lstm_steps64(G_in, W[1], h0, c0, y64.grad).dG.view(n, 4 * H).abs()
        bound = 2 * (n - 1) * 2.0 ** -24 * (dG64.sum(0) + n * gt * max(dG64.max().item(), 1e-3))
        assert ((db_ih - db_hh).abs().double().cpu() <= bound).all()
