"""GPU: the kernels of the bf16 encoder stack (csrc/encoder_stack.hip, csrc/stack_kernels.hip) against a float64
restatement of the same operation (tests/stack_ref.py), buffer by buffer, at the kernels' tile edges.

``EncoderStackFn.apply`` is driven directly (no projection), every recurrence route a geometry allows is run and
asserted through ``encoder_stack.last_mode``, and the buffers of the pass are read from the Function's plan:

  forward, per layer      the gates, h, c, final states against ``layer_forward64`` fed the kernel's OWN stored input X_l
                          (a one-layer bound whatever the depth: 2e-2, OUT_TOL[bf16] of test_lstm_gpu / test_gru_gpu);
                          frame 0 of the h / c images exactly; the LayerNorm statistics against float64 statistics of the
                          kernel's own h rows (1e-5); X_0, X_{l+1} and ``out`` against the LayerNorm (+ pair mean) of the
                          kernel's own rows (one bf16 ulp, 2^-8: the bounds of tests/test_layer_kernels_gpu.py)
  weight-gradient         dW_ih, dW_hh, db against float64 products of the kernel's own dG, X, h_{t-1} buffers (exactly
  products, per layer     representable operands), ELEMENTWISE within K 2^-23 (|dG|^T |X|), K = T B terms: the bound of an
                          fp32 sum of K exact products in any order, so chunking, split-K and atomics fall under it
  backward, end to end    dG of every layer and every parameter gradient against ``stack_forward64`` + autograd: 4e-2
                          (GRAD_TOL[bf16] of test_lstm_gpu) for one layer; for more layers the yardstick of
                          test_stack_tracks_fp32_parity_mode - the per-layer bf16 path (pinned to float64 layer by layer
                          in test_lstm_gpu) on the same problem: err <= 2 err_per_layer + 2e-2 and never above 6e-2 (the
                          per-layer path's dG is read from its autograd nodes)

Every comparison is max |got - ref| <= tol max(|ref|, 1e-3) on the whole buffer AND on each tail alone (``_views``).

The same under dropout (``test_stack_kernels_under_dropout_match_fp64_under_the_same_masks``): the forward norm role
rounds to bf16, masks and scales, the LayerNorm backward regenerates the mask, both from the stateless hash that
tests/dropout_ref.py restates - so the float64 reference carries the IDENTICAL masks and every bound above stays as it
is; the masked outputs of every layer get exact zeros and two bf16 roundings (2 x 2^-8).
"""
import pytest
import torch

import dropout_ref as D
import stack_ref as S
from oracle import models_ref as M

pytestmark = pytest.mark.gpu

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
OUT_TOL = 2e-2              # test_lstm_gpu.OUT_TOL[bf16]: one layer, bf16 stores
GRAD_TOL = 4e-2             # test_lstm_gpu.GRAD_TOL[bf16]: one layer
STAT_TOL = 1e-5             # test_layer_kernels_gpu._ln_check: fp32 statistics of bf16-exact inputs
BF16_ULP = 2.0 ** -8        # test_layer_kernels_gpu.BF16_ULP: a bf16 LayerNorm output
DEEP_CAP, DEEP_SLACK = 6e-2, 2e-2      # test_stack_tracks_fp32_parity_mode: r_new < 6e-2 and < 2 r_old + 2e-2
DROP_P, DROP_SEED = 0.3, 21            # the dropout cases: p, and the torch.manual_seed the per-layer yardstick runs under

# name: (B, T0, I0, H, L, reductions, chunk, lag, initial states, dtype of x), forward kinds, backward kinds that can run
# (kind 0 = a launch per step, 1 = launch-persistent forward, 2 = split-K weights-stationary BPTT).  Checked against
# lpw_steps / sk_bwd_steps (csrc/encoder_stack.hip) and ed_stack_lpw_supported / ed_stack_sk_supported
# (csrc/stack_kernels.hip): the persistent forward needs H / 32 <= 32 and (H / 16) ceil(B / 64) <= 64, and an even number of
# steps per launch under a reduction (the chunks here are even); the split-K BPTT B <= 64, H % 64 == 0, H <= 1024.
CASES = {
    # one step, no gfrag_in, smallest I0 and H; one forward k-step: three waves with an empty K slice
    "a": ((3, 1, 8, 32, 1, [1], 2, 0, False, F32), (0, 1), (0,)),
    # one row past a 16-row tile; odd T under a reduction in layer 0: the lone last frame in the norm and its backward
    "b": ((17, 5, 24, 64, 1, [2], 2, 0, True, F32), (0, 1), (0, 2)),
    # one row past the 32-row group of bwd_step_role; KS = 3 forward (wave 3 idle), three 32-unit backward blocks; a
    # residual layer, a reduction in the LAST layer, bf16 x; the persistent forward with empty row tiles
    "c": ((33, 7, 40, 96, 2, [1, 2], 2, 0, True, BF16), (0, 1), (0,)),
    # two forward row groups, the second with one row; uneven K split (KS = 5); a reduction below a residual layer
    "d": ((65, 4, 16, 160, 2, [2, 1], 4, 0, False, F32), (0, 1), (0,)),
    # the benched topology: I0 = 240, reduction after layer 1; full tiles everywhere
    "e": ((64, 6, 240, 128, 3, [1, 2, 1], 2, 0, True, F32), (0, 1), (0, 2)),
    # two reductions, T0 no multiple of 4: both layers end on a lone frame; non-zero lag; several launches
    "f": ((2, 35, 8, 64, 2, [2, 2], 4, 3, False, F32), (0, 1), (0, 2)),
    # LayerNorm backward: the second 512-column pass with 32 live columns; KS = 17: waves split 5 / 5 / 5 / 2
    "g": ((5, 3, 16, 544, 1, [1], 2, 0, True, F32), (0, 1), (0,)),
    # H above 1024: the persistent forward must decline; second, partly filled load batch of the step kernel
    "h": ((5, 2, 16, 1056, 1, [1], 2, 0, False, F32), (0,), (0,)),
    # the largest H and I0 supported() admits: all four column passes of the LayerNorm backward, the input norm at 1024
    "i": ((3, 2, 1024, 2048, 1, [1], 2, 0, True, F32), (0,), (0,)),
}
RUNS = [(name, fk, bk) for name, (_, fks, bks) in CASES.items() for fk in fks for bk in bks]


# ------------------------------------------------------------------------------------------------------------ views
def _views(t, spec, B, H):
    """(label, view) of a buffer whose dimensions ``spec`` names: b batch rows, t time steps, u hidden units (H of them
    or one group of H per gate), i input columns, - anything else.  All of it; the rows from the last multiple of 16, 32
    and 64; the units of the last 16-, 32- and 64-unit block in every gate's group; the first and the last step (the last
    output frame is the lone one where a reduction leaves one); the last 8 input columns."""
    yield "all", t
    for d, kind in enumerate(spec):
        n = t.shape[d]
        if kind == "b":
            for tile in (16, 32, 64):
                r0 = B - (B % tile or tile)
                yield "rows %d:" % r0, t.narrow(d, r0, B - r0)
        elif kind == "u":
            assert n % H == 0
            for tile in (16, 32, 64):
                j0 = H - (H % tile or tile)
                idx = torch.cat([torch.arange(g * H + j0, g * H + H) for g in range(n // H)])
                yield "dim %d units %d:" % (d, j0), t.index_select(d, idx)
        elif kind == "t":
            yield "first step", t.select(d, 0)
            yield "last step", t.select(d, n - 1)
        elif kind == "i":
            yield "dim %d columns %d:" % (d, n - 8), t.narrow(d, n - 8, 8)


def _errors(got, ref, spec, B, H):
    """label -> max |got - ref| / max(|ref|, 1e-3) of every view."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    out = {}
    for (label, a), (_, b) in zip(_views(got, spec, B, H), _views(ref, spec, B, H)):
        out[label] = (a - b).abs().max().item() / max(b.abs().max().item(), 1e-3)
    return out


def _check(name, got, ref, tol, spec, B, H, worst):
    """Every view within ``tol`` (a number, or label -> number); ``worst[name]`` keeps the largest error / scale."""
    assert torch.isfinite(got).all(), name
    for label, e in _errors(got, ref, spec, B, H).items():
        worst[name] = max(worst.get(name, 0.0), e)
        bound = tol[label] if isinstance(tol, dict) else tol
        assert e <= bound, (name, label, e, bound)


def _check_products(name, got, ref, mag, K, extra, worst):
    """|got - ref| <= K 2^-23 mag (+ extra) elementwise; ``worst[name]``: the largest error in units of the bound."""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all(), name
    bound = K * 2.0 ** -23 * mag + extra
    err = (got - ref).abs()
    worst[name] = max(worst.get(name, 0.0), (err / bound.clamp_min(1e-300)).max().item())
    bad = err > bound
    assert not bad.any(), (name, int(bad.sum()), err[bad].max().item(), bound[bad].min().item())


# ---------------------------------------------------------------------------------------------------------- problems
_PROBLEMS = {}


def _frames(T0, reductions):
    Ts = []
    for r in reductions:
        Ts.append(T0)
        T0 = (T0 + r - 1) // r
    return Ts, T0


def _problem(name, drop=None):
    """Master parameters (fp32), inputs and the float64 reference of a case, built once per (name, drop): the reference
    sees what the kernels see - W_ih and W_hh rounded to bf16, x rounded where the case passes bf16 x, fp32 biases,
    LayerNorm parameters and states, dout rounded to bf16.  ``drop`` = (p, seeds) as EncoderStackFn takes it (or
    stack_ref's three-item form with wrong frame indices, for the negative controls): the same parameters and inputs,
    the reference with the masks."""
    if (name, drop) in _PROBLEMS:
        return _PROBLEMS[(name, drop)]
    B, T0, I0, H, L, red, chunk, lag, states, xdt = CASES[name][0]
    g = torch.Generator(device="cpu").manual_seed(1000 * H + 10 * B + T0)
    k = 1.0 / H ** 0.5
    u = lambda *s: (torch.rand(*s, generator=g) * 2 - 1) * k            # noqa: E731
    layers = []
    for l in range(L):
        I = I0 if l == 0 else H
        layers.append([u(4 * H, I), u(4 * H, H), u(4 * H), u(4 * H),
                       1.0 + 0.2 * torch.randn(H, generator=g), 0.2 * torch.randn(H, generator=g)])
    in_g, in_b = 1.0 + 0.2 * torch.randn(I0, generator=g), 0.2 * torch.randn(I0, generator=g)
    x = torch.randn(B, T0, I0, generator=g).to(xdt)
    h0 = 0.5 * torch.randn(L, B, H, generator=g) if states else None
    c0 = 0.5 * torch.randn(L, B, H, generator=g) if states else None
    Ts, T_out = _frames(T0, red)
    dout = torch.randn(B, T_out, H, generator=g).to(BF16)
    seen = [[lay[0].to(BF16), lay[1].to(BF16)] + lay[2:] for lay in layers]
    ref = S.stack_forward64(x, in_g, in_b, seen, red, h0, c0, drop)
    grads = S.stack_grads64(ref, dout, drop)
    p = dict(layers=layers, seen=seen, in_g=in_g, in_b=in_b, x=x, h0=h0, c0=c0, dout=dout, Ts=Ts, T_out=T_out,
             ref=ref, grads=grads, yard=None)
    _PROBLEMS[(name, drop)] = p
    return p


def _ref_tensors(p):
    """name -> (float64 reference, spec) of everything the end-to-end backward comparison covers."""
    out = {"d_in_gamma": (p["grads"]["in_gamma"], "i"), "d_in_beta": (p["grads"]["in_beta"], "i")}
    for l, gl in enumerate(p["grads"]["layers"]):
        for n, t, spec in zip(("dW_ih", "dW_hh", "db_ih", "db_hh", "dln_gamma", "dln_beta"), gl,
                              ("ui" if l == 0 else "uu", "uu", "u", "u", "u", "u")):
            out["%s[%d]" % (n, l)] = (t, spec)
    return out


def _yardstick(name, drop=None):
    """(``drop`` = (p, dropout_ref.seeds(DROP_SEED, 1, L)): the per-layer path in training mode draws exactly these
    seeds, one per layer in layer order, under torch.manual_seed(DROP_SEED) with its call counter at 0.)
    Errors of the per-layer bf16 path (config.USE_ENCODER_STACK off, the same weights, no projection) against the same
    float64 reference, per parameter gradient, per layer's dG and view: label -> error / scale.  Once per case.  The dG
    of a layer is the G buffer its autograd node holds (_LSTMBlockFn: ctx.inter[0], [B, T, 4H] in plain gate order), which
    its backward turns into dG in place; the nodes are found by walking the graph down from the output."""
    from edgedict_amd import config
    from edgedict_amd import models
    from edgedict_amd.models import Encoder
    p = _problem(name, drop)
    if p["yard"] is not None:
        return p["yard"]
    B, T0, I0, H, L, red, chunk, lag, states, xdt = CASES[name][0]
    assert drop is None or tuple(drop[1]) == tuple(D.seeds(DROP_SEED, 1, L))
    enc = Encoder(input_size=I0, hidden_size=H, num_layers=L, dropout=0.0 if drop is None else drop[0], proj_size=8,
                  time_reductions=[l for l, r in enumerate(red) if r == 2], has_proj=False).cuda()
    mine = [enc.norm.weight, enc.norm.bias]
    src = [p["in_g"], p["in_b"]]
    for l in range(L):
        mine += list(enc.lstm.lstms[l].layer(0)) + [enc.lstm.projs[l][0].weight, enc.lstm.projs[l][0].bias]
        src += p["layers"][l]
    with torch.no_grad():
        for a, b in zip(mine, src):
            assert a.shape == b.shape
            a.copy_(b)
    enc.compute_dtype = BF16
    old = config.USE_ENCODER_STACK, models._dropout_calls[0], torch.random.get_rng_state()
    config.USE_ENCODER_STACK = False
    try:
        hid = (p["h0"].cuda(), p["c0"].cuda()) if states else None
        if drop is not None:
            torch.manual_seed(DROP_SEED)
            models._dropout_calls[0] = 0
        out, _ = enc(p["x"].cuda(), hid)
        assert drop is None or models._dropout_calls[0] == L
        assert out.shape == p["dout"].shape
        Gs, node = [], out.grad_fn
        while node is not None:                  # the last layer's node first; input 0 of every node is its x
            if hasattr(node, "inter"):
                Gs.append(node.inter[0])
            node = node.next_functions[0][0] if node.next_functions else None
        Gs.reverse()
        assert len(Gs) == L and all(G.shape == (B, T, 4 * H) for G, T in zip(Gs, p["Ts"]))
        out.backward(p["dout"].cuda().to(out.dtype))
        torch.cuda.synchronize()
    finally:
        config.USE_ENCODER_STACK, models._dropout_calls[0] = old[:2]
        torch.random.set_rng_state(old[2])
    refs = _ref_tensors(p)
    names = ["d_in_gamma", "d_in_beta"]
    for l in range(L):
        names += ["%s[%d]" % (n, l) for n in ("dW_ih", "dW_hh", "db_ih", "db_hh", "dln_gamma", "dln_beta")]
    p["yard"] = {n: _errors(q.grad, refs[n][0], refs[n][1], B, H) for n, q in zip(names, mine)}
    for l in range(L):
        p["yard"]["dG[%d]" % l] = _errors(Gs[l], p["grads"]["dG"][l], "btu", B, H)
    return p["yard"]


# --------------------------------------------------------------------------------------------------------------- run
class _Knobs:
    """config.STACK_MIN_FRAMES = 1 and the module knobs CHUNK, LAG, SPLIT_K = 1, FLAGS = 0 (and, on request,
    config.DEFER_WEIGHT_GRADS), put back on exit - tests/test_encoder_stack_gpu._run's."""

    def __init__(self, chunk, lag, defer=None):
        self.chunk, self.lag, self.defer = chunk, lag, defer

    def __enter__(self):
        from edgedict_amd import config, encoder_stack as es
        self.old = (config.STACK_MIN_FRAMES, config.DEFER_WEIGHT_GRADS, es.CHUNK, es.LAG, es.SPLIT_K, es.FLAGS)
        config.STACK_MIN_FRAMES = 1
        if self.defer is not None:
            config.DEFER_WEIGHT_GRADS = self.defer
        es.CHUNK, es.LAG, es.SPLIT_K, es.FLAGS = self.chunk, self.lag, 1, 0

    def __exit__(self, *exc):
        from edgedict_amd import config, encoder_stack as es
        config.STACK_MIN_FRAMES, config.DEFER_WEIGHT_GRADS, es.CHUNK, es.LAG, es.SPLIT_K, es.FLAGS = self.old


def _select_route(monkeypatch, name, fk, bk):
    """A case that lists both kinds of a direction gets the one asked for; one that lists kind 0 alone asks for the
    persistent kernel, which its geometry must decline."""
    _, fks, bks = CASES[name]
    monkeypatch.setenv("EDGEDICT_STACK_LPW", "1" if (fk == 1 or len(fks) == 1) else "0")
    monkeypatch.setenv("EDGEDICT_STACK_BWD_SK", "1" if (bk == 2 or len(bks) == 1) else "0")
    monkeypatch.setenv("EDGEDICT_STACK_POISON", "1")       # a read that overtakes its producer sees NaN


def _device_operands(p):
    dev = [t.cuda().requires_grad_(True) for t in [p["in_g"], p["in_b"]] + [q for lay in p["layers"] for q in lay]]
    x = p["x"].cuda().requires_grad_(True)
    h0 = None if p["h0"] is None else p["h0"].cuda()
    c0 = None if p["c0"] is None else p["c0"].cuda()
    return dev, x, h0, c0


def _forward(name, p, dev, x, h0, c0, fk, worst, drop=None):
    """The forward pass and every forward check; returns (out, plan, per-layer kernel buffers as float64 CPU tensors).
    With ``drop`` = (p, seeds) the pass runs under dropout and every layer's X_next (the stored X_{l+1}, ``out`` for the
    last layer) is held to the mask (``_check_dropped``) instead of to the plain norm role."""
    from edgedict_amd import encoder_stack as es
    B, T0, I0, H, L, red, chunk, lag, states, xdt = CASES[name][0]
    out, hN, cN = es.EncoderStackFn.apply(x, dev[0], dev[1], h0, c0, tuple(red), None, drop, *dev[2:])
    torch.cuda.synchronize()
    es.check_wsr_error()
    assert es.last_mode(False)[0] == fk, ("forward kind", es.last_mode(False), fk)
    plan = out.grad_fn.plan
    assert out.dtype == BF16 and out.shape == (B, p["T_out"], H) and hN.shape == cN.shape == (L, B, H)
    cpu = lambda t: t.detach().double().cpu()           # noqa: E731
    # ---- input LayerNorm: statistics of x [B T0] (batch-first rows), X_0 [T0, B, I0]
    x64 = p["x"].double()
    mean, rstd = S.ln_stats(x64)
    _check("in_mean", cpu(plan.in_mean).view(B, T0), mean, STAT_TOL, "bt", B, H, worst)
    _check("in_rstd", cpu(plan.in_rstd).view(B, T0), rstd, STAT_TOL, "bt", B, H, worst)
    _check("X_0", S.batch_first(cpu(plan.layer_bufs[0]["X"])), M.layer_norm(x64, p["in_g"].double(), p["in_b"].double()),
           BF16_ULP, "bti", B, H, worst)
    kept = []
    for l in range(L):
        bufs = plan.layer_bufs[l]
        T = p["Ts"][l]
        assert bufs["X"].shape == (T, B, I0 if l == 0 else H) and bufs["Yx"].shape == (T + 1, B, H)
        Xk, Yx, Cx = S.batch_first(cpu(bufs["X"])), cpu(bufs["Yx"]), cpu(bufs["Cx"])
        gates = S.plain_gates(cpu(bufs["G"]), H)          # (a copy: the backward pass writes dG over the buffer)
        # frame 0 of the h / c images: bf16(h0) and c0 exactly, or zeros
        if states:
            assert torch.equal(bufs["Yx"][0].cpu(), p["h0"][l].to(BF16)) and torch.equal(bufs["Cx"][0].cpu(), p["c0"][l])
        else:
            assert not bufs["Yx"][0].any() and not bufs["Cx"][0].any()
        # ---- the layer on the kernel's own input and initial frames
        want = S.layer_forward64(Xk, p["seen"][l], red[l], l > 0, Yx[0], Cx[0])
        Yk, Ck = S.batch_first(Yx[1:]), S.batch_first(Cx[1:])
        _check("gates", gates, want.gates, OUT_TOL, "btu", B, H, worst)
        _check("Yx", Yk, want.Y, OUT_TOL, "btu", B, H, worst)
        _check("Cx", Ck, want.C, OUT_TOL, "btu", B, H, worst)
        _check("hN", hN[l], want.hN, OUT_TOL, "bu", B, H, worst)
        _check("cN", cN[l], want.cN, OUT_TOL, "bu", B, H, worst)
        # ---- LayerNorm of the kernel's own rows: statistics, then the next layer's input (or the output)
        Zk = Xk + Yk if l > 0 else Yk
        mean, rstd = S.ln_stats(Zk)
        _check("mean", S.batch_first(cpu(bufs["mean"])), mean, STAT_TOL, "bt", B, H, worst)
        _check("rstd", S.batch_first(cpu(bufs["rstd"])), rstd, STAT_TOL, "bt", B, H, worst)
        nxt = S.norm_role(Zk, p["layers"][l][4].double(), p["layers"][l][5].double(), red[l])
        got = cpu(out) if l == L - 1 else S.batch_first(cpu(plan.layer_bufs[l + 1]["X"]))
        if drop is None:
            _check("X_next", got, nxt, BF16_ULP, "btu", B, H, worst)
        else:
            _check_dropped(got, nxt, drop[0], drop[1][l], B, H, worst)
        kept.append(dict(X=Xk, Hprev=S.batch_first(Yx[:-1]), Z=Zk, X_next=got))
    return out, plan, kept


def _check_dropped(got, ln64, p, seed, B, H, worst):
    """A layer's output under dropout against the float64 LayerNorm (+ pair mean) ``ln64`` of the kernel's own rows:
    exact zeros wherever dropout_ref.mask drops; non-zero wherever it keeps and the float64 value is not within one
    bf16 ulp of zero (on the buffer's scale: 2^-8 max |ln64|); the kept values within 2 BF16_ULP of scale * ln64 on
    the relative-to-max metric of every view - two bf16 roundings, derived: the kernel rounds the LayerNorm to bf16 (one
    relative 2^-8), multiplies by the fp32 scale in fp32 and rounds again at its store (another)."""
    keep = torch.from_numpy(D.mask(tuple(ln64.shape), p, seed))
    assert not got[~keep].any(), "a dropped element is not zero"
    sure = keep & (ln64.abs() > BF16_ULP * ln64.abs().max())
    assert sure.float().mean().item() > 0.5 * (1 - p) and (got[sure] != 0).all(), "a kept element is zero"
    _check("X_next", got, ln64 * keep * float(D.scale(p)), 2 * BF16_ULP, "btu", B, H, worst)


def _line(tag, worst):
    print("%s: %s" % (tag, ", ".join("%s %.2e" % kv for kv in sorted(worst.items()))))


def _check_backward(name, p, yard, dev, plan, kept, tag):
    """The checks behind the backward pass: every layer's weight-gradient products from the kernel's own buffers, then
    dG of every layer and every parameter gradient end to end against ``p``'s float64 gradients (``kept[l]["dG"]`` is
    left holding the kernel's dG in plain gate order)."""
    B, T0, I0, H, L, red, chunk, lag, states, xdt = CASES[name][0]
    grads = {"d_in_gamma": dev[0].grad, "d_in_beta": dev[1].grad}
    for l in range(L):
        for n, q in zip(("dW_ih", "dW_hh", "db_ih", "db_hh", "dln_gamma", "dln_beta"), dev[2 + 6 * l:8 + 6 * l]):
            grads["%s[%d]" % (n, l)] = q.grad
    # ---- weight-gradient products of every layer from the kernel's own buffers
    worst = {}
    for l in range(L):
        dG = S.plain_gates(plan.layer_bufs[l]["G"].detach().double().cpu(), H)
        (dw_ih, dw_hh, db), (m_ih, m_hh, m_b) = S.weight_grads_from_buffers(dG, kept[l]["X"], kept[l]["Hprev"])
        K = p["Ts"][l] * B
        _check_products("dW_ih", grads["dW_ih[%d]" % l], dw_ih, m_ih, K, 0.0, worst)
        _check_products("dW_hh", grads["dW_hh[%d]" % l], dw_hh, m_hh, K, 0.0, worst)
        _check_products("db_ih", grads["db_ih[%d]" % l], db, m_b, K, 0.0, worst)
        _check_products("db_hh", grads["db_hh[%d]" % l], db, m_b, K, 0.0, worst)
        kept[l]["dG"] = dG
    _line(tag + " products (error / bound)", worst)
    # ---- backward end to end
    worst = {}
    for l in range(L):
        tol = GRAD_TOL
        if L > 1:
            tol = {label: min(DEEP_CAP, 2.0 * e + DEEP_SLACK) for label, e in yard["dG[%d]" % l].items()}
        _check("dG", kept[l]["dG"], p["grads"]["dG"][l], tol, "btu", B, H, worst)
    for n, (ref, spec) in _ref_tensors(p).items():
        tol = GRAD_TOL
        if L > 1:
            tol = {label: min(DEEP_CAP, 2.0 * e + DEEP_SLACK) for label, e in yard[n].items()}
        _check(n.split("[")[0], grads[n], ref, tol, spec, B, H, worst)
    _line(tag + " backward", worst)


@pytest.mark.parametrize("name,fk,bk", RUNS, ids=["%s-fwd%d-bwd%d" % r for r in RUNS])
def test_stack_kernels_match_fp64_buffer_by_buffer(hip_lib, monkeypatch, name, fk, bk):
    """Every case of CASES on every recurrence route it lists (see the module docstring for what is compared and on
    which scale).

    Largest error / max(|ref|, 1e-3) measured on an MI355X over all cases and views, per route (print with -s):
      forward kind 0 (a launch per step): gates 4.8e-3, Yx 5.2e-3, Cx 2.7e-3, hN 4.9e-3, cN 2.6e-3 (bound 2e-2); X_0 3.3e-3,
        X_next 3.5e-3 (bound 3.9e-3 = 2^-8); in_mean 1.5e-7, in_rstd 1.1e-7, mean 9.1e-8, rstd 1.1e-7 (bound 1e-5)
      forward kind 1 (launch-persistent): gates 4.8e-3, Yx 4.5e-3, Cx 2.4e-3, hN 4.5e-3, cN 2.1e-3; the norms as above (the
        same kernels on bit-identical rows)
      weight-gradient products, largest error in units of the derived bound K 2^-23 |dG|^T |X|: backward kind 0 dW_ih
        0.18, dW_hh 0.19, db 0.034 (case i, K = 6 terms); backward kind 2 dW_ih 0.028, dW_hh 0.019, db 0.004
      backward end to end, one layer (bound 4e-2): kind 0 dG 8.1e-3, dW_ih 5.7e-3, dW_hh 9.2e-3, db 4.9e-3, dln_gamma
        3.9e-3, dln_beta 1.7e-9, d_in_gamma 7.2e-3, d_in_beta 4.4e-3; kind 2 dG 8.1e-3, dW_ih 3.0e-3, dW_hh 7.7e-3, db
        4.1e-3, dln_gamma 2.2e-3, d_in_gamma 4.2e-3, d_in_beta 1.9e-3
      backward end to end, two and three layers (bound 2 x per-layer path + 2e-2, at most 6e-2), both kinds: dG 1.3e-2,
        dW_ih 6.4e-3, dW_hh 6.9e-3, db 6.0e-3, dln_gamma 8.0e-3, dln_beta 3.7e-3, d_in_gamma 9.7e-3, d_in_beta 4.4e-3
    - bf16 rounding at the kernels' stores and nothing on top."""
    from edgedict_amd import encoder_stack as es
    B, T0, I0, H, L, red, chunk, lag, states, xdt = CASES[name][0]
    assert es.supported(BF16, H, I0, L, red)
    p = _problem(name)
    yard = _yardstick(name) if L > 1 else None
    _select_route(monkeypatch, name, fk, bk)
    tag = "\nstack %s fwd %d bwd %d" % (name, fk, bk)
    with _Knobs(chunk, lag):
        dev, x, h0, c0 = _device_operands(p)
        worst = {}
        out, plan, kept = _forward(name, p, dev, x, h0, c0, fk, worst)
        _line(tag + " forward", worst)
        out.backward(p["dout"].cuda())
        torch.cuda.synchronize()
        es.check_wsr_error()
        assert es.last_mode(True)[0] == bk, ("backward kind", es.last_mode(True), bk)
    assert x.grad is None                                # the Function returns no gradient for xs
    _check_backward(name, p, yard, dev, plan, kept, tag)


# ----------------------------------------------------------------------------------------------------------- dropout
# b: odd T under a reduction, the lone last frame, drop_T = 3; c: a residual layer, the reduction in the last layer,
# B = 33; e: three layers, both backward kinds; f: two reductions, non-zero lag, several chunks (the frame mapping of
# the chunk-wise LayerNorm backward); g: H = 544, the second 512-column pass with 32 live columns in both norm kernels
DROP_CASES = ("b", "c", "e", "f", "g")
DROP_RUNS = [r for r in RUNS if r[0] in DROP_CASES]


def _drop_of(name):
    """(p, seeds) of a case: the seeds its per-layer yardstick draws (``_yardstick``)."""
    return (DROP_P, tuple(D.seeds(DROP_SEED, 1, CASES[name][0][4])))


def _wrong_masks(name):
    """Negative controls of a two-layer case: label -> (stack_ref's drop with a deliberately wrong mask, the layers whose
    mask is wrong).  ``shift``: the frame index off by one in the first time-reduced layer; ``swap``: the seeds of the
    two layers exchanged."""
    L, red = CASES[name][0][4:6]
    assert L == 2
    p, seeds = _drop_of(name)
    l = red.index(2)
    return {"shift": ((p, seeds, tuple(int(k == l) for k in range(L))), [l]),
            "swap": ((p, (seeds[1], seeds[0])), [0, 1])}


@pytest.mark.parametrize("name,fk,bk", DROP_RUNS, ids=["%s-fwd%d-bwd%d" % r for r in DROP_RUNS])
def test_stack_kernels_under_dropout_match_fp64_under_the_same_masks(hip_lib, monkeypatch, name, fk, bk):
    """``EncoderStackFn.apply(..., (p, seeds), ...)`` at p = 0.3 on every route of the cases b, c, e, f, g, against the
    float64 restatement with the masks of tests/dropout_ref.py (index (b T_out_l + tau) H + j over every layer's reduced
    output, one seed per layer).

    Every forward buffer check of the dropout-free test in the same form, each layer fed the kernel's own stored X_l -
    which now carries the mask; X_{l+1} of EVERY layer and ``out``: exact zeros exactly where the mask drops, kept values
    within 2 BF16_ULP of scale * LayerNorm64 (two bf16 roundings: before the mask, and at the store of the scaled value);
    the weight-gradient products at K 2^-23; dG of every layer and every parameter gradient end to end at GRAD_TOL (one
    layer) or min(6e-2, 2 x per-layer path + 2e-2), the per-layer bf16 path run with the SAME seeds (pinned layer by layer
    in tests/test_dropout_gpu.py); the same seeds twice give a bit-identical ``out``.

    Power (cases c and f, on the CPU, no kernel changed): against a reference whose mask is wrong in the ways this test
    is about - the frame index off by one in the reduced layer (it flips about 43 % of the mask bits at p = 0.3), the
    two layers' seeds exchanged - the same X_next and end-to-end dG comparisons of the affected layers FAIL their
    bounds.

    Largest error / max(|ref|, 1e-3) measured on an MI355X over these cases and routes (print with -s; the routes of a
    case agree to the digits shown):
      forward: gates 4.4e-3, Yx 3.8e-3, Cx 2.0e-3, hN 4.1e-3, cN 1.9e-3 (bound 2e-2); X_0 3.3e-3 (bound 2^-8); X_next 5.3e-3
        (bound 7.8e-3 = 2 x 2^-8; zero patterns equal to the mask everywhere); statistics <= 1.5e-7 (bound 1e-5)
      weight-gradient products: at most 0.075 of the derived bound (dW_hh, case g)
      backward end to end, one layer (b, g; bound 4e-2): dG 7.5e-3, dW_ih 4.7e-3, dW_hh 6.9e-3, db 6.3e-3, dln_gamma 4.1e-3,
        dln_beta 1.8e-7, d_in_gamma 6.7e-3, d_in_beta 4.6e-3
      backward end to end, two and three layers (c, e, f): dG 1.2e-2, dW_ih 1.1e-2, dW_hh 1.3e-2, db 1.5e-2, dln_gamma
        5.0e-3, dln_beta 4.0e-3, d_in_gamma 7.2e-3, d_in_beta 6.3e-3
      against the wrong masks: X_next 0.88 ... 1.08 (bound 7.8e-3), dG 0.82 ... 1.44 (bound at most 6e-2)
    - the figures of the dropout-free test: the masks are the reference's, bit for bit."""
    from edgedict_amd import encoder_stack as es
    B, T0, I0, H, L, red, chunk, lag, states, xdt = CASES[name][0]
    assert es.supported(BF16, H, I0, L, red)
    drop = _drop_of(name)
    p = _problem(name, drop)
    yard = _yardstick(name, drop) if L > 1 else None
    _select_route(monkeypatch, name, fk, bk)
    tag = "\nstack %s fwd %d bwd %d dropout %.1f" % (name, fk, bk, DROP_P)
    with _Knobs(chunk, lag):
        dev, x, h0, c0 = _device_operands(p)
        worst = {}
        out, plan, kept = _forward(name, p, dev, x, h0, c0, fk, worst, drop)
        _line(tag + " forward", worst)
        out.backward(p["dout"].cuda())
        torch.cuda.synchronize()
        es.check_wsr_error()
        assert es.last_mode(True)[0] == bk, ("backward kind", es.last_mode(True), bk)
        # ---- determinism: the same seeds again
        dev2, x2, h02, c02 = _device_operands(p)
        again = es.EncoderStackFn.apply(x2, dev2[0], dev2[1], h02, c02, tuple(red), None, drop, *dev2[2:])[0]
        torch.cuda.synchronize()
        es.check_wsr_error()
        assert torch.equal(again, out)
        del again, dev2, x2
    assert x.grad is None
    _check_backward(name, p, yard, dev, plan, kept, tag)
    if name not in ("c", "f"):
        return
    # ---- negative controls: the bounds above see a wrong mask
    seen = {}
    for kind, (wrong, layers) in _wrong_masks(name).items():
        q = _problem(name, wrong)
        for l in layers:
            nxt = S.norm_role(kept[l]["Z"], p["layers"][l][4].double(), p["layers"][l][5].double(), red[l],
                              S.layer_drop(wrong, l))
            e_x = _errors(kept[l]["X_next"], nxt, "btu", B, H)["all"]
            e_g = _errors(kept[l]["dG"], q["grads"]["dG"][l], "btu", B, H)["all"]
            tol = min(DEEP_CAP, 2.0 * yard["dG[%d]" % l]["all"] + DEEP_SLACK)
            seen["%s X_next[%d]" % (kind, l)], seen["%s dG[%d]" % (kind, l)] = e_x, e_g
            assert e_x > 2 * BF16_ULP, (kind, l, "X_next passes against a wrong mask", e_x)
            assert e_g > tol, (kind, l, "dG passes against a wrong mask", e_g, tol)
    _line(tag + " wrong masks (must exceed 7.8e-3 / 6e-2)", seen)


def test_in_place_gradient_path_accumulates_the_same_gradients(hip_lib, monkeypatch):
    """The trainer's path (ACCUM_GRADS in _Plan.backward): every parameter has a contiguous fp32 .grad and
    config.DEFER_WEIGHT_GRADS is on, so the pass adds into those buffers and returns nothing.  Case e with the buffers
    pre-filled with a known pattern: .grad - pattern meets the bounds of the returned gradients (the products with one
    more fp32 rounding of the accumulated value, 2^-23 (|pattern| + |gradient|)), in the SAME buffers, and b_ih.grad and
    b_hh.grad - written through two pointers - moved by the same db.

    Measured on an MI355X: products 7.1e-3 (dW_hh), 5.8e-3 (dW_ih), 9.2e-4 (db) of their elementwise bound; end to end
    dW_ih 6.4e-3, dW_hh 6.9e-3, db 6.0e-3, dln_gamma 8.0e-3, dln_beta 3.7e-3, d_in_gamma 9.7e-3, d_in_beta 4.4e-3;
    b_ih.grad and b_hh.grad bit-identical."""
    from edgedict_amd import encoder_stack as es
    name, fk, bk = "e", 1, 2
    B, T0, I0, H, L, red, chunk, lag, states, xdt = CASES[name][0]
    p = _problem(name)
    yard = _yardstick(name)
    _select_route(monkeypatch, name, fk, bk)
    with _Knobs(chunk, lag, defer=True):
        dev, x, h0, c0 = _device_operands(p)
        pats = []
        for q in dev:
            i = torch.arange(q.numel(), device="cuda").view(q.shape)
            pats.append(0.5 + 0.125 * ((i % 5) - 2).float())          # 0.25 ... 0.75, exact in fp32
            q.grad = pats[-1].clone()
        ptrs = [q.grad.data_ptr() for q in dev]
        worst = {}
        out, plan, kept = _forward(name, p, dev, x, h0, c0, fk, worst)
        out.backward(p["dout"].cuda())
        torch.cuda.synchronize()
        es.check_wsr_error()
        assert es.last_mode(True)[0] == bk
    assert plan.desc.flags & es.ACCUM_GRADS             # the in-place path ran: the Function returned nothing to add
    assert x.grad is None
    assert [q.grad.data_ptr() for q in dev] == ptrs and all(q.grad.dtype == F32 for q in dev)
    delta = [q.grad.double().cpu() - pat.double().cpu() for q, pat in zip(dev, pats)]
    names = ["d_in_gamma", "d_in_beta"]
    for l in range(L):
        names += ["%s[%d]" % (n, l) for n in ("dW_ih", "dW_hh", "db_ih", "db_hh", "dln_gamma", "dln_beta")]
    got = dict(zip(names, delta))
    pat = dict(zip(names, [t.double().cpu() for t in pats]))
    worst = {}
    for l in range(L):
        dG = S.plain_gates(plan.layer_bufs[l]["G"].detach().double().cpu(), H)
        (dw_ih, dw_hh, db), (m_ih, m_hh, m_b) = S.weight_grads_from_buffers(dG, kept[l]["X"], kept[l]["Hprev"])
        K = p["Ts"][l] * B
        for n, ref, mag in (("dW_ih", dw_ih, m_ih), ("dW_hh", dw_hh, m_hh), ("db_ih", db, m_b), ("db_hh", db, m_b)):
            key = "%s[%d]" % (n, l)
            _check_products(n, got[key], ref, mag, K, 2.0 ** -23 * (pat[key].abs() + ref.abs()), worst)
        # both bias buffers started from the same pattern and got the same db through two pointers: each is one fp32
        # rounding of pattern + db away from it, so the two deltas differ by at most 2^-23 (|pattern| + |db|)
        d_ih, d_hh = got["db_ih[%d]" % l], got["db_hh[%d]" % l]
        assert torch.equal(pat["db_ih[%d]" % l], pat["db_hh[%d]" % l])
        assert ((d_ih - d_hh).abs() <= 2.0 ** -23 * (pat["db_ih[%d]" % l].abs() + db.abs())).all(), l
        worst["db_ih - db_hh (abs)"] = max(worst.get("db_ih - db_hh (abs)", 0.0), (d_ih - d_hh).abs().max().item())
    _line("\nstack e in-place products (error / bound)", worst)
    worst = {}
    for n, (ref, spec) in _ref_tensors(p).items():
        tol = {label: min(DEEP_CAP, 2.0 * e + DEEP_SLACK) for label, e in yard[n].items()}
        _check(n.split("[")[0], got[n], ref, tol, spec, B, H, worst)
    _line("stack e in-place backward", worst)
