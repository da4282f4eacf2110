"""GPU: every per-layer dropout path against float64 UNDER THE IDENTICAL MASK.

The mask is a stateless hash of (seed, contiguous element index) (csrc/common.hpp), restated in numpy by
tests/dropout_ref.py and pinned on the host by tests/test_dropout_ref_host.py.  Here:

  the elementwise kernel   ``ops.dropout`` (csrc/elementwise.hip): the zero pattern equals the restated mask exactly, in
                           fp32 and bf16, through the grid-stride loop (several passes, the last one partial), at
                           p = 0 and at both ends of the seed range; dropped elements are +0 whatever x was (the
                           select, not a multiply by zero), kept ones the fp32 product x * (1.f / (1.f - p)) bit for
                           bit (bf16: its round-to-nearest-even); in place; a non-contiguous x over its contiguous order
  ``_DropoutFn``           a non-contiguous dy: x.grad = mask * scale * dy, the same bit-exact rule
  the per-layer paths      ``ResLayerNormLSTM`` / ``ResLayerNormGRU`` (config.USE_ENCODER_STACK off, a reduction in layer
                           1 under an odd T, so that layer 1's mask indexes the reduced tensor), ``Decoder`` (dropout
                           behind layer 0 only), ``LMModel`` (embedding and every LSTM layer) and one ``Transducer``:
                           output, final states, loss and EVERY parameter gradient against a float64 restatement from
                           ``oracle.models_ref`` pieces times ``mask * scale``, the masks built from the seeds the
                           product will draw (``dropout_ref.seeds`` under torch.manual_seed, call counter 0), at the
                           bounds the same paths meet without dropout

The bf16 encoder stack under dropout is in tests/test_stack_kernels_gpu.py.

NOT covered: the ``i >> 32`` term of the element index - it needs more than 2^32 elements; ``dropout_ref`` implements
it (and its host test pins it), no device test reaches it.
"""
import contextlib
import functools

import numpy as np
import pytest
import torch

import dropout_ref as D
from oracle import models_ref as M

pytestmark = pytest.mark.gpu

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
# one layer: test_lstm_gpu.OUT_TOL / GRAD_TOL and test_gru_gpu.OUT_TOL / GRAD_TOL
LSTM_TOL = {F32: (2e-4, 2e-4), BF16: (2e-2, 4e-2)}
GRU_TOL = {F32: (1e-4, 1e-4), BF16: (2e-2, 4e-2)}
DEEP_CAP, DEEP_SLACK = 6e-2, 2e-2      # test_stack_kernels_gpu: more than one bf16 layer, min(cap, 2 x one layer + slack)


def _tols(one_layer, cd):
    out, grad = one_layer[cd]
    if cd == BF16:
        return min(DEEP_CAP, 2 * out + DEEP_SLACK), min(DEEP_CAP, 2 * grad + DEEP_SLACK)
    return out, grad


def _close(name, got, ref, tol, worst):
    """max |got - ref| <= tol max(|ref|, 1e-3) (test_gru_gpu._close); ``worst[name]`` keeps the largest error / scale."""
    ref = ref.detach().double().cpu()
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (name, tuple(got.shape), tuple(ref.shape))
    assert torch.isfinite(got).all(), name
    err = (got - ref).abs().max().item()
    scale = max(ref.abs().max().item(), 1e-3)
    key = name.split("[")[0]
    worst[key] = max(worst.get(key, 0.0), err / scale)
    assert err <= tol * scale, (name, err, scale, tol)


def _line(tag, worst):
    print("\n%s: %s" % (tag, ", ".join("%s %.2e" % kv for kv in sorted(worst.items()))))


def _mask64(shape, p, seed):
    """mask * scale of a contiguous tensor of ``shape`` as float64 (the scale is the kernels' float32 one)."""
    return torch.from_numpy(D.mask(tuple(shape), p, seed).astype(np.float64) * float(D.scale(p)))


@contextlib.contextmanager
def _seeded(seed):
    """torch.manual_seed(seed) and the call counter of models._next_dropout_seed at 0; both put back on exit."""
    from edgedict_amd import models
    old, state = models._dropout_calls[0], torch.random.get_rng_state()
    torch.manual_seed(seed)
    models._dropout_calls[0] = 0
    try:
        yield models._dropout_calls
    finally:
        models._dropout_calls[0] = old
        torch.random.set_rng_state(state)


# ------------------------------------------------------------------------------------------- the elementwise kernel
PS = (0.0, 0.1, 0.5, 0.9)
SEEDS = (0, 0xFFFFFFFF, D.seeds(3, 1, 1)[0])
SIZES = (1, 255, 1025, 4096 * 256 + 257)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_mask_of_the_kernel_is_the_restated_mask(hip_lib, dtype, n):
    """``ops.dropout(ones) != 0`` equals ``dropout_ref.mask`` exactly, for every p and seed.  The launch is a
    grid-stride loop of min(ceil(n / 1024), 4096) blocks of 256 threads: n = 4096 * 256 + 257 takes four passes, the
    last one partial.  Measured on an MI355X: equal everywhere (the host literals of test_dropout_ref_host hold on
    the device)."""
    from edgedict_amd import ops
    ones = torch.ones(n, dtype=dtype, device="cuda")
    for p in PS:
        for seed in SEEDS:
            got = (ops.dropout(ones, p, seed) != 0).cpu().numpy()
            want = D.mask((n,), p, seed)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (p, hex(seed), bad.size, bad[:8])
    if n >= 32:
        bits = lambda p, s: "".join(str(int(v)) for v in (ops.dropout(ones[:32], p, s) != 0).cpu())   # noqa: E731
        assert bits(0.5, 1234) == "00001010101101100111000010111000"
        assert bits(0.1, 0x85EBCA6B) == "10111101111111111101111111111110"


def _values(dtype, shape=(37, 29)):
    """Random x with every special value planted several times: +-0, +-inf, NaN, the largest finite value."""
    g = torch.Generator(device="cpu").manual_seed(5)
    x = (4.0 * torch.randn(*shape, generator=g)).to(dtype)
    flat = x.view(-1)
    specials = [0.0, -0.0, float("inf"), float("-inf"), float("nan"), torch.finfo(dtype).max, -1.0, 1.0]
    for k in range(15 * len(specials)):
        flat[(k * 7) % flat.numel()] = specials[k % len(specials)]
    return x


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def _expect(x, p, seed):
    """What the kernel must write for a contiguous CPU tensor x: +0 where the mask drops, else the fp32 product
    float32(x) * scale(p) (IEEE single multiply on the host), rounded to nearest even for a bf16 store."""
    keep = torch.from_numpy(D.mask(tuple(x.shape), p, seed))
    prod = (x.float() * torch.tensor(float(D.scale(p)), dtype=F32)).to(x.dtype)
    return torch.where(keep, prod, torch.zeros_like(prod)), keep


def _assert_bit_equal(got, want, what):
    got, want = got.detach().cpu(), want.detach().cpu()
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), what
    a, b = _bits(got)[~nan], _bits(want)[~nan]
    bad = a != b
    assert not bad.any(), (what, int(bad.sum()), got[~nan][bad][:4], want[~nan][bad][:4])


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_values_are_a_select_and_one_correctly_rounded_product(hip_lib, dtype):
    """Dropped positions hold +0 whatever x was there (inf, NaN and -0 included); kept ones are bit-equal to
    float32(x) * (float32(1) / (float32(1) - float32(p))) - in bf16 to its round-to-nearest-even; p = 0 returns x bit
    for bit; in place (out=x) and on a non-contiguous x (masked over its contiguous order) the same.  Measured on an
    MI355X: bit-exact in both dtypes - the device's 1.f / (1.f - p) is the correctly rounded quotient."""
    from edgedict_amd import ops
    x = _values(dtype)
    seed = D.seeds(3, 1, 2)[1]
    for p in (0.1, 0.3, 0.5, 0.9):
        want, keep = _expect(x, p, seed)
        assert keep.any() and not keep.all()
        y = ops.dropout(x.cuda(), p, seed)
        assert y.dtype == dtype and y.shape == x.shape
        dropped = _bits(y.cpu())[~keep]
        assert not dropped.any(), (p, "a dropped element is not +0")
        special = ~torch.isfinite(x) & ~keep
        assert special.any()                                   # inf and NaN do sit under dropped positions
        _assert_bit_equal(y, want, ("values", p))
        # ---- in place
        xc = x.cuda().clone()
        assert ops.dropout(xc, p, seed, out=xc).data_ptr() == xc.data_ptr()
        _assert_bit_equal(xc, want, ("in place", p))
        # ---- a transposed view: the mask runs over the contiguous order of the tensor as given
        xt = x.cuda().t()
        assert not xt.is_contiguous()
        want_t, _ = _expect(x.t().contiguous(), p, seed)
        yt = ops.dropout(xt, p, seed)
        assert yt.shape == xt.shape and yt.is_contiguous()
        _assert_bit_equal(yt, want_t, ("non-contiguous", p))
    y0 = ops.dropout(x.cuda(), 0.0, seed)
    _assert_bit_equal(y0, x, "p = 0")
    assert torch.equal(_bits(y0.cpu())[~torch.isnan(x)], _bits(x)[~torch.isnan(x)])     # -0 stays -0


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_dropout_fn_backward_masks_a_non_contiguous_gradient(hip_lib, dtype):
    """The consumer reads y.transpose(0, 1), so autograd hands _DropoutFn.backward a non-contiguous dy: x.grad is
    mask * scale * dy over x's contiguous order, by the bit-exact rule of the forward kernel."""
    from edgedict_amd.models import _DropoutFn
    g = torch.Generator(device="cpu").manual_seed(11)
    p, seed = 0.3, D.seeds(3, 1, 3)[2]
    x = torch.randn(5, 7, 16, generator=g).to(dtype)
    w = torch.randn(7, 5, 16, generator=g).to(dtype)
    xd = x.cuda().requires_grad_(True)
    y = _DropoutFn.apply(xd, p, seed)
    seen = []
    y.register_hook(lambda grad: seen.append(grad.is_contiguous()))
    (y.transpose(0, 1) * w.cuda()).sum().backward()
    assert seen == [False]
    want_y, _ = _expect(x, p, seed)
    want_dx, _ = _expect(w.transpose(0, 1).contiguous(), p, seed)
    _assert_bit_equal(y, want_y, "y")
    _assert_bit_equal(xd.grad, want_dx, "x.grad")


# ------------------------------------------------------------------------- ResLayerNormLSTM / ResLayerNormGRU
RES_P, RES_SEED = 0.3, 7
RES_B, RES_T, RES_I, RES_L, RES_RED = 17, 9, 24, 3, (1, 2, 1)


def _res_params(kind, H):
    ng = 4 if kind == "lstm" else 3
    g = torch.Generator(device="cpu").manual_seed(100 * ng + H)
    k = 1.0 / H ** 0.5
    u = lambda *s: (torch.rand(*s, generator=g) * 2 - 1) * k            # noqa: E731
    layers = []
    for l in range(RES_L):
        I = RES_I if l == 0 else H
        layers.append([u(ng * H, I), u(ng * H, H), u(ng * H), u(ng * H),
                       1.0 + 0.2 * torch.randn(H, generator=g), 0.2 * torch.randn(H, generator=g)])
    x = torch.randn(RES_B, RES_T, RES_I, generator=g)
    T_out = RES_T
    for r in RES_RED:
        T_out = (T_out + r - 1) // r
    dout = torch.randn(RES_B, T_out, H, generator=g)
    return layers, x, dout


@functools.lru_cache(maxsize=None)
def _res_reference(kind, H, cd):
    """float64 on the operands the kernels see (x and the weight matrices rounded to ``cd``, fp32 biases and LayerNorm
    parameters): per layer the recurrence, the residual for l > 0, LayerNorm, the pair mean in layer 1, then
    mask * scale over the layer's [B, T_out_l, H] output with the seed of call l + 1."""
    layers, x, dout = _res_params(kind, H)
    seeds = D.seeds(RES_SEED, 1, RES_L)
    x64 = x.to(cd).double().requires_grad_(True)
    leaves, states = [], []
    cur = x64
    for l, lay in enumerate(layers):
        W = [w.to(cd).double().requires_grad_(True) for w in lay[:2]]
        rest = [q.double().requires_grad_(True) for q in lay[2:]]
        leaves.append(W + rest)
        if kind == "lstm":
            y, h, c = M.lstm_layer(cur, W[0], W[1], rest[0], rest[1], None, None, explicit=True)
            states.append((h, c))
        else:
            y, h = M.gru_layer(cur, W[0], W[1], rest[0], rest[1], None)
            states.append((h,))
        z = M.layer_norm(y if l == 0 else cur + y, rest[2], rest[3])
        if RES_RED[l] == 2:
            z = M.time_reduction(z, 2)
        cur = z * _mask64(z.shape, RES_P, seeds[l])
    assert cur.shape == dout.shape
    cur.backward(dout.to(cd).double())
    return dict(out=cur.detach(), states=[torch.stack([s[i].detach() for s in states]) for i in range(len(states[0]))],
                dx=x64.grad, grads=[[q.grad for q in lay] for lay in leaves])


@pytest.mark.parametrize("cd", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind,H", [("lstm", 64), ("gru", 40)])
def test_res_layer_norm_stack_matches_fp64_under_the_same_masks(hip_lib, kind, H, cd):
    """Three layers in training mode at p = 0.3 on the per-layer kernels, B = 17, T = 9 (frames 9, 5, 5 behind the
    layers): the output, the final states (never dropped), dx and every parameter gradient.  Bounds: fp32 the
    one-layer OUT_TOL / GRAD_TOL of test_lstm_gpu (2e-4) and test_gru_gpu (1e-4); bf16 min(6e-2, 2 x one layer + 2e-2).

    Largest error / max(|ref|, 1e-3) measured on an MI355X (print with -s): fp32 out 2.3e-7, hN 3.0e-7, cN 1.8e-7, dx
    4.7e-7, dw_ih 5.1e-7, dw_hh 5.2e-7, db 2.5e-7, dln_w 2.0e-7, dln_b 2.1e-7; bf16 out 6.3e-3, hN 5.8e-3, cN 2.4e-3, dx
    5.3e-3, dw_ih 6.7e-3, dw_hh 9.9e-3, db 7.6e-3, dln_w 6.3e-3, dln_b 6.3e-3 - what the same paths show without
    dropout (test_lstm_gpu, test_gru_gpu): the masks cost nothing."""
    from edgedict_amd import config
    from edgedict_amd.models import ResLayerNormGRU, ResLayerNormLSTM
    layers, x, dout = _res_params(kind, H)
    ref = _res_reference(kind, H, cd)
    mod = (ResLayerNormLSTM if kind == "lstm" else ResLayerNormGRU)(
        RES_I, H, RES_L, dropout=RES_P, time_reductions=[l for l, r in enumerate(RES_RED) if r == 2])
    mine = []
    for l in range(RES_L):
        mine.append(list(mod.lstms[l].layer(0)) + [mod.projs[l][0].weight, mod.projs[l][0].bias])
        with torch.no_grad():
            for a, b in zip(mine[-1], layers[l]):
                assert a.shape == b.shape
                a.copy_(b)
    mod = mod.cuda().train()
    xin = x.to(cd).cuda().requires_grad_(True)
    old = config.USE_ENCODER_STACK
    config.USE_ENCODER_STACK = False
    try:
        with _seeded(RES_SEED) as calls:
            out, states = mod(xin, None, cd)
            assert calls[0] == RES_L                               # one seed per layer, in layer order
            out.backward(dout.to(cd).cuda())
            torch.cuda.synchronize()
    finally:
        config.USE_ENCODER_STACK = old
    states = states if kind == "lstm" else (states,)
    ot, gt = _tols(LSTM_TOL if kind == "lstm" else GRU_TOL, cd)
    worst = {}
    assert out.dtype == cd
    # the zero pattern: the last layer's mask, wherever the float64 value is not itself (nearly) zero
    keep = torch.from_numpy(D.mask(tuple(out.shape), RES_P, D.seeds(RES_SEED, 1, RES_L)[-1]))
    assert not out.cpu()[~keep].any()
    assert (out.cpu()[keep] != 0).float().mean().item() > 0.99
    _close("out", out, ref["out"], ot, worst)
    for n, got, want in zip(("hN", "cN"), states, ref["states"]):
        _close(n, got, want, ot, worst)
    _close("dx", xin.grad, ref["dx"], gt, worst)
    for l in range(RES_L):
        for n, q, r in zip(("dw_ih", "dw_hh", "db_ih", "db_hh", "dln_w", "dln_b"), mine[l], ref["grads"][l]):
            _close("%s[%d]" % (n, l), q.grad, r, gt, worst)
    _line("res %s %s p=%.1f" % (kind, "bf16" if cd == BF16 else "fp32", RES_P), worst)


# ------------------------------------------------------------------------------------------------------- Decoder
DEC_P, DEC_SEED = 0.2, 5
DEC_B, DEC_U, DEC_E, DEC_H, DEC_V, DEC_PROJ = 3, 6, 16, 32, 50, 24


def _dec_params():
    g = torch.Generator(device="cpu").manual_seed(77)
    k = 1.0 / DEC_H ** 0.5
    u = lambda *s: (torch.rand(*s, generator=g) * 2 - 1) * k            # noqa: E731
    sd = {"embed.weight": torch.randn(DEC_V, DEC_E, generator=g)}
    sd["embed.weight"][M.PAD] = 0
    for l in range(2):
        I = DEC_E if l == 0 else DEC_H
        sd.update({"lstm.weight_ih_l%d" % l: u(4 * DEC_H, I), "lstm.weight_hh_l%d" % l: u(4 * DEC_H, DEC_H),
                   "lstm.bias_ih_l%d" % l: u(4 * DEC_H), "lstm.bias_hh_l%d" % l: u(4 * DEC_H)})
    sd["proj.weight"], sd["proj.bias"] = u(DEC_PROJ, DEC_H), u(DEC_PROJ)
    ys = torch.randint(4, DEC_V, (DEC_B, DEC_U), generator=g, dtype=torch.int32)
    dout = torch.randn(DEC_B, DEC_U + 1, DEC_PROJ, generator=g)
    return sd, ys, dout


def _seen(sd, cd):
    """float64 leaves of a state dict as the kernels see it: matrices rounded to ``cd``, vectors in fp32."""
    return {k: (v.to(cd) if v.dim() == 2 else v).double().requires_grad_(True) for k, v in sd.items()}


@functools.lru_cache(maxsize=None)
def _dec_reference(cd):
    sd, ys, dout = _dec_params()
    sd64 = _seen(sd, cd)
    seed = D.seeds(DEC_SEED, 1, 1)[0]

    def behind(k, x):                                  # nn.LSTM(dropout): behind every layer but the last
        return x * _mask64(x.shape, DEC_P, seed) if k == 0 else x

    y, (h, c) = M.decoder_forward({"decoder." + k: v for k, v in sd64.items()}, ys, None, explicit=True,
                                  after_layer=behind)
    y.backward(dout.to(cd).double())
    return y.detach(), h.detach(), c.detach(), {k: v.grad for k, v in sd64.items()}


@pytest.mark.parametrize("cd", [F32, BF16], ids=["fp32", "bf16"])
def test_decoder_dropout_sits_behind_layer_0_only(hip_lib, cd):
    """Decoder(2 layers, p = 0.2) in training mode: ONE seed is drawn (never behind the last layer), and the output,
    the final states and every parameter gradient match float64 with that one mask over layer 0's [B, U + 1, H]
    output.  Bounds as for the three-layer stacks above (LSTM).

    Measured on an MI355X: fp32 everything <= 3.3e-7; bf16 out 3.1e-3, hN 2.0e-3, cN 1.4e-3, d embed 7.3e-3, the LSTM
    gradients <= 6.3e-3, d proj.weight 1.7e-3, d proj.bias 0 (an fp32 sum of bf16 values)."""
    from edgedict_amd.models import Decoder
    sd, ys, dout = _dec_params()
    y64, h64, c64, grads = _dec_reference(cd)
    dec = Decoder(vocab_embed_size=DEC_E, vocab_size=DEC_V, hidden_size=DEC_H, num_layers=2, dropout=DEC_P,
                  proj_size=DEC_PROJ)
    dec.load_state_dict(sd, strict=True)
    dec = dec.cuda().train()
    dec.compute_dtype = cd
    with _seeded(DEC_SEED) as calls:
        y, (h, c) = dec(ys.cuda())
        assert calls[0] == 1
        y.backward(dout.to(cd).cuda())
        torch.cuda.synchronize()
    ot, gt = _tols(LSTM_TOL, cd)
    worst = {}
    _close("out", y, y64, ot, worst)
    _close("hN", h, h64, ot, worst)
    _close("cN", c, c64, ot, worst)
    names = [n for n, _ in dec.named_parameters()]
    assert set(names) == set(grads)
    for n, q in dec.named_parameters():
        _close("d " + n, q.grad, grads[n], gt, worst)
    assert not dec.embed.weight.grad[M.PAD].any()
    _line("decoder %s p=%.1f" % ("bf16" if cd == BF16 else "fp32", DEC_P), worst)


# ------------------------------------------------------------------------------------------------------- LMModel
LM_P, LM_SEED = 0.5, 9


@functools.lru_cache(maxsize=None)
def _lm_reference(cfg):
    """test_lm_train_gpu.RefLM's arithmetic in float64 with the three kinds of mask site: behind the embedding, behind
    every LSTM layer (the last included); seeds in that order."""
    from test_lm_train_gpu import _batch, _lm_sd
    ntoken, ninp, nhid, nl, tied = cfg
    sd = _lm_sd(*cfg)
    leaves = {k: v.double().requires_grad_(True) for k, v in sd.items() if not (tied and k == "decoder.weight")}
    inputs, targets = _batch()
    seeds = D.seeds(LM_SEED, 1, nl + 1)
    x = leaves["encoder.weight"][inputs]
    x = x * _mask64(x.shape, LM_P, seeds[0])
    for k in range(nl):
        x, _, _ = M.lstm_layer(x, *[leaves["rnn.%s_l%d" % (n, k)] for n in ("weight_ih", "weight_hh", "bias_ih",
                                                                           "bias_hh")], None, None, explicit=True)
        x = x * _mask64(x.shape, LM_P, seeds[k + 1])
    w = leaves["encoder.weight" if tied else "decoder.weight"]
    logp = torch.log_softmax((x @ w.t() + leaves["decoder.bias"]).reshape(-1, ntoken), dim=-1)
    loss = torch.nn.NLLLoss(ignore_index=0)(logp, targets.flatten())
    loss.backward()
    return loss.item(), {k: v.grad for k, v in leaves.items()}


@pytest.mark.parametrize("cfg", ["plain", "tied"])
def test_lm_loss_and_gradients_match_fp64_under_the_same_masks(hip_lib, cfg):
    """LMModel(dropout = 0.5) in training mode, fp32, the PLAIN and TIED configurations and the batch of
    test_lm_train_gpu: nlayers + 1 seeds are drawn (embedding, then every LSTM layer, the last included); the loss within
    1e-5 relative and every gradient max|got - ref| / max(|ref|, 1e-6) < 2e-3 - the bounds of
    test_fp32_loss_and_gradients_match_the_restatement.

    Measured on an MI355X: loss 5.9e-8 (plain), 1.1e-8 (tied); worst gradient 3.3e-7, 3.0e-7."""
    import test_lm_train_gpu as T
    cfg = T.PLAIN if cfg == "plain" else T.TIED
    want, grads = _lm_reference(cfg)
    lm = T._engine(cfg, "fp32", dropout=LM_P)
    inputs, targets = T._batch()
    with _seeded(LM_SEED) as calls:
        loss, _ = lm.loss(inputs.cuda(), targets.cuda())
        assert calls[0] == cfg[3] + 1
        loss.backward()
        torch.cuda.synchronize()
    rel = abs(loss.item() - want) / want
    worst = T._check_grads(lm, grads, "loss under dropout")
    print("\nlm.loss dropout %.1f %s: loss rel err %.3g, worst gradient err %.3g" % (LM_P, cfg, rel, worst))
    assert rel < 1e-5, (loss.item(), want)


# ---------------------------------------------------------------------------------------------------- Transducer
def test_transducer_loss_and_gradients_match_fp64_under_the_same_masks(hip_lib, monkeypatch):
    """Transducer(enc_dropout = 0.3, dec_dropout = 0.2, output_loss=True) on the ``tiny`` golden case in fp32 (three
    encoder layers on the per-layer kernels, two prediction layers): the encoder draws seeds 1..3 in layer order, the
    prediction network seed 4.  Loss within 1e-5 relative, every parameter gradient within 2e-3 of max(|ref|, 1e-6):
    the bounds of test_models_gpu.test_all_parameter_gradients_match_cpu_autograd.

    Measured on an MI355X: loss 4.8e-8, worst gradient 3.0e-7."""
    from edgedict_amd import config
    from edgedict_amd.models import Transducer
    from oracle import rnnt_loss_ref as R
    from oracle.make_golden import CASES
    cfg, B, T0, U, seed = CASES["tiny"]
    sd = M.make_state_dict(cfg, seed)
    xs, ys, xlen, ylen = M.make_batch(cfg, seed + 1, B, T0, U)
    pe, pd, s0 = 0.3, 0.2, 13
    L = cfg["enc_layers"]
    seeds = D.seeds(s0, 1, L + 1)
    sd64 = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    h_enc, _ = M.encoder_forward(sd64, xs[:, :int(xlen.max())].double(), None, (1,), True,
                                 after_layer=lambda i, x: x * _mask64(x.shape, pe, seeds[i]))
    h_dec, _ = M.decoder_forward(sd64, ys[:, :int(ylen.max())], None, True,
                                 after_layer=lambda k, x: x * _mask64(x.shape, pd, seeds[L]) if k == 0 else x)
    logits = M.joint_forward(sd64, h_enc, h_dec)
    act_lens = M.scale_length(logits.shape[1], xlen)
    costs, dlogits = R.rnnt_loss_torch_fast(logits.detach(), ys[:, :int(ylen.max())], act_lens, ylen)
    logits.backward(dlogits / B)

    monkeypatch.setattr(config, "DECODER_ENQUEUE_FIRST", False)      # the encoder draws its seeds first
    m = Transducer(enc_dropout=pe, dec_dropout=pd, output_loss=True, **cfg)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().train()
    m.compute_dtype = "fp32"
    with _seeded(s0) as calls:
        loss = m(xs.cuda(), ys.cuda(), xlen.cuda(), ylen.cuda())
        assert calls[0] == L + 1
        loss.backward()
        torch.cuda.synchronize()
    rel = abs(loss.item() - costs.mean().item()) / costs.mean().item()
    worst = 0.0
    for name, q in m.named_parameters():
        ref = sd64[name].grad
        assert q.grad is not None, name
        err = (q.grad.double().cpu() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-6)
        worst = max(worst, err)
        assert err < 2e-3, (name, err)
    print("\ntransducer tiny enc_dropout %.1f dec_dropout %.1f: loss rel err %.3g, worst gradient err %.3g"
          % (pe, pd, rel, worst))
    assert rel < 1e-5, (loss.item(), costs.mean().item())
    assert m.decoder.embed.weight.grad[M.PAD].abs().max().item() == 0
