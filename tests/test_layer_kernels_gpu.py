"""GPU: the layer kernels between the big products - LayerNorm (+ residual, + TimeReduction), the prediction
network's embedding, the front-end's causal convolution and GELU-GroupNorm, and the colsum / cast / transpose helpers -
against a float64 restatement of the same operation, at the shapes where their tails live: scalar vs 16-byte vector
paths, the odd last frame of the time reduction, grid-stride loops past the grid caps, partial 256-row slabs, tiles
that do not divide the matrix.  Every output and gradient is compared element by element; a tail is also compared on
its own, so that a wrong tail cannot hide under the scale of the bulk."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import frontend_ref as FR
from oracle import models_ref as M

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
BF16_ULP = 2.0 ** -8          # one bf16 ulp relative to the value: half an ulp of output rounding + fp32 arithmetic


def _close(got, ref, tol, what=""):
    """max |got - ref| <= tol * max |ref| (the test_lstm_gpu._close criterion, here in float64)."""
    ref = ref.detach().double().cpu()
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    assert torch.isfinite(got).all(), what
    err = (got - ref).abs().max().item() if ref.numel() else 0.0
    scale = max(ref.abs().max().item() if ref.numel() else 0.0, 1e-3)
    assert err <= tol * scale, (what, err, scale, tol)


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


# ------------------------------------------------------------------------------------------------ LayerNorm
def _ln_ref(x, res, gamma, beta, reduce, dout, eps=1e-5):
    """float64: y = time_reduction(layer_norm(x + res)), the zero frame added after the norm; returns
    (y, mean, rstd, ds, dgamma, dbeta) with ds the gradient of the sum x + res."""
    s = (x.double() + (res.double() if res is not None else 0.0)).requires_grad_(True)
    g = gamma.double().requires_grad_(True)
    b = beta.double().requires_grad_(True)
    mean = s.mean(-1)
    rstd = 1.0 / torch.sqrt(((s - mean[..., None]) ** 2).mean(-1) + eps)
    y = M.layer_norm(s, g, b, eps)
    if reduce == 2:
        y = M.time_reduction(y, 2)
    y.backward(dout.double())
    return y.detach(), mean.detach().reshape(-1), rstd.detach().reshape(-1), s.grad, g.grad, b.grad


def _ln_inputs(B, T, D, dtype, residual, reduce, seed):
    g = _gen(seed)
    # a per-row offset and spread, so that the mean and the variance both matter
    x = (torch.randn(B, T, D, generator=g) * (0.5 + torch.rand(B, T, 1, generator=g))
         + torch.randn(B, T, 1, generator=g)).to(dtype)
    res = torch.randn(B, T, D, generator=g).to(dtype) if residual else None
    gamma = 1.0 + 0.5 * torch.randn(D, generator=g)
    beta = 0.5 * torch.randn(D, generator=g)
    Tout = (T + reduce - 1) // reduce
    dout = torch.randn(B, Tout, D, generator=g).to(dtype)
    return x, res, gamma, beta, dout


def _ln_run(x, res, gamma, beta, reduce, dout):
    from edgedict_amd import ops
    xd = x.cuda()
    rd = res.cuda() if res is not None else None
    y, mean, rstd = ops.layernorm_fwd(xd, rd, gamma.cuda(), beta.cuda(), reduce)
    ds, dg, db = ops.layernorm_bwd(dout.cuda(), xd, rd, gamma.cuda(), mean, rstd, reduce)
    return y, mean, rstd, ds, dg, db


def _ln_check(got, ref, dtype, T, reduce, big=False):
    y, mean, rstd, ds, dg, db = got
    ry, rmean, rrstd, rds, rdg, rdb = ref
    out_tol = 1e-5 if dtype == F32 else BF16_ULP      # fp32: normalisation arithmetic; bf16: rounding of y / ds
    _close(mean, rmean, 1e-5, "mean")                 # fp32 statistics of the (bf16-exact) inputs in both dtypes
    _close(rstd, rrstd, 1e-5, "rstd")
    _close(y, ry, out_tol, "y")
    _close(ds, rds, out_tol, "ds")
    red_tol = 3e-5 if big else 1e-5                   # fp32 sums over B*T rows (per-wave LDS, then atomics)
    _close(dg, rdg, red_tol, "dgamma")
    _close(db, rdb, red_tol, "dbeta")
    if reduce == 2 and T % 2 == 1:
        # the odd last output frame is (LN(x_last) + 0) / 2, and its input frame gets half the gradient
        _close(y[:, -1], ry[:, -1], out_tol, "y last frame")
        _close(ds[:, -1], rds[:, -1], out_tol, "ds last frame")


# (D, residual, reduce, T), each in both dtypes: D 250 takes the scalar path (250 % 4 != 0), the others the 16-byte
# vector path; T 1 and 7 with reduce 2 end on a lone frame; D 2048 fills the backward's LDS accumulators exactly
LN_CASES = [(24, True, 2, 7), (24, False, 1, 1), (250, True, 2, 1), (250, False, 2, 8), (256, True, 1, 2),
            (256, False, 2, 7), (1000, True, 2, 7), (1000, False, 1, 8), (1024, True, 2, 2), (1024, False, 2, 1),
            (2048, True, 2, 7), (2048, False, 1, 2)]


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("D,residual,reduce,T", LN_CASES)
def test_layernorm_fwd_bwd_matches_fp64(hip_lib, dtype, D, residual, reduce, T):
    x, res, gamma, beta, dout = _ln_inputs(3, T, D, dtype, residual, reduce, seed=D + T + 10 * reduce)
    got = _ln_run(x, res, gamma, beta, reduce, dout)
    _ln_check(got, _ln_ref(x, res, gamma, beta, reduce, dout), dtype, T, reduce)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_layernorm_past_both_grid_caps(hip_lib, dtype):
    """B*T = 38464 rows: the forward's 19232 output rows need more than its 4096 workgroups x 4 waves (grid-stride
    loop), and the backward's 1202 workgroups are capped at 1024 (grid-stride loop, then dgamma / dbeta through the
    cross-workgroup atomics)."""
    B, T, D = 64, 601, 256
    x, res, gamma, beta, dout = _ln_inputs(B, T, D, dtype, True, 2, seed=5)
    got = _ln_run(x, res, gamma, beta, 2, dout)
    _ln_check(got, _ln_ref(x, res, gamma, beta, 2, dout), dtype, T, 2, big=True)
    # the last batch row is the one a grid-stride loop reaches last
    _close(got[0][-1], _ln_ref(x[-1:], res[-1:], gamma, beta, 2, dout[-1:])[0][0],
           1e-5 if dtype == F32 else BF16_ULP, "last sample")


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("D", [24, 256, 1024])
def test_layernorm_scalar_path_equals_vector_path_bit_for_bit(hip_lib, dtype, D):
    """x as a contiguous view one element past a 16-byte boundary forces the scalar path on a D the vector path would
    take.  The scalar path once summed a row in another order (lane-strided) than the vector path (VEC consecutive
    elements per lane): the statistics, and every output, then depended on the alignment of the input."""
    from edgedict_amd import ops
    B, T = 3, 7
    x, res, gamma, beta, dout = _ln_inputs(B, T, D, dtype, True, 2, seed=D)
    xa = x.cuda()
    buf = torch.empty(B * T * D + 1, dtype=dtype, device="cuda")
    xm = buf[1:].view(B, T, D)
    xm.copy_(xa)
    assert xm.is_contiguous() and xm.data_ptr() % 16 != 0
    for r in (None, res.cuda()):
        a = ops.layernorm_fwd(xa, r, gamma.cuda(), beta.cuda(), 2)
        m = ops.layernorm_fwd(xm, r, gamma.cuda(), beta.cuda(), 2)
        for name, u, v in zip(("y", "mean", "rstd"), a, m):
            assert torch.equal(u, v), (name, (u.float() - v.float()).abs().max().item())
        da = ops.layernorm_bwd(dout.cuda(), xa, r, gamma.cuda(), a[1], a[2], 2)
        dm = ops.layernorm_bwd(dout.cuda(), xm, r, gamma.cuda(), m[1], m[2], 2)
        assert torch.equal(da[0], dm[0])
    _ln_check(_ln_run(x, res, gamma, beta, 2, dout), _ln_ref(x, res, gamma, beta, 2, dout), dtype, T, 2)


def test_layernorm_bwd_rejects_a_row_too_wide_for_its_lds_accumulators(hip_lib):
    from edgedict_amd import ops
    D = 2056                                          # 4 waves x 2 x D floats > 64 KiB of LDS
    x, res, gamma, beta, dout = _ln_inputs(2, 3, D, F32, False, 1, seed=1)
    y, mean, rstd = ops.layernorm_fwd(x.cuda(), None, gamma.cuda(), beta.cuda(), 1)
    with pytest.raises(RuntimeError, match="too large for the LDS"):
        ops.layernorm_bwd(dout.cuda(), x.cuda(), None, gamma.cuda(), mean, rstd, 1)
    torch.cuda.synchronize()


@pytest.mark.parametrize("cd", [F32, BF16])
def test_input_norm_fn_casts_and_honours_needs_input_grad(hip_lib, cd):
    """_InputNormFn (the encoder's input LayerNorm): fp32 features in, compute dtype out, dx back in fp32."""
    from edgedict_amd.models import _InputNormFn
    B, T, D = 4, 9, 240
    x, _, gamma, beta, dout = _ln_inputs(B, T, D, F32, False, 1, seed=11)
    dout = dout.to(cd)
    xc = x.to(cd)                                     # the operand the kernel sees
    ry, _, _, rds, rdg, rdb = _ln_ref(xc, None, gamma, beta, 1, dout)
    g = gamma.cuda().requires_grad_(True)
    b = beta.cuda().requires_grad_(True)
    xin = x.cuda().requires_grad_(True)
    y = _InputNormFn.apply(xin, g, b, cd)
    assert y.dtype == cd
    y.backward(dout.cuda())
    tol = 1e-5 if cd == F32 else BF16_ULP
    _close(y, ry, tol, "y")
    assert xin.grad.dtype == F32
    _close(xin.grad, rds, tol, "dx")
    _close(g.grad, rdg, 1e-5, "dgamma")
    _close(b.grad, rdb, 1e-5, "dbeta")
    # no input gradient wanted: the parameters still get theirs
    g.grad = b.grad = None
    _InputNormFn.apply(x.cuda(), g, b, cd).backward(dout.cuda())
    _close(g.grad, rdg, 1e-5, "dgamma without dx")


# ------------------------------------------------------------------------------------------------ embedding
def _emb_case(B, U, V, E, prepend, cd, seed, n_distinct=None, strided=False):
    from edgedict_amd.models import _EmbeddingFn
    from edgedict_amd.tokenizer import BOS, PAD
    g = _gen(seed)
    hi = n_distinct or V
    wide = torch.randint(0, hi, (B, U + 7), generator=g, dtype=torch.int32)
    if U > 2:
        wide[:, 3 + U // 2] = PAD                     # PAD inside every row
        wide[0, 3:3 + U] = PAD                        # and a row of nothing but PAD
    tok_cpu = wide[:, 3:3 + U]                        # a row slice of a wider tensor: tok_stride = U + 7
    if strided:
        tokens = wide.cuda()[:, 3:3 + U]
        assert not tokens.is_contiguous() or U == 0
    else:
        tokens = tok_cpu.contiguous().cuda()
    weight = torch.randn(V, E, generator=g)
    dout = torch.randn(B, U + (1 if prepend else 0), E, generator=g).to(cd)
    # float64 reference: BOS left-pad, nn.Embedding(padding_idx=PAD)
    full = tok_cpu.long()
    if prepend:
        full = torch.cat([torch.full((B, 1), BOS, dtype=torch.long), full], 1)
    w64 = weight.double().requires_grad_(True)
    ref = F.embedding(full, w64, padding_idx=PAD)
    ref.backward(dout.double())
    wd = weight.cuda().requires_grad_(True)
    out = _EmbeddingFn.apply(tokens, wd, prepend, cd)
    out.backward(dout.cuda())
    return out, wd.grad, ref.detach(), w64.grad, PAD


@pytest.mark.parametrize("cd", [F32, BF16])
@pytest.mark.parametrize("B,U,E,prepend,n_distinct,strided", [
    (5, 9, 8, True, None, False), (7, 13, 250, False, None, True), (64, 50, 640, True, 8, False),
    (33, 17, 250, True, 5, True), (4, 0, 640, True, None, False), (3, 1, 8, False, None, True)])
def test_embedding_fwd_bwd_matches_fp64(hip_lib, cd, B, U, E, prepend, n_distinct, strided):
    out, grad, ref, rgrad, pad = _emb_case(B, U, 2048, E, prepend, cd, seed=B * 31 + U + E, n_distinct=n_distinct,
                                           strided=strided)
    assert out.dtype == cd
    assert torch.equal(out.cpu(), ref.to(cd))         # a gather: exact (bf16 = the round-to-nearest-even of the row)
    # fp32 atomics: up to B*(U+1) rows land on one token when only a few ids occur
    _close(grad, rgrad, 1e-5, "dweight")
    assert (grad[pad] == 0).all()                     # padding_idx: the PAD row never receives gradient


def test_embedding_rejects_tokens_without_unit_column_stride(hip_lib):
    """The kernels read token (b, u) at ``tokens[b * tok_stride + u]``: a column-strided view (or int64 ids) was read
    as if it were a contiguous int32 row, silently gathering the wrong rows."""
    from edgedict_amd import ops
    w = torch.randn(64, 8, device="cuda")
    wide = torch.randint(3, 64, (4, 12), dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="unit column stride"):
        ops.embedding_fwd(wide[:, ::2], w, F32, True, 2)
    with pytest.raises(ValueError, match="int32"):
        ops.embedding_fwd(wide.long(), w, F32, True, 2)
    with pytest.raises(ValueError, match="unit column stride"):
        ops.embedding_bwd(wide[:, ::2], torch.randn(4, 7, 8, device="cuda"), 64, True, 2, 1)


# ------------------------------------------------------------------------------------------------ front-end
def _tin_min(k, s):
    """Smallest input length with one output frame: (Tin + k - 2) // s + 1 - (k - 1) >= 1."""
    return (k - 1) * (s - 1) + 1


@pytest.mark.parametrize("cd", [F32, BF16])
@pytest.mark.parametrize("k,s,C,Cout,B,Tin", [
    (1, 1, 1, 16, 2, 50), (2, 2, 37, 24, 3, 41), (3, 3, 100, 64, 2, 29), (5, 2, 256, 32, 2, 33),
    (5, 3, 1, 16, 3, _tin_min(5, 3)), (3, 1, 256, 128, 2, _tin_min(3, 1)), (2, 3, 100, 32, 2, _tin_min(2, 3)),
    (1, 2, 37, 16, 2, _tin_min(1, 2))])
def test_causal_conv_matches_fp64(hip_lib, cd, k, s, C, Cout, B, Tin):
    from edgedict_amd import ops
    from edgedict_amd.models import _CausalConvFn
    g = _gen(k * 100 + s * 10 + C)
    x = torch.randn(B, Tin, C, generator=g)
    w = torch.randn(Cout, C, k, generator=g) / math.sqrt(C * k)
    b = 0.1 * torch.randn(Cout, generator=g)
    Tout = ops.conv_out_frames(Tin, k, s)
    # float64 on the operands as the kernels see them (fp32 input cast to cd by im2col, weight cast once)
    x64 = x.to(cd).double().requires_grad_(True)
    w64 = w.to(cd).double().requires_grad_(True)
    b64 = b.double().requires_grad_(True)
    ref = FR.causal_conv(x64.permute(0, 2, 1), w64, b64, s).permute(0, 2, 1)
    assert ref.shape == (B, Tout, Cout) and Tout >= 1
    dy = torch.randn(B, Tout, Cout, generator=g).to(cd)
    ref.backward(dy.double())
    xin = x.cuda().requires_grad_(True)
    wd = w.cuda().requires_grad_(True)
    bd = b.cuda().requires_grad_(True)
    y = _CausalConvFn.apply(xin, wd, bd, s, cd)
    y.backward(dy.cuda())
    assert y.dtype == cd and xin.grad.dtype == F32
    K = C * k
    if cd == F32:
        tol = 2e-5 * math.sqrt(K)                     # the fp32 GEMM's bound (test_gemm_gpu)
        _close(y, ref, tol, "y")
        _close(xin.grad, x64.grad, 2e-5 * math.sqrt(Cout), "dx")
        _close(wd.grad, w64.grad, 2e-5 * math.sqrt(B * Tout), "dW")
    else:
        _close(y, ref, BF16_ULP, "y")                 # fp32 accumulation of exact bf16 products, one rounding
        # ceil(k / s) overlapping dcols terms, each rounded to bf16, summed in fp32 and rounded once more
        _close(xin.grad, x64.grad, 2.0 ** -8 * math.ceil(k / s), "dx")
        _close(wd.grad, w64.grad, 1e-5 * math.sqrt(B * Tout), "dW")   # fp32 output of exact bf16 products
    _close(bd.grad, b64.grad, 1e-5, "db")             # column sum of dy
    # the last output frame reads the last (partially padded) window
    _close(y[:, -1], ref[:, -1], BF16_ULP if cd == BF16 else 2e-5 * math.sqrt(K), "y last frame")
    if Tin > 1:
        with pytest.raises(ValueError, match="too few"):
            _CausalConvFn.apply(x[:, :_tin_min(k, s) - 1].cuda(), wd, bd, s, cd)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("B,T,C", [(3, 300, 100), (2, 200, 1), (5, 77, 256), (4, 131, 37), (1, 1, 256)])
def test_gelu_groupnorm_matches_fp64(hip_lib, dtype, B, T, C):
    """B*T rows in 256-row slabs of the backward, slab edges inside samples (300, 200, 77 and 131 frames), row lanes
    per workgroup 256 // C with idle threads when C does not divide 256."""
    from edgedict_amd.models import _GeluGroupNormFn
    g = _gen(B * T + C)
    y = (1.5 * torch.randn(B, T, C, generator=g) + 0.3).to(dtype)
    gamma = 1.0 + 0.3 * torch.randn(C, generator=g)
    beta = 0.3 * torch.randn(C, generator=g)
    dout = torch.randn(B, T, C, generator=g).to(dtype)
    y64 = y.double().requires_grad_(True)
    g64 = gamma.double().requires_grad_(True)
    b64 = beta.double().requires_grad_(True)
    ref = FR.group_norm_1(F.gelu(y64).permute(0, 2, 1), g64, b64).permute(0, 2, 1)
    ref.backward(dout.double())
    yd = y.cuda().requires_grad_(True)
    gd = gamma.cuda().requires_grad_(True)
    bd = beta.cuda().requires_grad_(True)
    out = _GeluGroupNormFn.apply(yd, gd, bd)
    out.backward(dout.cuda())
    if dtype == F32:
        _close(out, ref, 1e-5, "out")
        _close(yd.grad, y64.grad, 2e-5, "dy")         # erf / exp of the device math library: a few ulp
    else:
        _close(out, ref, BF16_ULP, "out")
        _close(yd.grad, y64.grad, BF16_ULP, "dy")
    _close(gd.grad, g64.grad, 2e-5, "dgamma")         # fp32 per-slab partial rows, summed slab by slab
    _close(bd.grad, b64.grad, 2e-5, "dbeta")
    # the last sample's rows come last in the last (partial) slab
    _close(out[-1], ref[-1], 1e-5 if dtype == F32 else BF16_ULP, "out last sample")
    _close(yd.grad[-1], y64.grad[-1], 2e-5 if dtype == F32 else BF16_ULP, "dy last sample")


# ------------------------------------------------------------------------------------------------ helpers
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("M,N,view,acc", [(1, 1, False, False), (3, 257, True, True), (64, 255, False, True),
                                          (65, 257, True, False), (200003, 255, True, True), (200003, 1, False, False)])
def test_colsum_matches_fp64(hip_lib, dtype, M, N, view, acc):
    from edgedict_amd import ops
    g = _gen(M + N)
    wide = (torch.randn(M, N + 13, generator=g) + 0.25).to(dtype)
    x = wide[:, :N] if view else wide[:, :N].contiguous()
    out0 = torch.randn(N, generator=g) if acc else torch.zeros(N)
    xd = wide.cuda()[:, :N] if view else x.cuda()
    assert not view or xd.stride(0) == N + 13
    got = ops.colsum(xd, out=out0.cuda())
    ref = x.double().sum(0) + out0.double()
    _close(got, ref, 1e-5, "colsum")                  # fp32 partial sums (4 per thread, then atomics per row block)
    if N > 256:
        # the last, partial 256-column block on its own (a dropped or repeated remainder row would move every column
        # by ~1 against a scale of ~M / 4: far outside the bound above)
        _close(got[256:], ref[256:], 1e-5, "last column block")


def test_cast_rounds_to_nearest_even_like_torch(hip_lib):
    """fp32 -> bf16 is torch's round-to-nearest-even bit for bit (ties, +-0, +-inf, overflow to inf, random bit
    patterns of every exponent); bf16 -> fp32 is exact for all 65536 patterns; NaN stays NaN.  fp32 subnormals: the
    kernels are built without flush-to-zero, so the hardware conversion keeps them and rounds them as torch does
    (0x00008000 -> bf16 0x0001, 0x00007fff -> +0, 0x80018000 -> 0x8002): pinned here bit for bit."""
    from edgedict_amd import ops
    special = torch.tensor([
        0x3F808000, 0x3F818000, 0x3F80C000, 0x3F817FFF, 0xBF808000, 0xBF818000,   # ties (to even) and near ties
        0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF,   # +-0, +-inf, max -> inf
        0x7F7F8000, 0x7F7F7FFF, 0x00800000, 0x80800000,                           # overflow tie, smallest normals
        0x00000001, 0x00007FFF, 0x00008000, 0x00018000, 0x007FFFFF, 0x80018000,   # subnormals
        0x807FFFFF, 0x00400000], dtype=torch.int64).to(torch.int32)
    rnd = torch.randint(-2 ** 31, 2 ** 31 - 1, (1 << 20,), generator=_gen(3), dtype=torch.int64).to(torch.int32)
    bits = torch.cat([special, rnd])
    x = bits.view(F32)
    got = ops.cast(x.cuda(), BF16).cpu()
    want = x.to(BF16)
    nan = torch.isnan(x)
    assert torch.isnan(got[nan].float()).all()
    assert torch.equal(got[~nan].view(torch.int16), want[~nan].view(torch.int16)), \
        (x[~nan][got[~nan].view(torch.int16) != want[~nan].view(torch.int16)][:8])
    sub = (bits & 0x7F800000) == 0
    assert sub.sum() > 1000                           # the random patterns include subnormals
    all16 = torch.arange(-2 ** 15, 2 ** 15, dtype=torch.int32).to(torch.int16).view(BF16)
    back = ops.cast(all16.cuda(), F32).cpu()
    nan16 = torch.isnan(all16.float())
    assert torch.isnan(back[nan16]).all()
    assert torch.equal(back[~nan16].view(torch.int32), all16[~nan16].float().view(torch.int32))


@pytest.mark.parametrize("src,dst", [(F32, F32), (F32, BF16), (BF16, BF16), (BF16, F32)])
@pytest.mark.parametrize("R,C", [(1, 1), (33, 65), (100, 7), (257, 31)])
def test_transpose_matches_torch_exactly(hip_lib, src, dst, R, C):
    from edgedict_amd import ops
    x = torch.randn(R, C, generator=_gen(R * C)).to(src)
    got = ops.transpose(x.cuda(), dst)
    assert got.shape == (C, R) and got.dtype == dst
    assert torch.equal(got.cpu(), x.t().to(dst))      # a permutation and (at most) one RNE rounding
