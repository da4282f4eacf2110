"""GPU: MFMA GEMM vs a plain torch fp32/fp64 reference of the same product.

Every product is an entry of tests/gemm_cases.py; ``_gemm`` asserts, on the real tensors, that it plans to the kernel
the entry (and the test's name) says before it runs it.  tests/test_gemm_routes_host.py holds the table itself to its
routes without a device."""
import pytest
import torch

import gemm_cases
from gemm_cases import CASES

pytestmark = pytest.mark.gpu

IMPL = {}       # what ran the last _gemm product: "kernel <id>" or "hipBLASLt (vendor route <n>)"


def _assert_route(c, rec):
    assert rec[0] == c.kernel, (c.name, rec)
    assert c.split is None or rec[4] == c.split, (c.name, rec)
    assert c.vendor is None or rec[8] == c.vendor, (c.name, rec)


def _gemm(c, a, b, out=None, bias=None, bias2=None):
    """ops.gemm of the entry ``c`` on these tensors - after asserting that it plans to the entry's route."""
    from edgedict_amd import _lib, ops
    assert (a.shape, b.shape) == ((c.M, c.K), (c.N, c.K)), c.name
    kw = gemm_cases.kwargs(c, out, bias, bias2)
    rec = ops.gemm_plan(a, b, **kw)
    _assert_route(c, rec)
    lib = _lib.load()
    before = lib.edgedict_blaslt_calls()
    res = ops.gemm(a, b, **kw)
    vendor_ran = lib.edgedict_blaslt_calls() != before
    assert not vendor_ran or rec[8] != 0, (c.name, rec)
    IMPL["last"] = "hipBLASLt (vendor route %d)" % rec[8] if vendor_ran else "kernel %d" % rec[0]
    return res


def _mk(shape, dtype, seed, transposed=False):
    g = torch.Generator(device="cpu").manual_seed(seed)
    if transposed:
        x = torch.randn(shape[1], shape[0], generator=g).to(dtype).cuda().t()
    else:
        x = torch.randn(*shape, generator=g).to(dtype).cuda()
    return x


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (64, 16, 1024), (300, 200, 72), (1, 7, 8),
                                   (513, 1030, 264), (129, 640, 896)])
@pytest.mark.parametrize("ta,tb", [(False, False), (True, False), (False, True), (True, True)])
def test_gemm_layouts(hip_lib, dtype, M, N, K, ta, tb):
    c = CASES["layouts/%s-%dx%dx%d-%s%s" % ("f32" if dtype == torch.float32 else "bf16", M, N, K, "nt"[ta], "nt"[tb])]
    a, b = gemm_cases.operands(c, "cuda", 1, 2)   # asymmetric operands: catches row/col swaps
    bias = torch.arange(N, dtype=torch.float32).cuda() * 0.01
    out = _gemm(c, a, b, bias=bias)
    assert out.dtype == torch.float32
    ref = (a.double() @ b.double().t() + bias.double()).float()
    tol = 2e-5 * (K ** 0.5) if dtype == torch.float32 else 2e-5 * (K ** 0.5)
    # bf16 products are exact in fp32; only the accumulation order differs in both modes
    assert (out - ref).abs().max().item() <= tol * max(1.0, ref.abs().max().item() / 10)


def test_gemm_bf16_output_accumulate_and_splitk(hip_lib):
    M, N, K = 256, 384, 4096
    a = _mk((M, K), torch.bfloat16, 3)
    b = _mk((N, K), torch.bfloat16, 4)
    ref = a.double() @ b.double().t()
    # bf16 out: the 64 x 64 ring kernel of gemm_nt.hip (id 10) - or, vendor word 2, hipBLASLt where the bridge is built in
    out = _gemm(CASES["splitk/bf16_out"], a, b)
    assert out.dtype == torch.bfloat16
    assert (out.double() - ref).abs().max().item() < 0.02 * ref.abs().max().item(), "computed by " + IMPL["last"]
    acc = torch.ones(M, N, device="cuda")
    _gemm(CASES["splitk/acc_f32"], a, b, out=acc)
    assert (acc.double() - ref - 1).abs().max().item() < 1e-3 * ref.abs().max().item()
    sk = torch.ones(M, N, device="cuda")
    _gemm(CASES["splitk/acc_split8"], a, b, out=sk)
    assert (sk.double() - ref - 1).abs().max().item() < 1e-3 * ref.abs().max().item()
    sk2 = torch.full((M, N), 7.0, device="cuda")
    _gemm(CASES["splitk/store_split5"], a, b, out=sk2)      # not accumulating: prior contents must not leak
    assert (sk2.double() - ref).abs().max().item() < 1e-3 * ref.abs().max().item()


def test_gemm_strided_views_and_second_bias(hip_lib):
    w = _mk((640, 896), torch.float32, 5)
    x = _mk((77, 640), torch.float32, 6)
    b1 = torch.randn(640).cuda()
    b2 = torch.randn(640).cuda()
    out = _gemm(CASES["strided/left_cols_two_biases"], x, w[:, :640], bias=b1, bias2=b2)   # column slice of W (ld = 896)
    ref = x @ w[:, :640].t() + b1 + b2
    assert (out - ref).abs().max().item() < 1e-3
    out2 = _gemm(CASES["strided/right_cols"], x[:, :256].contiguous(), w[:, 640:])
    ref2 = x[:, :256] @ w[:, 640:].t()
    assert (out2 - ref2).abs().max().item() < 1e-3


@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (1, 8, 64), (300, 200, 640), (1029, 2048, 128),
                                   (64 * 33, 4096, 1024), (130, 136, 4096)])
def test_gemm_nt_direct_to_lds_path(hip_lib, M, N, K):
    """bf16 x bf16 -> bf16 with K-contiguous operands and K % 64 == 0 runs gemm_nt.hip
    (global_load_lds double buffering, source-side swizzle; the 64 x 64, the 128 x 128 and, from K = 1024 on few tiles,
    the ring kernel): ragged M/N edges, both biases, strided operands, in-place accumulation - into a view of a
    larger buffer whose margin (two rows below, eight columns to the right) must stay as it was."""
    cs, ca = CASES["nt/%dx%dx%d-store" % (M, N, K)], CASES["nt/%dx%dx%d-acc" % (M, N, K)]
    a, b = gemm_cases.operands(cs, "cuda", 11, 12)      # a = full[:, 64:]: lda = K + 64, 128-byte offset
    b1 = torch.randn(N, generator=torch.Generator().manual_seed(1)).cuda()
    b2 = torch.randn(N, generator=torch.Generator().manual_seed(2)).cuda()
    ref = a.double() @ b.double().t() + b1.double() + b2.double()
    out, buf = gemm_cases.output(cs, "cuda")
    before = buf.clone()
    _gemm(cs, a, b, out=out, bias=b1, bias2=b2)
    assert out.dtype == torch.bfloat16
    # one bf16 rounding of an fp32-accumulated value
    err = (out.double() - ref).abs()
    assert (err <= 2.0 ** -8 * ref.abs() + 1e-3 * (K ** 0.5)).all()
    assert gemm_cases.margin_untouched(cs, buf, before).all()
    base = _mk((M, N), torch.bfloat16, 13)
    acc, buf = gemm_cases.output(ca, "cuda", fill=base)
    before = buf.clone()
    _gemm(ca, a, b, out=acc)
    ref2 = base.double() + (a.double() @ b.double().t())
    err2 = (acc.double() - ref2).abs()
    assert (err2 <= 2.0 ** -7 * ref2.abs() + 2e-3 * (K ** 0.5)).all()
    assert gemm_cases.margin_untouched(ca, buf, before).all()


def test_large_short_k_product_vendor_route_matches_own_kernel(hip_lib):
    """M*N >= 2^28 with K <= 1024 (the joint's logits product): 513 x 8 macro-tiles, and from 512 macro-tiles on the
    persistent ring kernel of gemm_nt256r.hip (kernel id 12) wins BEFORE the vendor branch of the plan - the vendor
    word is 0, hipBLASLt is never tried (the vendor branch takes such a product only with the macro-tile kernels
    switched off).  A row slice of the same operands is small enough to run the 64 x 64-tile kernel of gemm_nt.hip
    (id 7): same values up to the summation order of an fp32-accumulated, bf16-rounded result, ragged M included."""
    M, N, K = 131072 + 37, 2048, 640
    a = _mk((M, K), torch.bfloat16, 21)
    b = _mk((N, K), torch.bfloat16, 22)
    bias = torch.randn(N, generator=torch.Generator().manual_seed(3)).cuda()
    out = _gemm(CASES["bigshortk/whole"], a, b, bias=bias)
    assert out.dtype == torch.bfloat16 and out.shape == (M, N) and IMPL["last"] == "kernel 12"
    for r0 in (0, 70001, M - 300):
        own = _gemm(CASES["bigshortk/rows-%d" % r0], a[r0:r0 + 300], b, bias=bias)
        ref = a[r0:r0 + 300].double() @ b.double().t() + bias.double()
        assert ((out[r0:r0 + 300].double() - ref).abs() <= 2.0 ** -8 * ref.abs() + 0.03).all()
        assert ((out[r0:r0 + 300].float() - own.float()).abs() <= 2.0 ** -7 * own.float().abs() + 0.03).all()


@pytest.mark.parametrize("M,N,K", [(256 * 33 + 37, 4096, 128), (256 * 66 + 1, 2048, 640), (256 * 130, 1000, 192)])
def test_gemm_nt256_macro_tile_path(hip_lib, M, N, K):
    """Large bf16 NT products (>= 512 macro-tiles) run gemm_nt256.hip (256 x 256 tiles, half-tile DMA
    pipeline with counted waits): ragged M and N edges, both biases, strided A - against fp64 on row
    slices, and against the 64 x 64-tile kernel of gemm_nt.hip on the same operands (EDGEDICT_GEMM_NT256 is read once
    per process, so the comparison kernel is reached through a row slice that is too small for this path).  With the
    ring kernel on (the default) these products plan to its persistent form, kernel id 12."""
    cw = CASES["nt256/%dx%dx%d-whole" % (M, N, K)]
    a, b = gemm_cases.operands(cw, "cuda", 31, 32)      # a = full[:, 64:]
    b1 = torch.randn(N, generator=torch.Generator().manual_seed(4)).cuda()
    b2 = torch.randn(N, generator=torch.Generator().manual_seed(5)).cuda()
    out = _gemm(cw, a, b, bias=b1, bias2=b2)
    assert out.dtype == torch.bfloat16 and out.shape == (M, N)
    for r0 in (0, 255, M // 2 + 3, M - 300):
        ref = a[r0:r0 + 300].double() @ b.double().t() + b1.double() + b2.double()
        err = (out[r0:r0 + 300].double() - ref).abs()
        assert (err <= 2.0 ** -8 * ref.abs() + 1e-3 * (K ** 0.5)).all(), r0
        small = _gemm(CASES["nt256/%dx%dx%d-rows-%d" % (M, N, K, r0)], a[r0:r0 + 300], b, bias=b1, bias2=b2)
        assert ((out[r0:r0 + 300].float() - small.float()).abs() <= 2.0 ** -7 * small.float().abs() + 0.03).all()
    assert torch.isfinite(out.float()).all()


@pytest.mark.parametrize("M,N,K,lse,bias", [
    (256 * 40, 2048, 640, True, True),          # 320 tiles: some workgroups walk two tiles, all full
    (256 * 70 + 37, 2048, 640, True, True),     # the logits shape, ragged last row panel, 3 tiles per workgroup
    (256 * 100 + 5, 640, 2048, False, False),   # the dhid shape: 3 column tiles, the last one ragged (N = 640)
    (256 * 36, 4096, 128, False, True),         # K = 128: two K tiles per tile, the ring wraps every tile
    (256 * 80 + 100, 1000, 192, True, True),    # odd number of K tiles (slot parity flips between tiles), ragged N
    (300, 520, 256, False, True),               # fewer tiles than CUs: one tile per workgroup
])
def test_gemm_nt256_ring_kernel_full_output(hip_lib, M, N, K, lse, bias):
    """The persistent ring kernel (gemm_nt256r.hip): EVERY element of C - and every log-sum-exp partial - against
    the one-tile-per-workgroup kernel of round 2-5 on the same operands (bit-identical: same MFMA order over K) and
    against an fp32 product; twice in a row (a stale ring slot or a race would not repeat)."""
    import ctypes
    import os
    from edgedict_amd import _lib
    from edgedict_amd.ops import _ll
    a = _mk((M, K), torch.bfloat16, 41)
    b = _mk((N, K), torch.bfloat16, 42)
    bv = torch.randn(N, generator=torch.Generator().manual_seed(6)).cuda() if bias else None
    slots = (N + 63) // 64
    entry = CASES["ring_lse/%dx%dx%d" % (M, N, K)]
    assert (entry.lse, entry.bias) == (True, int(bias))

    def run():
        c = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device="cuda")
        parts = torch.full((M, slots, 2), float("nan"), device="cuda") if lse else None
        rec = (ctypes.c_int32 * 9)()
        assert hip_lib.edgedict_gemm_plan(1, 1, _lib.ptr(a), _ll(K), 1, _lib.ptr(b), _ll(K), 1, _lib.ptr(c), _ll(N), M, N, K,
                                          _lib.ptr(bv), None, 0, 1, 0, None, 1, 0, rec) == 0
        # the switch is read at every call: the ring kernel (the entry's id 13), or one tile per workgroup (11)
        assert (rec[0], rec[8]) == ((entry.kernel if os.environ["EDGEDICT_GEMM_NT256R"] == "1" else 11), 0), list(rec)
        if lse:
            _lib.call("gemm_nt_lse", a, _ll(K), b, _ll(K), c, _ll(N), M, N, K, bv, parts)
        else:
            # the macro-tile entry behind edgedict_gemm needs >= 512 tiles; the lse entry with a scratch buffer does not
            scratch = torch.empty(M, slots, 2, device="cuda")
            _lib.call("gemm_nt_lse", a, _ll(K), b, _ll(K), c, _ll(N), M, N, K, bv, scratch)
        torch.cuda.synchronize()
        return c, parts

    old_env = os.environ.get("EDGEDICT_GEMM_NT256R")
    try:
        os.environ["EDGEDICT_GEMM_NT256R"] = "1"
        c1, p1 = run()
        c2, p2 = run()
        os.environ["EDGEDICT_GEMM_NT256R"] = "0"
        c0, p0 = run()
    finally:
        if old_env is None:
            os.environ.pop("EDGEDICT_GEMM_NT256R", None)
        else:
            os.environ["EDGEDICT_GEMM_NT256R"] = old_env
    assert torch.isfinite(c1.float()).all()
    assert torch.equal(c1.view(torch.int16), c2.view(torch.int16))
    assert torch.equal(c1.view(torch.int16), c0.view(torch.int16))
    if lse:
        assert torch.isfinite(p1).all()
        assert torch.equal(p1, p2)
        # same values, same reduction tree; the exponentials go through the same instructions
        assert torch.allclose(p1, p0, rtol=1e-6, atol=0)
        mx, sm = p1[..., 0].double(), p1[..., 1].double()
        got = (mx.max(dim=1).values + torch.log((sm * torch.exp(mx - mx.max(dim=1, keepdim=True).values)).sum(1)))
        pad = slots * 64 - N
        cf = c1.double()
        ref_lse = torch.logsumexp(cf, dim=1)
        assert (got - ref_lse).abs().max().item() < 1e-4, pad
    ref = a.float() @ b.float().t()
    if bias:
        ref = ref + bv
    err = (c1.float() - ref).abs()
    assert (err <= 2.0 ** -7 * ref.abs() + 1e-3 * (K ** 0.5)).all()


def _worst(err, tol):
    """Where the largest excess over the bound sits (row, column) - for the assertion message."""
    over = err - tol
    i = int(over.argmax())
    return "worst excess %.3g at (row %d, col %d)" % (over.flatten()[i].item(), i // err.shape[1], i % err.shape[1])


def _check_weight_gradient(ca, cs):
    """dW (+)= dY^T X (both operands row-major over the reduction, dy = full[:, 8:]: row stride M + 8) through the
    background form: entry ``ca`` accumulates into a random fp32 gradient, ``cs`` stores - against fp64 (bf16 products
    are exact in fp32, only the summation order differs)."""
    M, N, K = ca.M, ca.N, ca.K
    a, b = gemm_cases.operands(ca, "cuda", 41, 42)          # a = dy.t() [M, K], b = x.t() [N, K]
    grad0 = torch.randn(M, N, generator=torch.Generator().manual_seed(6)).cuda()
    prod = a.double() @ b.double().t()
    want = grad0.double() + prod
    grad, buf = gemm_cases.output(ca, "cuda", fill=grad0)
    before = buf.clone()
    _gemm(ca, a, b, out=grad)
    tol = 3e-5 * (K ** 0.5) * max(1.0, want.abs().max().item() / 10)
    err = (grad.double() - want).abs()
    assert err.max().item() <= tol, _worst(err, tol)
    assert (err <= tol).all()
    assert gemm_cases.margin_untouched(ca, buf, before).all()
    # and without accumulate: a fresh output, or NaN-filled with a margin
    if cs.fresh:
        out = _gemm(cs, a, b)
    else:
        out, buf = gemm_cases.output(cs, "cuda")
        before = buf.clone()
        _gemm(cs, a, b, out=out)
        assert gemm_cases.margin_untouched(cs, buf, before).all()
    err = (out.double() - prod).abs()
    assert err.max().item() <= tol, _worst(err, tol)
    assert (err <= tol).all()


@pytest.mark.parametrize("M,N,K,split", [(2048, 640, 9000, 4)] + [t[:4] for t in gemm_cases.TN256_RAGGED])
def test_gemm_tn256_weight_gradient_path(hip_lib, M, N, K, split):
    """Background weight-gradient products with M * N >= 2^18 and K >= 1024 run gemm_tn256.hip (kernel id 14): 256 x 128
    tiles, transpose reads out of LDS, fp32 K-slice partials written once and summed by the reduce pass.  One whole-tile
    shape with as many workgroups as items, and the ragged ones of gemm_cases.TN256_RAGGED: last row / column tiles of
    8 (the operand clamps at M - 8 and N - 8, the epilogue's masks), 289 items on 145 workgroups (the item walk), K not
    a multiple of the 32-k stage or of the slice length, requested slices lowered by the plan - strided operands,
    accumulate into an existing gradient and plain store into a NaN-filled view whose margin must stay as it was."""
    ca, cs = CASES["tn256/%dx%dx%d-acc" % (M, N, K)], CASES["tn256/%dx%dx%d-store" % (M, N, K)]
    assert ca.split_k == cs.split_k == split and ca.kernel == cs.kernel == 14
    _check_weight_gradient(ca, cs)


def test_gemm_weight_gradient_with_odd_m_runs_the_generic_quiet_form(hip_lib):
    """M % 8 != 0 is not for gemm_tn256.hip: the guarded generic kernel (id 3) writes the K slices to the partials
    buffer and the reduce pass sums them - same bound."""
    ca, cs = CASES["tn256_fallback/1028x264x1031-acc"], CASES["tn256_fallback/1028x264x1031-store"]
    _check_weight_gradient(ca, cs)


@pytest.mark.parametrize("M,N,K,split", [(512, 256, 4096, 2), (1024, 240, 5003, 4), (264, 648, 1111, 1)])
def test_gemm_generic_quiet_form_small_weight_gradients(hip_lib, M, N, K, split):
    """Background weight-gradient products with M * N < 2^18 stay on the generic kernel (id 4, FAST <bf16, f32>) in its
    quiet form: K slices to a partials buffer with plain stores, then the reduce pass.  tiles x slices is 16, 64 and
    18 - far below the residency cap, one item per workgroup (the cap binds in
    test_gemm_background_form_with_the_cap_binding)."""
    ca, cs = CASES["quiet_small/%dx%dx%d-acc" % (M, N, K)], CASES["quiet_small/%dx%dx%d-store" % (M, N, K)]
    assert ca.split_k == cs.split_k == split
    _check_weight_gradient(ca, cs)


@pytest.mark.parametrize("M,N,K", [(768, 1024, 4096), (1000, 1000, 1024), (1536, 1024, 4096), (70, 200, 2048)])
def test_gemm_nt_small_long_k_ring_path(hip_lib, M, N, K):
    """Small-M long-K bf16 NT products with in-place accumulation (the encoder stack's per-chunk
    dX = dG x W_ih under the BPTT) run the 64 x 64-tile ring kernel of gemm_nt.hip (four K stages, counted
    waits): ragged edges, accumulate and plain store, against fp64 with bf16 output rounding."""
    a = _mk((M, K), torch.bfloat16, 51)
    b = _mk((N, K), torch.bfloat16, 52)
    c0 = _mk((M, N), torch.bfloat16, 53)
    prod = a.double() @ b.double().t()
    # (M >= 256 with K >= 2048: the plan's vendor word is 2, and a library built with the hipBLASLt bridge runs these
    # there - the message says which implementation was measured; the bound is the same)
    out = _gemm(CASES["ring64/%dx%dx%d-store" % (M, N, K)], a, b)
    assert ((out.double() - prod).abs() <= 2.0 ** -7 * prod.abs() + 1e-3 * (K ** 0.5)).all(), "computed by " + IMPL["last"]
    acc = c0.clone()
    _gemm(CASES["ring64/%dx%dx%d-acc" % (M, N, K)], a, b, out=acc)
    want = c0.double() + out.double()         # the kernel adds its bf16-rounded tile to the bf16 C
    assert ((acc.double() - want).abs() <= 2.0 ** -6 * want.abs() + 1e-2).all(), "computed by " + IMPL["last"]


def test_gemm_nt256_one_tile_per_workgroup_kernel_with_bias_by_default_routing(hip_lib):
    """N = 768 is three column tiles: with a bias and more tiles (258) than the ring kernel's 256 workgroups, a
    workgroup's tiles would not share their column tile, so the product runs the one-tile-per-workgroup kernel of
    gemm_nt256.hip (kernel id 11 of edgedict_gemm_plan) - without any switch.  Against the fp32 product."""
    import ctypes
    from edgedict_amd import _lib
    from edgedict_amd.ops import _ll
    M, N, K = 256 * 86, 768, 128
    a = _mk((M, K), torch.bfloat16, 61)
    b = _mk((N, K), torch.bfloat16, 62)
    bv = torch.randn(N, generator=torch.Generator().manual_seed(7)).cuda()
    c = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device="cuda")
    parts = torch.full((M, N // 64, 2), float("nan"), device="cuda")
    rec = (ctypes.c_int32 * 9)()
    assert hip_lib.edgedict_gemm_plan(1, 1, _lib.ptr(a), _ll(K), 1, _lib.ptr(b), _ll(K), 1, _lib.ptr(c), _ll(N), M, N, K,
                                      _lib.ptr(bv), None, 0, 1, 0, None, 1, 0, rec) == 0
    assert list(rec)[:4] == [11, 258, 512, 128 * 1024]
    entry = CASES["nt256_one_tile/22016x768x128"]
    assert (entry.M, entry.N, entry.K, entry.kernel, entry.lse, entry.bias) == (M, N, K, rec[0], True, 1)
    _lib.call("gemm_nt_lse", a, _ll(K), b, _ll(K), c, _ll(N), M, N, K, bv, parts)
    ref = a.float() @ b.float().t() + bv
    err = (c.float() - ref).abs()
    assert (err <= 2.0 ** -7 * ref.abs() + 1e-3 * (K ** 0.5)).all()
    cf = c.double()
    mx, sm = parts[..., 0].double(), parts[..., 1].double()
    top = mx.max(dim=1, keepdim=True).values
    got = top[:, 0] + torch.log((sm * torch.exp(mx - top)).sum(1))
    assert (got - torch.logsumexp(cf, dim=1)).abs().max().item() < 1e-4


# ------------------------------------------------------------------------------------------------ routes nothing reached
def _names(prefix):
    return [c.name for c in gemm_cases.group(prefix)]


def _run_with_margin(c, seed):
    """Run entry ``c`` into a view of a larger buffer (NaN-filled; a seeded tensor under accumulate) and check the
    margin.  Returns (out, fp64 product + biases, the fp64 starting values or None)."""
    a, b = gemm_cases.operands(c, "cuda", seed, seed + 1)
    bs = [torch.randn(c.N, generator=torch.Generator().manual_seed(seed + 2 + i)).cuda() for i in range(c.bias)] + [None, None]
    base = _mk((c.M, c.N), gemm_cases.DTYPES[c.out], seed + 4) if c.accumulate else None
    out, buf = gemm_cases.output(c, "cuda", fill=base if c.accumulate else float("nan"))
    before = buf.clone()
    _gemm(c, a, b, out=out, bias=bs[0], bias2=bs[1])
    assert gemm_cases.margin_untouched(c, buf, before).all(), c.name
    ref = a.double() @ b.double().t()
    for v in bs[:c.bias]:
        ref = ref + v.double()
    return out, ref, None if base is None else base.double()


def _assert_bf16_result(c, out, ref, base):
    # the bounds of test_gemm_nt_direct_to_lds_path: one bf16 rounding of an fp32-accumulated value
    assert out.dtype == torch.bfloat16
    if base is None:
        err, tol = (out.double() - ref).abs(), 2.0 ** -8 * ref.abs() + 1e-3 * (c.K ** 0.5)
    else:
        err, tol = (out.double() - (base + ref)).abs(), 2.0 ** -7 * (base + ref).abs() + 2e-3 * (c.K ** 0.5)
    assert (err <= tol).all(), _worst(err, tol)


@pytest.mark.parametrize("name", _names("generic_bf16"))
def test_gemm_generic_bf16_output(hip_lib, name):
    """gemm_kernel<bf16, bf16> of gemm.hip - FAST (id 2) and guarded (id 1) - which the NT kernels leave only what they
    cannot take: K % 64 != 0, a transposed operand, a K tail of 5, an A that lost its 16-byte alignment.  The
    vectorised C store through LDS, its scalar fallback (N % 8 != 0), biases, accumulate into bf16."""
    c = CASES[name]
    _assert_bf16_result(c, *_run_with_margin(c, 71))


@pytest.mark.parametrize("name", _names("ktail"))
def test_gemm_k_tails_fp32_output(hip_lib, name):
    """K-contiguous operands whose K is not a multiple of the vector width (bf16: 8, fp32: 4) run the guarded generic
    kernels (ids 3 and 5); K = 1; and K = 0, where nothing is read and C is the bias rows (or stays as it is)."""
    c = CASES[name]
    out, ref, base = _run_with_margin(c, 81)
    want = ref if base is None else base + ref
    tol = 2e-5 * (c.K ** 0.5) * max(1.0, want.abs().max().item() / 10)     # K = 0: exact
    err = (out.double() - want).abs()
    assert (err <= tol).all(), _worst(err, tol)
    if c.K == 0 and c.accumulate:
        assert torch.equal(out.view(torch.int32), base.float().view(torch.int32))
    elif c.K == 0:
        bias = torch.randn(c.N, generator=torch.Generator().manual_seed(83)).cuda()
        assert torch.equal(out, bias.expand(c.M, c.N))


@pytest.mark.parametrize("name", _names("split"))
def test_gemm_split_k_variants(hip_lib, name):
    """Split-K beyond FAST bf16 without a bias: a bias (added once, by slice 0) into a zeroed C whose old contents (7.0)
    must not show, the guarded kernel, fp32 operands with the slices rounded up to 8, more slices than K tiles."""
    c = CASES[name]
    a, b = gemm_cases.operands(c, "cuda", 91, 92)
    bias = torch.randn(c.N, generator=torch.Generator().manual_seed(93)).cuda() if c.bias else None
    base = _mk((c.M, c.N), torch.float32, 94) if c.accumulate else None
    out, buf = gemm_cases.output(c, "cuda", fill=base if c.accumulate else 7.0 if c.bias else float("nan"))
    before = buf.clone()
    _gemm(c, a, b, out=out, bias=bias)
    assert gemm_cases.margin_untouched(c, buf, before).all()
    ref = a.double() @ b.double().t()
    if c.bias:
        ref = ref + bias.double()
    got = out.double() - base.double() if c.accumulate else out.double()
    err = (got - ref).abs()
    assert (err < 1e-3 * ref.abs().max().item()).all(), _worst(err, 1e-3 * ref.abs().max().item())


@pytest.mark.parametrize("name", _names("bg"))
def test_gemm_background_form_with_the_cap_binding(hip_lib, name):
    """The background form where the residency cap binds: 64 tiles x 8 slices = 512 items on 256 workgroups (two items
    each, the slice fixed per workgroup) - quiet (partials + reduce pass), atomic (a bias: zero pass, slice 0 adds the
    bias) - and on 512 workgroups with two per CU; bf16 output with a bias under the cap."""
    c = CASES[name]
    out, ref, _ = _run_with_margin(c, 101)
    if c.out == "bf16":
        _assert_bf16_result(c, out, ref, None)
        return
    tol = 3e-5 * (c.K ** 0.5) * max(1.0, ref.abs().max().item() / 10)
    err = (out.double() - ref).abs()
    assert (err <= tol).all(), _worst(err, tol)


def test_gemm_nt_128_tile_ragged_edges_with_margin(hip_lib):
    """gemm_nt_kernel<128,128,64> (id 8) with a last row tile of ONE row and a last column tile of 8 columns, a bias,
    into a view whose margin must stay as it was."""
    c = CASES["nt/1153x1544x128-store"]
    _assert_bf16_result(c, *_run_with_margin(c, 111))
