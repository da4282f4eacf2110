"""Every product that tests/test_gemm_gpu.py runs, as data: shapes, dtypes, layouts, view offsets, biases, accumulate,
split_k, max_wg_per_cu - and the DECISION each one is meant to exercise: the kernel id of edgedict_gemm_plan
(include/edgedict_hip.h) and, where it matters, the K slices that run and the vendor word.

tests/test_gemm_routes_host.py dry-plans every entry on meta tensors (no device) and holds it to its expected route;
tests/test_gemm_gpu.py builds its operands from the same entries and asserts the route again on the real tensors before
it runs them.  A GPU test that is named after a kernel therefore cannot drift off it unnoticed.

Kernel id 9 (gemm_nt_kernel<256,128,64>) is reachable only with EDGEDICT_GEMM_NT_TILE=256 and has no entry here.
"""
import types

import torch

DTYPES = {"bf16": torch.bfloat16, "f32": torch.float32}
# the kernels that default routing can reach (0 is the empty product, 9 needs a switch)
DEFAULT_KERNELS = {1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 12, 13, 14}

CASES = {}


def _case(name, M, N, K, kernel, dtype="bf16", out=None, ta=False, tb=False, a_off=0, a_pad=0, a_row0=0, b_off=0,
          b_pad=0, bias=0, accumulate=False, split_k=1, max_wg=0, fresh=False, margin=False, lse=False, split=None,
          vendor=None, new=False):
    """name: "<group>/<what>".  ta / tb: the operand is a transposed view ([K, rows] storage).  x_off / x_pad: columns of
    the storage before / after the view (x_off moves the pointer, both widen the leading dimension); a_row0: the view
    starts at this row of a taller storage.  bias: how many of (bias, bias2) are passed.  fresh: no ``out`` tensor
    (``out_dtype`` instead); margin: ``out`` is a view into a larger buffer (see ``output``).  lse: the product goes
    through edgedict_gemm_nt_lse.  split / vendor: expected record words 4 / 8 (None: not part of what the entry is
    about).  new: vendor word must be 0 - the result has to come from this library's kernel on every machine."""
    assert name not in CASES, name
    assert not (fresh and (margin or accumulate))
    if new and vendor is None:
        vendor = 0
    CASES[name] = types.SimpleNamespace(
        name=name, M=M, N=N, K=K, kernel=kernel, dtype=dtype, out=out or dtype, ta=ta, tb=tb, a_off=a_off, a_pad=a_pad,
        a_row0=a_row0, b_off=b_off, b_pad=b_pad, bias=bias, accumulate=accumulate, split_k=split_k, max_wg=max_wg,
        fresh=fresh, margin=margin, lse=lse, split=split, vendor=vendor, new=new)


def group(prefix):
    return [c for c in CASES.values() if c.name.startswith(prefix + "/")]


# ---------------------------------------------------------------------------------------------------- building operands
def _matrix(rows, inner, transposed, off, pad, row0, dtype, device, seed):
    """[rows, inner] view: K-contiguous rows of a [row0 + rows, off + inner + pad] storage, or the transpose of the
    columns off.. of a [inner, off + rows + pad] storage.  Values: seeded CPU normal draws of the whole storage."""
    assert not (transposed and row0)
    shape = (inner, off + rows + pad) if transposed else (row0 + rows, off + inner + pad)
    if device == "meta":
        full = torch.empty(*shape, dtype=dtype, device="meta")
    else:
        g = torch.Generator(device="cpu").manual_seed(seed)
        full = torch.randn(*shape, generator=g).to(dtype).to(device)
    if transposed:
        return full[:, off:off + rows].t()
    return full[row0:, off:off + inner]


def operands(c, device, seed_a=1, seed_b=2):
    """(a [M, K], b [N, K]) of an entry, asymmetric (different seeds)."""
    dt = DTYPES[c.dtype]
    return (_matrix(c.M, c.K, c.ta, c.a_off, c.a_pad, c.a_row0, dt, device, seed_a),
            _matrix(c.N, c.K, c.tb, c.b_off, c.b_pad, 0, dt, device, seed_b))


def output(c, device, fill=float("nan")):
    """(out [M, N], buffer).  margin: ``out`` is the top-left corner of a [M + 2, ldc] buffer, ldc = N + 8 (bf16) or
    N + 4 (fp32): two spare rows and a spare column block that no edge tile may touch.  ``fill``: a number, or a
    [M, N] tensor whose values ``out`` starts with (the margin is NaN then)."""
    dt = DTYPES[c.out]
    rows, ld = (c.M + 2, c.N + (8 if c.out == "bf16" else 4)) if c.margin else (c.M, c.N)
    if device == "meta":
        buf = torch.empty(rows, ld, dtype=dt, device="meta")
        return buf[:c.M, :c.N], buf
    if isinstance(fill, torch.Tensor):
        buf = torch.full((rows, ld), float("nan"), dtype=dt, device=device)
        buf[:c.M, :c.N] = fill.to(dt)
    else:
        buf = torch.full((rows, ld), fill, dtype=dt, device=device)
    return buf[:c.M, :c.N], buf


def margin_untouched(c, buf, before):
    """Elementwise: the part of ``buf`` outside out[M, N] is bit-identical to ``before`` (a clone taken before the call)."""
    it = torch.int16 if buf.element_size() == 2 else torch.int32
    same = buf.view(it) == before.view(it)
    same[:c.M, :c.N] = True
    return same


def kwargs(c, out=None, bias=None, bias2=None):
    """The keyword arguments of ops.gemm / ops.gemm_plan for an entry."""
    assert (out is None) == c.fresh, c.name
    assert (bias is not None) + (bias2 is not None) == c.bias, c.name
    kw = dict(out=out, bias=bias, bias2=bias2, accumulate=c.accumulate, split_k=c.split_k, max_wg_per_cu=c.max_wg)
    if c.fresh:
        kw["out_dtype"] = DTYPES[c.out]
    return kw


def plan_on_meta(c):
    """The 9-word record of an entry, planned without a device."""
    from edgedict_amd import ops
    a, b = operands(c, "meta")
    out = None if c.fresh else output(c, "meta")[0]
    bs = [torch.empty(c.N, dtype=torch.float32, device="meta") for _ in range(c.bias)] + [None, None]
    if c.lse:       # edgedict_gemm_nt_lse(A, lda, B, ldb, C, ldc, M, N, K, bias, parts): bf16, K-contiguous, one bias
        assert c.dtype == c.out == "bf16" and not (c.ta or c.tb or c.accumulate or c.max_wg) and c.split_k == 1 and c.bias < 2
        _, args, _ = ops._gemm_args(a, b, out, bs[0], None, False, 1, None, 0, dry=True)
        return ops._gemm_plan_record(args, 0, 0, lse=1)
    return ops.gemm_plan(a, b, **kwargs(c, out, bs[0], bs[1]))


# ----------------------------------------------------------------------------------------------------------- the table
# test_gemm_layouts: every layout pair, bias, fp32 output.  (dtype, M, N, K): {(ta, tb): kernel}.  FAST (even id) needs
# each operand's contiguous extent (K when K-contiguous, else its M or N) to be a multiple of 8 (bf16) or 4 (fp32).
_NN, _TN, _NT, _TT = (False, False), (True, False), (False, True), (True, True)
for _dt, _slow in (("f32", 5), ("bf16", 3)):
    _f = _slow + 1
    for (_M, _N, _K), _ids in (
            ((128, 128, 64), {_NN: _f, _TN: _f, _NT: _f, _TT: _f}),
            ((64, 16, 1024), {_NN: _f, _TN: _f, _NT: _f, _TT: _f}),
            ((300, 200, 72), {_NN: _f, _TN: _f if _dt == "f32" else _slow, _NT: _f, _TT: _f if _dt == "f32" else _slow}),
            # (a one-row operand has unit stride both ways: a [8, 1] matrix transposed IS a K-contiguous row)
            ((1, 7, 8), {_NN: _f, _TN: _f, _NT: _slow, _TT: _slow}),
            ((513, 1030, 264), {_NN: _f, _TN: _slow, _NT: _slow, _TT: _slow}),
            ((129, 640, 896), {_NN: _f, _TN: _slow, _NT: _f, _TT: _slow})):
        for (_ta, _tb), _id in _ids.items():
            _case("layouts/%s-%dx%dx%d-%s%s" % (_dt, _M, _N, _K, "nt"[_ta], "nt"[_tb]), _M, _N, _K, _id, dtype=_dt,
                  out="f32", ta=_ta, tb=_tb, bias=1, fresh=True)

# test_gemm_bf16_output_accumulate_and_splitk
_case("splitk/bf16_out", 256, 384, 4096, 10, fresh=True, vendor=2)           # long K, few tiles: the ring kernel
_case("splitk/acc_f32", 256, 384, 4096, 4, out="f32", accumulate=True, vendor=0)
_case("splitk/acc_split8", 256, 384, 4096, 4, out="f32", accumulate=True, split_k=8, split=8, vendor=0)
_case("splitk/store_split5", 256, 384, 4096, 4, out="f32", split_k=5, split=8, vendor=0)

# test_gemm_strided_views_and_second_bias (fp32; b is a column slice of a [640, 896] matrix)
_case("strided/left_cols_two_biases", 77, 640, 640, 6, dtype="f32", b_pad=256, bias=2, fresh=True)
_case("strided/right_cols", 77, 640, 256, 6, dtype="f32", b_off=640, fresh=True)

# test_gemm_nt_direct_to_lds_path: a = full[:, 64:]; store with both biases, then accumulate into bf16
for (_M, _N, _K), _id in (((128, 128, 64), 7), ((1, 8, 64), 7), ((300, 200, 640), 7), ((1029, 2048, 128), 8),
                          ((64 * 33, 4096, 1024), 8), ((130, 136, 4096), 10)):
    _case("nt/%dx%dx%d-store" % (_M, _N, _K), _M, _N, _K, _id, a_off=64, bias=2, margin=True, vendor=0)
    _case("nt/%dx%dx%d-acc" % (_M, _N, _K), _M, _N, _K, _id, a_off=64, accumulate=True, margin=True, vendor=0)
_case("nt/1153x1544x128-store", 1153, 1544, 128, 8, bias=1, margin=True, new=True)   # last tiles: 1 row, 8 columns

# test_large_short_k_product...: >= 512 macro-tiles win before the vendor branch: the persistent ring kernel
_BIG_M = 131072 + 37
_case("bigshortk/whole", _BIG_M, 2048, 640, 12, bias=1, fresh=True, vendor=0)
for _r0 in (0, 70001, _BIG_M - 300):
    _case("bigshortk/rows-%d" % _r0, 300, 2048, 640, 7, a_row0=_r0, bias=1, fresh=True, vendor=0)

# test_gemm_nt256_macro_tile_path: a = full[:, 64:], both biases; row slices of 300 run the 64 x 64-tile kernel
for _M, _N, _K in ((256 * 33 + 37, 4096, 128), (256 * 66 + 1, 2048, 640), (256 * 130, 1000, 192)):
    _case("nt256/%dx%dx%d-whole" % (_M, _N, _K), _M, _N, _K, 12, a_off=64, bias=2, fresh=True, vendor=0)
    for _r0 in (0, 255, _M // 2 + 3, _M - 300):
        _case("nt256/%dx%dx%d-rows-%d" % (_M, _N, _K, _r0), 300, _N, _K, 7, a_off=64, a_row0=_r0, bias=2, fresh=True,
              vendor=0)

# test_gemm_nt256_ring_kernel_full_output: edgedict_gemm_nt_lse (13; 11 with EDGEDICT_GEMM_NT256R=0, asserted there)
for _M, _N, _K, _bias in ((256 * 40, 2048, 640, 1), (256 * 70 + 37, 2048, 640, 1), (256 * 100 + 5, 640, 2048, 0),
                          (256 * 36, 4096, 128, 1), (256 * 80 + 100, 1000, 192, 1), (300, 520, 256, 1)):
    _case("ring_lse/%dx%dx%d" % (_M, _N, _K), _M, _N, _K, 13, bias=_bias, lse=True, vendor=0)
# test_gemm_nt256_one_tile_per_workgroup_kernel_with_bias_by_default_routing
_case("nt256_one_tile/22016x768x128", 256 * 86, 768, 128, 11, bias=1, lse=True, vendor=0)

# test_gemm_nt_small_long_k_ring_path: store, then accumulate into bf16
for (_M, _N, _K), _v in (((768, 1024, 4096), 2), ((1000, 1000, 1024), 0), ((1536, 1024, 4096), 2), ((70, 200, 2048), 0)):
    _case("ring64/%dx%dx%d-store" % (_M, _N, _K), _M, _N, _K, 10, fresh=True, vendor=_v)
    _case("ring64/%dx%dx%d-acc" % (_M, _N, _K), _M, _N, _K, 10, accumulate=True, vendor=_v)

# test_gemm_tn256_weight_gradient_path: dW = dY^T X, dy = full[:, 8:] (row stride M + 8), fp32 out, background form.
# The one whole-tile shape of before (grid = items = 160) ...
_case("tn256/2048x640x9000-acc", 2048, 640, 9000, 14, out="f32", ta=True, tb=True, a_off=8, accumulate=True, split_k=4,
      max_wg=2, split=4, vendor=0)
_case("tn256/2048x640x9000-store", 2048, 640, 9000, 14, out="f32", ta=True, tb=True, a_off=8, split_k=4, max_wg=1,
      fresh=True, split=4, vendor=0)
# ... and the ragged ones: (M, N, K, split_k, slices that run)
TN256_RAGGED = ((4104, 2056, 1031, 1, 1),     # 17 x 17 tiles on 256 CUs: two items per workgroup; last tiles 8 rows / 8 columns
                (264, 1032, 1111, 1, 1),      # second row tile 8 rows, ninth column tile 8 columns
                (520, 520, 2100, 4, 4),       # ragged both ways, four slices of 576, the last one shorter (372 = 11.6 stages)
                (1032, 264, 5003, 4, 4),
                (512, 520, 1024, 8, 4),       # eight slices lowered to four (at least eight 32-k stages each)
                (8, 32768, 1024, 2, 1))       # one 8-row tile (clamp at row 0), 256 column tiles: slices lowered to one
for _M, _N, _K, _s, _run in TN256_RAGGED:
    for _acc in (True, False):
        _case("tn256/%dx%dx%d-%s" % (_M, _N, _K, "acc" if _acc else "store"), _M, _N, _K, 14, out="f32", ta=True, tb=True,
              a_off=8, accumulate=_acc, split_k=_s, max_wg=2, margin=True, split=_run, new=True)
# M % 8 != 0: not for gemm_tn256.hip - the generic kernel's quiet form with the reduce pass
for _acc in (True, False):
    _case("tn256_fallback/1028x264x1031-%s" % ("acc" if _acc else "store"), 1028, 264, 1031, 3, out="f32", ta=True,
          tb=True, a_off=8, accumulate=_acc, split_k=2, max_wg=2, margin=True, split=2, new=True)

# test_gemm_generic_quiet_form_small_weight_gradients: M * N < 2^18, so NOT gemm_tn256.hip (they were listed under it)
for _M, _N, _K, _s, _run in ((512, 256, 4096, 2, 2), (1024, 240, 5003, 4, 4), (264, 648, 1111, 1, 1)):
    _case("quiet_small/%dx%dx%d-acc" % (_M, _N, _K), _M, _N, _K, 4, out="f32", ta=True, tb=True, a_off=8,
          accumulate=True, split_k=_s, max_wg=2, split=_run, vendor=0)
    _case("quiet_small/%dx%dx%d-store" % (_M, _N, _K), _M, _N, _K, 4, out="f32", ta=True, tb=True, a_off=8, split_k=_s,
          max_wg=1, fresh=True, split=_run, vendor=0)

# test_gemm_generic_bf16_output: gemm_kernel<bf16, bf16>, FAST (2) and guarded (1)
_case("generic_bf16/300x200x72-bias", 300, 200, 72, 2, bias=1, margin=True, new=True)
_case("generic_bf16/300x203x72-two_biases", 300, 203, 72, 2, bias=2, margin=True, new=True)     # N % 8: scalar C store
_case("generic_bf16/300x200x72-acc", 300, 200, 72, 2, accumulate=True, margin=True, new=True)
_case("generic_bf16/304x200x256-at-bias", 304, 200, 256, 2, ta=True, bias=1, margin=True, new=True)
_case("generic_bf16/130x72x77-bias", 130, 72, 77, 1, bias=1, margin=True, new=True)             # K tail of 5
_case("generic_bf16/130x72x77-acc", 130, 72, 77, 1, accumulate=True, margin=True, new=True)
# an NT-eligible shape (K = 128) whose A lost its 16-byte alignment: a = full[:, 4:] of a [300, 132] matrix ...
_case("generic_bf16/300x200x128-a_off4", 300, 200, 128, 1, a_off=4, margin=True, new=True)
# ... and of a [300, 136] one, where the leading dimension is still a multiple of 8 and only the pointer is off
_case("generic_bf16/300x200x128-a_off4_ld136", 300, 200, 128, 1, a_off=4, a_pad=4, margin=True, new=True)

# test_gemm_k_tails_fp32_output
_case("ktail/bf16-130x72x77", 130, 72, 77, 3, out="f32", bias=1, margin=True, new=True)
_case("ktail/f32-130x70x13", 130, 70, 13, 5, dtype="f32", bias=1, margin=True, new=True)
_case("ktail/f32-5x3x1", 5, 3, 1, 5, dtype="f32", margin=True, new=True)
_case("ktail/f32-5x7x0-bias", 5, 7, 0, 5, dtype="f32", bias=1, margin=True, new=True)           # K = 0: the bias rows
_case("ktail/f32-5x7x0-acc", 5, 7, 0, 5, dtype="f32", accumulate=True, margin=True, new=True)   # K = 0: unchanged

# test_gemm_split_k_variants
_case("split/bf16-256x384x4096-bias-store", 256, 384, 4096, 4, out="f32", bias=1, split_k=8, margin=True, split=8, new=True)
_case("split/bf16-130x70x4099-store", 130, 70, 4099, 3, out="f32", split_k=8, margin=True, split=8, new=True)
_case("split/f32-130x70x1000-acc", 130, 70, 1000, 6, dtype="f32", accumulate=True, split_k=3, margin=True, split=8, new=True)
_case("split/bf16-130x70x100-clamp", 130, 70, 100, 3, out="f32", split_k=8, margin=True, split=2, new=True)

# test_gemm_background_form_with_the_cap_binding: a, b = [520, 1024].t(); 64 tiles x 8 slices = 512 items
_case("bg/quiet-cap1", 1024, 1024, 520, 4, out="f32", ta=True, tb=True, split_k=8, max_wg=1, margin=True, split=8, new=True)
_case("bg/atomic-bias-cap1", 1024, 1024, 520, 4, out="f32", ta=True, tb=True, bias=1, split_k=8, max_wg=1, margin=True,
      split=8, new=True)
_case("bg/quiet-cap2", 1024, 1024, 520, 4, out="f32", ta=True, tb=True, split_k=8, max_wg=2, margin=True, split=8, new=True)
_case("bg/bf16_out-bias-cap1", 1024, 1024, 520, 2, ta=True, tb=True, bias=1, max_wg=1, margin=True, new=True)
