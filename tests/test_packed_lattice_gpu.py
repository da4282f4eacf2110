"""GPU: the packed-lattice joint + loss chain of the training step (models._JointLossFn), kernel by kernel against the
float64 restatement oracle/packed_ref.py (itself pinned by tests/test_packed_ref_host.py):

    joint_hidden_fwd_packed -> gemm_nt_lse -> rnnt_loss_forward_packed[_parts] -> rnnt_loss_backward_packed[_colsum]
    -> joint_hidden_bwd_packed

Every comparison is element by element over ALL elements of an output; padding is asserted to be exactly zero.  Output
buffers are handed to the kernels full of NaN (a NaN fails every `<=`), and ``hid`` / ``dl`` carry a few sentinel rows
behind row M that must come back untouched: an element a kernel does not write, or a row written past the end, fails.
The comments on the cases say which branch of which kernel each one is there for."""
import ctypes
import math

import pytest
import torch

from oracle import packed_ref as PR

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
BF16_ULP = 2.0 ** -8          # one output rounding, relative to the value (test_layer_kernels_gpu.BF16_ULP)
GUARD, SENT = 4, 768.0        # guard rows behind row M and their (bf16-exact) fill
PATTERNS = ("full", "ragged", "u0", "t1", "cell", "b1")


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _lens(pattern, B, T, U1, seed):
    """(act_lens, label_lens) lists with max == (T, U1 - 1), as _JointLossFn requires; the longest utterance is the
    LAST row, and from three utterances on the longest in frames and the longest in labels are different rows."""
    if pattern == "b1" or B == 1:
        return [T], [U1 - 1]
    if pattern == "full":
        return [T] * B, [U1 - 1] * B
    g = _gen(seed)
    al = torch.randint(1, T + 1, (B,), generator=g).tolist()
    ll = torch.randint(0, U1, (B,), generator=g).tolist()
    al[B - 1], ll[B - 1] = T, U1 - 1
    if B >= 3:
        ll[B - 1], ll[B - 2] = (U1 - 1) // 2, U1 - 1
    if pattern in ("u0", "cell"):
        ll[0] = 0                       # no labels: a box of one column
    if pattern in ("t1", "cell"):
        al[0] = 1                       # one frame; with "cell" a one-cell box
    assert max(al) == T and max(ll) == U1 - 1
    return al, ll


def _dev_lens(al, ll):
    off, m = PR.offsets(al, ll)
    return (torch.tensor(al, dtype=torch.int32).cuda(), torch.tensor(ll, dtype=torch.int32).cuda(), off.cuda(), m)


def _guarded(m, n, dtype):
    """[m + GUARD, n] buffer: NaN where the kernel must write, SENT behind it."""
    buf = torch.full((m + GUARD, n), float("nan"), dtype=dtype, device="cuda")
    buf[m:] = SENT
    return buf


def _guard_ok(buf, m):
    return bool((buf[m:] == SENT).all())


def _inside(al, ll, T, U1):
    ok_t = torch.arange(T)[None, :] < torch.tensor(al)[:, None]           # [B, T]
    ok_u = torch.arange(U1)[None, :] <= torch.tensor(ll)[:, None]         # [B, U1]
    return ok_t, ok_u


# ------------------------------------------------------------------------------------------ a. joint_hidden_fwd_packed
FWD_SHAPES = [
    (2, 5, 3, 8), (3, 11, 21, 72), (2, 37, 80, 136), (4, 9, 65, 640), (1, 1, 1, 64),    # test_joint_gpu.SHAPES, made ragged
    (3, 6, 5, 640),          # bf16: 80 column chunks -> 3 label lanes, 16 idle threads; fp32: 160 chunks, one lane
    (2, 4, 3, "wide"),       # J / VEC == 256 (2048 bf16, 1024 fp32): every thread a chunk, one label lane
    (130, 130, 3, 64),       # B * T = 16900 > the 16384-workgroup cap: second trip of the grid-stride loop over (b, t)
]


def _fwd_bound(ref, dtype):
    # fp32: the dense test's absolute 1e-6; bf16: ONE output rounding (the fast-tanh form is good to ~1e-7 absolute)
    return torch.full_like(ref, 1e-6) if dtype == F32 else BF16_ULP * ref.abs() + 1e-6


def _run_fwd_packed(E1, D1, al, ll):
    from edgedict_amd import _lib
    B, T, J = E1.shape
    U1 = D1.shape[1]
    al_d, ll_d, off_d, m = _dev_lens(al, ll)
    buf = _guarded(m, J, E1.dtype)
    _lib.call("joint_hidden_fwd_packed", _lib.dtype_code(E1.dtype), E1, D1, buf, al_d, ll_d, off_d, B, T, U1, J)
    torch.cuda.synchronize()
    return buf, m


@pytest.mark.parametrize("shape", FWD_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_joint_hidden_fwd_packed(hip_lib, shape, dtype):
    from edgedict_amd import ops
    B, T, U1, J = shape
    if J == "wide":
        J = 1024 if dtype == F32 else 2048
    g = _gen(B * 1000 + T * 100 + U1 + J)
    E1 = torch.randn(B, T, J, generator=g).to(dtype).cuda()
    D1 = torch.randn(B, U1, J, generator=g).to(dtype).cuda()
    # the dense entry point, to the same (for bf16: tightened) bound
    dense = ops.joint_hidden_fwd(E1, D1)
    ref_d = torch.tanh(E1.double()[:, :, None] + D1.double()[:, None])
    assert ((dense.double() - ref_d).abs() <= _fwd_bound(ref_d, dtype)).all()
    dense = dense.cpu()
    for pattern in PATTERNS:
        al, ll = _lens(pattern, B, T, U1, seed=7 + B + T)
        Bp = len(al)                              # "b1": the first utterance alone
        buf, m = _run_fwd_packed(E1[:Bp].contiguous(), D1[:Bp].contiguous(), al, ll)
        assert _guard_ok(buf, m), pattern         # nothing written behind row M
        hid = buf[:m].cpu()
        ref = PR.joint_hidden(E1[:Bp].cpu(), D1[:Bp].cpu(), al, ll)
        assert hid.shape == ref.shape
        bad = ~((hid.double() - ref).abs() <= _fwd_bound(ref, dtype))        # NaN (unwritten) counts as bad
        assert not bad.any(), (pattern, al, ll, bad.nonzero()[:4].tolist())
        # same per-cell arithmetic as the dense kernel: bit for bit
        assert torch.equal(hid, PR.pack(dense[:Bp, :max(al), :max(ll) + 1], al, ll)), pattern


# ------------------------------------------------------------------------------------------ b. joint_hidden_bwd_packed
# the kernel walks the labels in passes of 72 (8 label lanes x 9 positions), J in 64-column blocks, t in slabs
BWD_CASES = {
    # second label pass; row 0's box ends exactly with the first pass (U_b + 1 = 72) while rows 1 and 2 go on; row 3 inside it
    "u80": dict(T=9, U1=80, J=64, al=[9, 4, 9, 1], ll=[71, 79, 72, 30]),
    # third label pass: U_b on both sides of 72 and of 144; a one-cell box last
    "u150": dict(T=5, U1=150, J=72, al=[3, 5, 5, 2, 1], ll=[143, 149, 144, 71, 0]),
    # J = 136: the third 64-column block has one live 8-vector; B small -> 5 slabs of 8 frames, the last one partial
    "j136_slabs": dict(T=37, U1=80, J=136, al=[30, 37], ll=[79, 12]),
    # T = 1: one slab, waves 1..3 have no frame at all
    "t1": dict(T=1, U1=6, J=136, al=[1, 1, 1], ll=[5, 0, 3]),
    # T = 7 < 8: one slab, the waves take one or two frames each
    "t7": dict(T=7, U1=21, J=72, al=[7, 2, 5], ll=[3, 20, 0]),
    # B * (J / 64) = 80 * 16 = 1280 workgroups already: ONE slab of all 37 frames
    "t37_one_slab": dict(T=37, U1=3, J=1024, B=80),
    # the length patterns on the dense test's (3, 11, 21, 72)
    **{"pat_" + p: dict(T=11, U1=21, J=72, B=3, pattern=p) for p in PATTERNS},
}


@pytest.mark.parametrize("name", list(BWD_CASES))
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_joint_hidden_bwd_packed(hip_lib, name, dtype):
    from edgedict_amd import _lib, ops
    c = BWD_CASES[name]
    T, U1, J = c["T"], c["U1"], c["J"]
    if "al" in c:
        al, ll = c["al"], c["ll"]
    else:
        al, ll = _lens(c.get("pattern", "ragged"), c["B"], T, U1, seed=len(name))
    B = len(al)
    assert max(al) == T and max(ll) == U1 - 1
    g = _gen(31 * T + U1 + J + B)
    E1 = torch.randn(B, T, J, generator=g).to(dtype).cuda()
    D1 = torch.randn(B, U1, J, generator=g).to(dtype).cuda()
    buf, m = _run_fwd_packed(E1, D1, al, ll)
    # both operands sit at the front of a NaN-filled buffer of the DENSE capacity: a kernel that walked the packed rows
    # with the dense stride, or past an utterance's last frame, reads NaN (and fails below), not memory behind the tensor
    hid = torch.full((B * T * U1, J), float("nan"), dtype=dtype, device="cuda")
    dhid = torch.full((B * T * U1, J), float("nan"), dtype=dtype, device="cuda")
    hid[:m] = buf[:m]
    dhid[:m] = torch.randn(m, J, generator=g).to(dtype).cuda()
    al_d, ll_d, off_d, _ = _dev_lens(al, ll)
    # _JointLossFn hands the kernel torch.empty buffers: every element must be written, padding included
    dE1 = torch.full((B, T, J), float("nan"), device="cuda")
    dD1 = torch.full((B, U1, J), float("nan"), device="cuda")
    _lib.call("joint_hidden_bwd_packed", _lib.dtype_code(dtype), dhid, hid, dE1, dD1, al_d, ll_d, off_d, B, T, U1, J)
    torch.cuda.synchronize()
    hid, dhid = hid[:m].cpu(), dhid[:m].cpu()
    rE, rD = PR.joint_hidden_bwd(dhid, hid, al, ll, T=T, U1=U1)                  # float64 of the operands as stored
    dE1, dD1 = dE1.cpu().double(), dD1.cpu().double()
    tolE = 1e-4 * max(1.0, rE.abs().max().item())
    tolD = 1e-4 * max(1.0, rD.abs().max().item())
    assert ((dE1 - rE).abs() <= tolE).all(), (name, (dE1 - rE).abs().max().item(), tolE)
    assert ((dD1 - rD).abs() <= tolD).all(), (name, (dD1 - rD).abs().max().item(), tolD)
    ok_t, ok_u = _inside(al, ll, T, U1)
    assert (dE1[~ok_t] == 0).all() and (dD1[~ok_u] == 0).all()         # exact zeros outside the boxes
    # the dense kernel on the zero-filled box layout differs in fp32 summation order only
    dE1d, dD1d = ops.joint_hidden_bwd(PR.unpack(dhid, al, ll, T=T, U1=U1, fill=0.0).cuda(),
                                      PR.unpack(hid, al, ll, T=T, U1=U1, fill=0.0).cuda())
    assert ((dE1d.cpu().double() - dE1).abs() <= tolE).all() and ((dD1d.cpu().double() - dD1).abs() <= tolD).all()


# ------------------------------------------------------------------------------------------ c / d. packed loss
# One lattice for every (V, blank): B = 256 utterances of a [61, 70] slab, so that rnnt_lse_from_parts gets
# grid.x = min(ceil(T U1 / 256), 256 * 16 / B) = 16 workgroups per utterance = 4096 rows per grid-stride pass (2048 on
# the 32-row staging path) and the one long utterance (61 x 70 = 4270 cells) needs a SECOND pass, whose last wave gets
# a partial block of rows (nrows < step).  U1 = 70 > 64 is the two-columns-per-lane alpha / beta kernel.
LOSS_B, LOSS_T, LOSS_U1, LOSS_J = 256, 61, 70, 128
LOSS_V = [264,      # slots 5: odd -> 8-byte loads, no staging; rows of 528 bytes; colsum in both dtypes
          1000,     # slots 16 (the last one 40 columns wide): 64 rows per wave staged through LDS
          2048,     # slots 32: the bench's path; colsum limit in bf16
          4096,     # slots 64: 32 rows per wave staged
          4608]     # slots 72: direct 16-byte loads


def _loss_lens():
    g = _gen(5)
    al = torch.randint(1, 4, (LOSS_B,), generator=g).tolist()          # the crowd: boxes of 1 .. 9 cells
    ll = torch.randint(0, 3, (LOSS_B,), generator=g).tolist()
    al[0], ll[0] = 5, 4            # 25 cells: fewer than 32
    al[1], ll[1] = 10, 6           # 70 cells: not a multiple of 64
    al[2], ll[2] = 1, 0            # one cell
    al[3], ll[3] = 7, 0            # no labels
    al[4], ll[4] = 1, 30           # one frame
    al[200], ll[200] = LOSS_T, LOSS_U1 - 1     # the long one, not row 0
    return al, ll


def _cell_index(al, ll, T, U1):
    """dense cell index (b T + t) U1 + u of every packed row."""
    out = []
    for b, (t, u) in enumerate(zip(al, ll)):
        out.append(((b * T + torch.arange(t))[:, None] * U1 + torch.arange(u + 1)[None, :]).reshape(-1))
    return torch.cat(out)


def _denominators(lib, ws, B, T, U1, cells):
    base = ws.data_ptr()
    p = lib.edgedict_rnnt_workspace_view(ctypes.c_void_p(base), B, T, U1, 0)
    n = B * T * U1
    return ws[p - base:p - base + 4 * n].view(torch.float32)[cells]


@pytest.mark.parametrize("blank", [0, 5, -1], ids=["blank0", "blank5", "blankV-1"])
@pytest.mark.parametrize("V", LOSS_V)
def test_packed_loss_forward_and_backward(hip_lib, V, blank):
    """c. the three forward routes and d. the gradient kernels on one set of logits - those the logits product wrote -
    against ONE float64 run of the oracle on the logits as stored."""
    from edgedict_amd import _lib
    from edgedict_amd.ops import _ll
    lib = hip_lib
    B, T, U1, J = LOSS_B, LOSS_T, LOSS_U1, LOSS_J
    blank = V - 1 if blank < 0 else blank
    al, ll = _loss_lens()
    al_d, ll_d, off_d, M = _dev_lens(al, ll)
    grid = min((T * U1 + 255) // 256, max(1, 256 * 16 // B))         # ed_grid_for(T * U1, 256, 256 * 16 / B)
    cells = [t * (u + 1) for t, u in zip(al, ll)]
    assert max(cells) > grid * 256 and (max(cells) - grid * 256) % 64 != 0      # second pass, with a partial last block
    assert min(cells) == 1 and 25 in cells and 70 in cells
    g = _gen(V + blank)
    hid = torch.tanh(torch.randn(M, J, generator=g)).to(BF16).cuda()
    w2 = (torch.randn(V, J, generator=g) / 4).to(BF16).cuda()
    b2 = torch.randn(V, generator=g).cuda()
    r = torch.randint(0, V - 1, (B, U1 - 1), generator=g, dtype=torch.int32)
    labels = (r + (r >= blank).int()).cuda()                         # any id but the blank: ids BELOW a blank of 5 occur
    slots = (V + 63) // 64
    parts = torch.full((M, slots, 2), float("nan"), device="cuda")
    logits_bf = torch.full((M, V), float("nan"), dtype=BF16, device="cuda")
    _lib.call("gemm_nt_lse", hid, _ll(J), w2, _ll(J), logits_bf, _ll(V), M, V, J, b2, parts)
    torch.cuda.synchronize()
    assert torch.isfinite(logits_bf).all()
    logits_f = logits_bf.float()                                     # the same values for the fp32 route
    ref_costs, ref_grads = PR.loss_from_packed_logits(logits_f.cpu(), labels.cpu(), al, ll, blank=blank)
    ref_grads = ref_grads.cuda()
    ref_den = logits_bf.double().logsumexp(dim=1)
    cell_idx = _cell_index(al, ll, T, U1).cuda()
    ws_bytes = lib.edgedict_rnnt_workspace_bytes(B, T, U1)

    # ---- c. forward: fp32 logits, bf16 logits, bf16 logits + the product's log-sum-exp partials
    ws = {}
    for route, rtol in (("f32", 1e-5), ("bf16", 1e-4), ("parts", 1e-4)):
        w = ws[route] = torch.full((ws_bytes,), 0xFF, dtype=torch.uint8, device="cuda")     # NaN wherever nothing is written
        costs = torch.full((B,), float("nan"), device="cuda")
        red = torch.full((1,), float("nan"), device="cuda")
        if route == "parts":
            _lib.call("rnnt_loss_forward_packed_parts", logits_bf, labels, al_d, ll_d, off_d, B, T, U1, V, blank,
                      costs, red, 1.0 / B, w, parts, slots)
        else:
            lg, code = (logits_f, 0) if route == "f32" else (logits_bf, 1)
            _lib.call("rnnt_loss_forward_packed", lg, code, labels, al_d, ll_d, off_d, B, T, U1, V, blank,
                      costs, red, 1.0 / B, w)
        torch.cuda.synchronize()
        den = _denominators(lib, w, B, T, U1, cell_idx)
        err = (den.double() - ref_den).abs()
        assert (err <= 2e-5).all(), (route, err.max().item(), int((~(err <= 2e-5)).nonzero()[0]))
        cerr = (costs.cpu().double() - ref_costs).abs()
        assert (cerr <= rtol * ref_costs.abs()).all(), (route, (cerr / ref_costs.abs()).max().item())
        want = costs.cpu().double().sum().item() / B
        assert abs(red.item() - want) <= 1e-6 * abs(want), (route, red.item(), want)

    # ---- d. backward: every element of dl against the float64 gradient x scale / B
    scale_vec = torch.linspace(0.2, 1.7, B)                          # distinct per utterance
    rows_b = torch.repeat_interleave(torch.arange(B), torch.tensor(cells))       # utterance of every packed row
    modes = {"none": (None, 0, torch.ones(B)),
             "scalar": (torch.tensor([0.37]).cuda(), 0, torch.full((B,), 0.37)),     # what _JointLossFn passes
             "vector": (scale_vec.cuda(), 1, scale_vec)}
    for route, dtype, code in (("f32", F32, 0), ("bf16", BF16, 1), ("parts", BF16, 1)):
        lg = logits_f if dtype == F32 else logits_bf
        n_cs = lib.edgedict_rnnt_grad_colsum_rows(code, B, T, U1, V)
        assert (n_cs > 0) == (V * (4 if dtype == F32 else 2) % 16 == 0 and V <= (1024 if dtype == F32 else 2048))
        for mode, (sdev, stride, svals) in modes.items():
            if route == "parts" and mode != "scalar":
                continue                                             # the training step's own combination, once
            s_row = (svals.double() / B)[rows_b].cuda()[:, None]     # total scale of every row
            want = ref_grads * s_row
            # the bounds the dense tests hold this kernel to, times the gradient scale
            tol = (1e-3 * want.abs() + 2e-5 * s_row) if dtype == F32 else 4e-3 * s_row
            buf = _guarded(M, V, dtype)
            _lib.call("rnnt_loss_backward_packed", lg, code, buf, labels, al_d, ll_d, off_d, B, T, U1, V, blank,
                      ws[route], 1.0 / B, sdev, stride)
            torch.cuda.synchronize()
            assert _guard_ok(buf, M), (route, mode)
            bad = ~((buf[:M].double() - want).abs() <= tol)
            assert not bad.any(), (route, mode, bad.nonzero()[:4].tolist())
            if n_cs <= 0:
                continue
            cs = torch.full((n_cs, V), float("nan"), device="cuda")
            fused = _guarded(M, V, dtype)
            _lib.call("rnnt_loss_backward_packed_colsum", lg, code, fused, labels, al_d, ll_d, off_d, B, T, U1, V,
                      blank, ws[route], 1.0 / B, sdev, stride, cs)
            torch.cuda.synchronize()
            assert _guard_ok(fused, M) and torch.equal(fused[:M], buf[:M]), (route, mode)
            got = cs.double().sum(0)
            ctol = 1e-5 if dtype == F32 else 2.0 ** -8               # test_fused_column_sums_of_the_gradient's criterion
            assert ((got - want.sum(0)).abs() <= ctol * want.abs().sum(0) + 1e-12).all(), (route, mode)


# ------------------------------------------------------------------------------------------ e. _JointLossFn end to end
E_P = 24
E_LATTICES = {
    "m344": dict(T=20, U1=10, al=[7, 20, 1, 13, 20, 2], ll=[9, 4, 0, 0, 6, 9]),        # M = 344 >= 256
    "m88": dict(T=9, U1=6, al=[9, 1, 4, 9], ll=[2, 0, 5, 3]),                          # M = 88 < 256
}
# (lattice, J, V): which side of FUSED_LSE (bf16 only: J >= 128 and J % 64 == 0 and V % 8 == 0 and M >= 256) runs
E_CASES = [("m344", 128, 264, True), ("m344", 136, 264, False), ("m344", 640, 2048, True), ("m88", 128, 264, False)]
E_OUTPUTS = ("denc", "ddec", "dW1", "db1", "dW2", "db2", "costs")
# bf16: max |got - ref| / max |ref| per output, the largest over E_CASES as measured on an MI355X (see the docstring)
E_BF16_MEASURED = dict(denc=5.4e-3, ddec=3.0e-3, dW1=4.9e-3, db1=8.9e-4, dW2=3.0e-3, db2=1.1e-5, costs=2.0e-4)
E_GOUT = 0.37                  # the upstream gradient: reaches the loss-gradient kernel as its device-side scale


def _joint_loss_case(lattice, J, V, dtype, blank):
    from edgedict_amd import _lib, config, ops
    from edgedict_amd.models import _JointLossFn
    lat = E_LATTICES[lattice]
    T, U1, al, ll = lat["T"], lat["U1"], lat["al"], lat["ll"]
    B, P = len(al), E_P
    g = _gen(J + V + T)
    rnd = lambda *s: torch.randn(*s, generator=g)
    enc = rnd(B, T, P).to(dtype).cuda().requires_grad_(True)
    dec = rnd(B, U1, P).to(dtype).cuda().requires_grad_(True)
    w1 = torch.nn.Parameter((rnd(J, 2 * P) / math.sqrt(2 * P)).cuda())
    b1 = torch.nn.Parameter((0.1 * rnd(J)).cuda())
    w2 = torch.nn.Parameter((rnd(V, J) / math.sqrt(J)).cuda())
    b2 = torch.nn.Parameter((0.1 * rnd(V)).cuda())
    r = torch.randint(0, V - 1, (B, U1 - 1), generator=g, dtype=torch.int32)
    labels = r + (r >= blank).int()
    ops.TIMERS = {}
    try:
        loss = _JointLossFn.apply(enc, dec, w1, b1, w2, b2, labels.cuda(), torch.tensor(al, dtype=torch.int32),
                                  torch.tensor(ll, dtype=torch.int32), blank, dtype)
        costs = ops.LAST["joint_costs"].detach().double().cpu()
        loss.backward(torch.full_like(loss, E_GOUT))
        torch.cuda.synchronize()
        timers = set(ops.timer_summary())
    finally:
        ops.TIMERS = None
    got = dict(denc=enc.grad, ddec=dec.grad, dW1=w1.grad, db1=b1.grad, dW2=w2.grad, db2=b2.grad)
    got = {k: v.detach().double().cpu() for k, v in got.items()}
    got["costs"] = costs
    # float64 autograd through packed_ref on the operands as the kernels see them
    e64 = enc.detach().double().cpu().requires_grad_(True)
    d64 = dec.detach().double().cpu().requires_grad_(True)
    w1_64 = w1.detach().to(dtype).double().cpu().requires_grad_(True)
    w2_64 = w2.detach().to(dtype).double().cpu().requires_grad_(True)
    b1_64 = b1.detach().double().cpu().requires_grad_(True)
    b2_64 = b2.detach().double().cpu().requires_grad_(True)
    hid = PR.joint_hidden(e64 @ w1_64[:, :P].t(), d64 @ w1_64[:, P:].t() + b1_64, al, ll)
    logits = hid @ w2_64.t() + b2_64
    rcosts, dlogits = PR.loss_from_packed_logits(logits, labels, al, ll, blank=blank)
    logits.backward(dlogits * (E_GOUT / B))
    ref = dict(denc=e64.grad, ddec=d64.grad, dW1=w1_64.grad, db1=b1_64.grad, dW2=w2_64.grad, db2=b2_64.grad, costs=rcosts)
    cs_rows = _lib.load().edgedict_rnnt_grad_colsum_rows(_lib.dtype_code(dtype), B, T, U1, V)
    info = dict(fused_lse="rnnt_loss_fwd" in timers, fused_db2=bool(config.FUSED_DB2 and cs_rows > 0), timers=timers,
                al=al, ll=ll, T=T, U1=U1)
    return got, ref, info


def _e_errors(got, ref):
    return {k: (got[k] - ref[k]).abs().max().item() / ref[k].abs().max().item() for k in E_OUTPUTS}


def _e_zeros(got, info):
    ok_t, ok_u = _inside(info["al"], info["ll"], info["T"], info["U1"])
    assert (got["denc"][~ok_t] == 0).all() and (got["ddec"][~ok_u] == 0).all()        # exact zeros for t >= T_b / u > U_b


@pytest.mark.parametrize("lattice,J,V,fused", E_CASES)
def test_joint_loss_fn_fp32(hip_lib, lattice, J, V, fused):
    """fp32: every output within 2e-5 * max |ref| (test_packed_lattice_path_matches_golden_loss_and_dense_gradients'
    bound, here against float64 and per element).  fp32 never takes the fused log-sum-exp route; V = 2048 is above the
    fp32 limit of the fused column sums (1024), V = 264 below: both sides of FUSED_DB2."""
    got, ref, info = _joint_loss_case(lattice, J, V, F32, blank=5)
    assert not info["fused_lse"] and {"joint_hidden_fwd", "joint_logits_gemm", "rnnt_grad", "joint_hidden_bwd"} <= info["timers"]
    assert info["fused_db2"] == (V <= 1024)
    errs = _e_errors(got, ref)
    print("joint_loss_fn fp32", lattice, J, V, {k: "%.3g" % v for k, v in errs.items()})
    for k in E_OUTPUTS:
        assert ((got[k] - ref[k]).abs() <= 2e-5 * ref[k].abs().max()).all(), (k, errs[k])
    _e_zeros(got, info)


@pytest.mark.parametrize("lattice,J,V,fused", E_CASES)
def test_joint_loss_fn_bf16(hip_lib, lattice, J, V, fused):
    """bf16: every output within 4 x the error measured on an MI355X against the float64 reference,
    max |got - ref| / max |ref| per output, the largest over the four cases (E_BF16_MEASURED; DESIGN_APPENDIX.md):

        case               denc     ddec     dW1      db1      dW2      db2      costs
        m344 J128 V264     4.2e-3   2.7e-3   4.9e-3   6.4e-4   1.9e-3   5.8e-6   9.0e-5     (fused log-sum-exp)
        m344 J136 V264     2.7e-3   2.8e-3   4.8e-3   8.0e-4   3.0e-3   5.3e-6   1.9e-4
        m344 J640 V2048    5.1e-3   2.4e-3   3.1e-3   8.8e-4   2.8e-3   1.4e-6   9.0e-5     (fused log-sum-exp)
        m88  J128 V264     5.3e-3   3.0e-3   2.0e-3   7.1e-4   1.6e-3   1.1e-5   1.8e-4

    denc / ddec stay below 2^-6 = 1.6e-2 (two bf16 roundings of an O(1)-scaled sum); db2 comes from the fp32 column
    sums the gradient kernel takes in front of its store, so it carries no output rounding at all.

    4 x keeps one more bit of head-room for the seed-dependent rounding of re-ordered fp32 sums and stays far below
    the 6e-2 norm-relative bound of test_e6d2_parity_gpu."""
    got, ref, info = _joint_loss_case(lattice, J, V, BF16, blank=5)
    assert info["fused_lse"] == fused, sorted(info["timers"])        # which side of the FUSED_LSE condition ran
    assert info["fused_db2"]                                         # V <= 2048: the fused column sums in every bf16 case
    errs = _e_errors(got, ref)
    print("joint_loss_fn bf16", lattice, J, V, {k: "%.3g" % v for k, v in errs.items()})
    for k in E_OUTPUTS:
        assert ((got[k] - ref[k]).abs() <= 4 * E_BF16_MEASURED[k] * ref[k].abs().max()).all(), (k, errs[k])
    _e_zeros(got, info)
