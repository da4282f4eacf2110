"""GPU: the RNN-T lattice walks rnnt_alpha_beta<C, VIT> (csrc/rnnt_loss.hip) at EVERY columns-per-lane variant the
dispatcher can pick, against the float64 oracle (oracle/rnnt_loss_ref.py), and the one label limit on both sides.

    U1 = U + 1     C    D (ring)   reached here by                                   and by
    1 .. 64        1    8          U1 = 64                                           almost every loss test
    65 .. 128      2    8          U1 = 65, 128                                      test_rnnt_loss_gpu (70), test_rnnt_align_gpu (70)
    129 .. 256     4    4          U1 = 129, 256                                     test_long_lattice_drift_is_bounded (201),
                                                                                     test_band_gpu (150), test_rnnt_align_gpu (129)
    257 .. 512     8    2          U1 = 257, 512; ring phase (c) at 257              test_rnnt_align_gpu (257)
    513 .. 1024    16   1          U1 = 513, 1024; ring phase (c), FastEmit and      test_rnnt_align_gpu (513, 1024)
                                   windows at 513
    1025 ..        -    -          refused before any launch (test_label_limit_*)

Every U1 above runs (a) cost and gradient by five routes - test_cost_and_gradient_match_fp64 - and (b) the alpha and
beta planes themselves - test_lattices_match_fp64.  The Viterbi instantiations (VIT = true) are tests/
test_rnnt_align_gpu.py's, on the same batches (tests/rnnt_walk_cases.py).

All bounds are the project's own: fp32 cost 2e-6 relative (test_long_lattice_drift_is_bounded, a chain of 1200
log-adds - longer than any here), fp32 gradient rtol 1e-3 / atol 2e-5 (test_fp32_matches_oracle), bf16 cost rtol 1e-4
and gradient atol 4e-3 with the oracle seeing the bf16-rounded logits (test_bf16_logits), the partials route's cost
within 1e-6 relative of the packed route's on the same logits (test_fused_lse_epilogue_matches_separate_pass), lattice
cells 1e-4 (test_debug_views_alpha_beta) + 2e-6 relative, the two likelihoods within 1e-5 relative of each other
(test_full_size_lattice_properties)."""
import functools

import numpy as np
import pytest
import torch

import arloss_ref as AR
import fastemit_ref as FR
import rnnt_walk_cases as WC
from oracle import packed_ref as PR
from oracle import rnnt_loss_ref as R

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
T, B = WC.T_WALK, WC.B_WALK
# (U1, V): V = 8 is one 16-byte vector per row in bf16 and two in fp32; V = 5 takes the scalar row path
SHAPES = [(U1, 8) for U1 in WC.U1_WALK] + [(513, 5)]
ROUTES = [("dense", F32), ("dense", BF16), ("packed", F32), ("packed", BF16), ("parts", BF16)]
ROUTE_IDS = [r + "-" + ("f32" if d == F32 else "bf16") for r, d in ROUTES]


def _shape_id(s):
    return "U1=%d-V=%d" % s


def _dev(a, dtype=torch.int32):
    return torch.tensor(np.asarray(a), dtype=dtype, device="cuda").contiguous()


@functools.lru_cache(maxsize=None)
def _inputs(U1, V):
    """fp32 logits [B, T, U1, V] (numpy), labels, lengths: the longest utterance is row 3 at every second U1."""
    rng = np.random.default_rng(1000 * U1 + V)
    acts = (2.0 * rng.normal(size=(B, T, U1, V))).astype(np.float32)
    labels = rng.integers(1, V, size=(B, U1 - 1)).astype(np.int32)
    rotate = 3 if WC.U1_WALK.index(U1) % 2 else 0
    al, ll = WC.length_rows(T, U1, rotate)
    assert (int(np.argmax(al * (ll + 1))) != 0) == bool(rotate)
    return acts, labels, al, ll


@functools.lru_cache(maxsize=None)
def _reference(U1, V, dtype):
    """The float64 oracle on the logits as the kernels see them (bf16: rounded first), computed once per case and never
    modified: costs [B] (numpy), gradient of their sum [B, T, U1, V] (torch float64, zeros outside the boxes)."""
    acts, labels, al, ll = _inputs(U1, V)
    seen = torch.tensor(acts).to(dtype).double()
    costs, grads = R.rnnt_loss_torch_fast(seen, torch.tensor(labels), torch.tensor(al), torch.tensor(ll), blank=0)
    assert torch.isfinite(costs).all() and torch.isfinite(grads).all()
    return costs.numpy(), grads


def _run_dense(acts, labels, al, ll, dtype, blank=0, check_lengths=True, **kw):
    """(costs [B], gradient) of RNNTLoss(reduction='none') on the device; kw: fastemit_lambda."""
    from edgedict_amd.loss import RNNTLoss
    windows = kw.pop("windows", None)
    ta = torch.tensor(acts, device="cuda").to(dtype).requires_grad_(True)
    loss = RNNTLoss(blank=blank, reduction="none", check_lengths=check_lengths, **kw)(
        ta, _dev(labels), _dev(al), _dev(ll), windows=windows)
    loss.sum().backward()
    return loss.detach().clone(), ta.grad


def _run_packed(acts, labels, al, ll, dtype, parts):
    """(costs [B], packed gradient [M, V]) through the C ABI; every output starts NaN-filled and must be written."""
    from edgedict_amd import _lib
    from test_rnnt_align_gpu import _lse_parts
    Bn, Tn, U1, V = acts.shape
    off, M = PR.offsets(al, ll)
    packed = PR.pack(torch.tensor(acts).to(dtype), al, ll).cuda().contiguous()
    lab_d, al_d, ll_d, off_d = _dev(labels), _dev(al), _dev(ll), off.cuda()
    ws = torch.full((_lib.load().edgedict_rnnt_workspace_bytes(Bn, Tn, U1),), 0xFF, dtype=torch.uint8, device="cuda")
    costs = torch.full((Bn,), float("nan"), device="cuda")
    red = torch.full((1,), float("nan"), device="cuda")
    if parts:
        lse, slots = _lse_parts(packed)
        _lib.call("rnnt_loss_forward_packed_parts", packed, lab_d, al_d, ll_d, off_d, Bn, Tn, U1, V, 0, costs, red, 1.0,
                  ws, lse, slots)
    else:
        _lib.call("rnnt_loss_forward_packed", packed, _lib.dtype_code(dtype), lab_d, al_d, ll_d, off_d, Bn, Tn, U1, V, 0,
                  costs, red, 1.0, ws)
    grads = torch.full_like(packed, float("nan"))
    _lib.call("rnnt_loss_backward_packed", packed, _lib.dtype_code(dtype), grads, lab_d, al_d, ll_d, off_d, Bn, Tn, U1, V,
              0, ws, 1.0, None, 0)
    torch.cuda.synchronize()
    assert grads.shape == (M, V)
    assert torch.isfinite(costs).all() and torch.isfinite(red).all(), (costs, red)
    assert torch.isfinite(grads.float()).all(), "packed gradient rows left unwritten"
    # `reduced`: an fp32 sum of B positive costs in some order, each addition within 2^-24 relative of the total
    assert abs(red.item() - costs.double().sum().item()) <= Bn * 2.0 ** -23 * abs(red.item())
    return costs, grads


def _check(what, cost, g, costs, grads, dtype):
    """the module docstring's bounds; every figure is printed before it is asserted"""
    cost = cost.double().cpu().numpy()
    err_c = np.abs(cost - costs) / np.abs(costs)
    err = (g.double().cpu() - grads).abs()
    if dtype == F32:
        excess = (err - 1e-3 * grads.abs()).max().item()
        print("walks", what, "f32 cost rel err %.3g (bound 2e-6), gradient max err %.3g, max err - 1e-3 |g| %.3g "
              "(bound 2e-5)" % (err_c.max(), err.max().item(), excess))
        assert (err_c <= 2e-6).all(), (what, cost, costs)
        assert (err <= 1e-3 * grads.abs() + 2e-5).all(), (what, err.max().item())
    else:
        print("walks", what, "bf16 cost rel err %.3g (bound 1e-4), gradient max err %.3g (bound 4e-3)"
              % (err_c.max(), err.max().item()))
        assert (err_c <= 1e-4).all(), (what, cost, costs)
        assert (err <= 4e-3).all(), (what, err.max().item())


# ------------------------------------------------------------------------------------ (a) cost and gradient, five routes
@pytest.mark.parametrize("U1,V", SHAPES, ids=[_shape_id(s) for s in SHAPES])
@pytest.mark.parametrize("route,dtype", ROUTES, ids=ROUTE_IDS)
def test_cost_and_gradient_match_fp64(hip_lib, route, dtype, U1, V):
    acts, labels, al, ll = _inputs(U1, V)
    costs, grads = _reference(U1, V, dtype)
    what = "%s %s C=%d D=%d" % (route, _shape_id((U1, V)), *WC.variant(U1))
    if route == "dense":
        cost, g = _run_dense(acts, labels, al, ll, dtype)
        _check(what, cost, g, costs, grads, dtype)
        for b in range(B):       # rows behind act_lens, columns behind label_lens: exact zeros
            assert int(al[b]) == T or (g[b, int(al[b]):] == 0).all(), b
            assert int(ll[b]) == U1 - 1 or (g[b, :, int(ll[b]) + 1:] == 0).all(), b
        return
    cost, g = _run_packed(acts, labels, al, ll, dtype, parts=route == "parts")
    _check(what, cost, g, costs, PR.pack(grads, al, ll), dtype)
    if route == "parts":
        # the same logits by the pass over them: denominators in another summation order only
        cost_p, _ = _run_packed(acts, labels, al, ll, dtype, parts=False)
        rel = ((cost - cost_p).abs() / cost_p.abs()).max().item()
        print("walks", what, "partials against the pass over the logits: cost rel diff %.3g (bound 1e-6)" % rel)
        assert ((cost - cost_p).abs() <= 1e-6 * cost_p.abs()).all(), (cost, cost_p)


# ------------------------------------------------------------------------------------ (b) the lattices themselves
@pytest.mark.parametrize("U1", WC.U1_WALK)
def test_lattices_match_fp64(hip_lib, U1):
    """Every alpha and beta inside every box, so that a wrong column, lane or ring slot is named directly."""
    from edgedict_amd.loss import rnnt_loss_debug
    V = 8
    acts, labels, al, ll = _inputs(U1, V)
    C, D = WC.variant(U1)
    _, _, alphas, betas, lls = rnnt_loss_debug(torch.tensor(acts, device="cuda"), _dev(labels), _dev(al), _dev(ll))
    alphas, betas, lls = alphas.cpu().numpy(), betas.cpu().numpy(), lls.cpu().numpy()
    for b in range(B):
        Tb, Ub = int(al[b]), int(ll[b])
        lp = R.log_softmax(acts[b, :Tb, :Ub + 1].astype(np.float64))
        alpha, beta, loglike = R.lattice(lp, labels[b], Tb, Ub)
        for name, got, want in (("alpha", alphas[b, :Tb, :Ub + 1], alpha), ("beta", betas[b, :Tb, :Ub + 1], beta)):
            excess = np.abs(got - want) - (1e-4 + 2e-6 * np.abs(want))
            t, u = np.unravel_index(np.argmax(excess), excess.shape)
            col = u if name == "alpha" else Ub - u              # beta's columns are counted from the right
            print("walks lattice U1=%d C=%d D=%d row %d (T_b=%d, U_b=%d) %s: max |err| %.3g, worst cell (t=%d, u=%d) = lane "
                  "%d slot %d" % (U1, C, D, b, Tb, Ub, name, np.abs(got - want).max(), t, u, col // C, col % C))
            assert (excess <= 0).all(), (name, b, int(t), int(u), got[t, u], want[t, u])
        assert abs(lls[b, 0] - lls[b, 1]) <= 1e-5 * abs(lls[b, 0]), (b, lls[b])
        assert abs(lls[b, 0] - loglike) <= 2e-6 * abs(loglike), (b, lls[b], loglike)
        assert abs(lls[b, 1] - loglike) <= 2e-6 * abs(loglike), (b, lls[b], loglike)


# ------------------------------------------------------------------------------------ (c) another ring phase, same bits
@pytest.mark.parametrize("U1", [257, 513])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_trailing_padding_frames_change_no_bit(hip_lib, dtype, U1):
    """1, 2 and 3 frames behind every act_lens: the workspace's frame stride and the grids change, no cell's
    arithmetic does - costs and gradients inside the old tensor bit for bit, exact zeros in the new frames."""
    V = 8
    acts, labels, al, ll = _inputs(U1, V)
    cost0, g0 = _run_dense(acts, labels, al, ll, dtype)
    rng = np.random.default_rng(U1)
    for pad in (1, 2, 3):
        more = np.concatenate([acts, (2.0 * rng.normal(size=(B, pad, U1, V))).astype(np.float32)], axis=1)
        cost, g = _run_dense(more, labels, al, ll, dtype, check_lengths=False)
        assert torch.equal(cost, cost0), (pad, cost, cost0)
        assert torch.equal(g[:, :T], g0), pad
        assert (g[:, T:] == 0).all(), pad


# ------------------------------------------------------------------------------------ (d) a blank other than 0
@pytest.mark.parametrize("Bn,Tn,U1,V", [(3, 7, 5, 11), (2, 9, 6, 16)], ids=["scalar-rows", "vector-rows"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("where", ["last", "middle"])
def test_nonzero_blank_on_the_dense_operator_and_the_aligner(hip_lib, where, dtype, Bn, Tn, U1, V):
    """Bounds: test_fp32_matches_oracle's (cost rtol 1e-5 / atol 1e-4, gradient rtol 1e-3 / atol 2e-5),
    test_bf16_logits' (cost rtol 1e-4, gradient atol 4e-3), the aligner's own (test_rnnt_align_gpu._close)."""
    from edgedict_amd.loss import rnnt_align
    from test_rnnt_align_gpu import _close
    blank = V - 1 if where == "last" else V // 2
    rng = np.random.default_rng(100 * V + blank)
    acts = rng.normal(size=(Bn, Tn, U1, V)).astype(np.float32)
    labels = rng.integers(0, V - 1, size=(Bn, U1 - 1)).astype(np.int32)
    labels[labels >= blank] += 1                                     # every symbol but the blank
    labels[0, 0] = 0                                                 # symbol 0, the blank of every other dense test
    assert (labels != blank).all()
    al = rng.integers(1, Tn + 1, size=Bn).astype(np.int32)
    ll = rng.integers(0, U1, size=Bn).astype(np.int32)
    al[0], ll[0] = Tn, U1 - 1
    seen = torch.tensor(acts).to(dtype).double().numpy()
    costs, grads = R.rnnt_loss(seen, labels, al, ll, blank=blank)
    cost, g = _run_dense(acts, labels, al, ll, dtype, blank=blank)
    cost, g = cost.cpu().numpy(), g.float().cpu().numpy()
    print("walks blank %d %s %s: cost max err %.3g, gradient max err %.3g"
          % (blank, dtype, (Bn, Tn, U1, V), np.abs(cost - costs).max(), np.abs(g - grads).max()))
    if dtype == F32:
        np.testing.assert_allclose(cost, costs, rtol=1e-5, atol=1e-4)
        np.testing.assert_allclose(g, grads, rtol=1e-3, atol=2e-5)
    else:
        np.testing.assert_allclose(cost, costs, rtol=1e-4)
        np.testing.assert_allclose(g, grads, atol=4e-3)
    frames, scores = rnnt_align(torch.tensor(acts, device="cuda").to(dtype), _dev(labels), _dev(al), _dev(ll), blank)
    frames, scores = frames.cpu().numpy(), scores.cpu().numpy()
    for b in range(Bn):
        Tb, Ub = int(al[b]), int(ll[b])
        lpb, lpl = FR.cell_logprobs(seen[b], labels[b], Tb, Ub, blank=blank)
        best, _ = FR.viterbi_one(lpb, lpl)
        fr = frames[b]
        assert (fr[Ub:] == -1).all(), (b, fr)
        assert (fr[:Ub] >= 0).all() and (fr[:Ub] < Tb).all() and (np.diff(fr[:Ub]) >= 0).all(), (b, fr)
        assert _close(float(scores[b]), best, dtype), (b, scores[b], best)
        assert _close(FR.path_score(lpb, lpl, fr[:Ub]), best, dtype), (b, fr, best)
        assert scores[b] <= -cost[b] + 1e-4 * abs(cost[b])


# ------------------------------------------------------------------------------------ the two kernel flags on the long axis
def test_fastemit_gradient_on_the_long_axis(hip_lib):
    """*_fe at U1 = 513 (C = 16, D = 1), lambda = 0.01; tests/test_fastemit_gpu.py's bounds."""
    U1, V, lam = 513, 8, 0.01
    acts, labels, al, ll = _inputs(U1, V)
    costs, grads = FR.fastemit_loss(acts.astype(np.float64), labels, al, ll, lam)
    cost, g = _run_dense(acts, labels, al, ll, F32, fastemit_lambda=lam)
    cost0, g0 = _run_dense(acts, labels, al, ll, F32)
    assert torch.equal(cost, cost0) and not torch.equal(g, g0)       # the costs stay the plain ones
    err = np.abs(g.double().cpu().numpy() - grads)
    print("walks fastemit U1=513: gradient max err %.3g" % err.max())
    np.testing.assert_allclose(cost.cpu().numpy(), costs, rtol=1e-5, atol=1e-4)
    assert (err <= (1 + lam) * (1e-3 * np.abs(grads) + 2e-5)).all(), err.max()


def test_alignment_windows_on_the_long_axis(hip_lib):
    """*_ar at U1 = 513: windows of 2 frames either side of a random alignment; tests/test_arloss_gpu.py's bounds."""
    U1, V = 513, 8
    acts, labels, al, ll = _inputs(U1, V)
    rng = np.random.default_rng(513)
    frames = AR.random_alignment(rng, al, ll, U1 - 1)
    lo, hi = AR.windows_from_frames(frames, al, ll, 2, 2, Tm=T)
    costs, grads, live = AR.ar_loss(acts.astype(np.float64), labels, al, ll, lo, hi, 0.0)
    assert np.isfinite(costs).all() and 0 < live.sum() < int((al * (ll + 1)).sum())
    cost, g = _run_dense(acts, labels, al, ll, F32, windows=(_dev(lo), _dev(hi)))
    err = np.abs(g.double().cpu().numpy() - grads)
    print("walks windows U1=513: cost max err %.3g, gradient max err %.3g"
          % (np.abs(cost.cpu().numpy() - costs).max(), err.max()))
    np.testing.assert_allclose(cost.cpu().numpy(), costs, rtol=1e-5, atol=1e-4)
    assert (err <= 1e-3 * np.abs(grads) + 2e-5).all(), err.max()
    assert (g.cpu()[torch.tensor(~live)] == 0).all()                 # dead cells and cells outside the boxes


# ------------------------------------------------------------------------------------ the one limit, from the far side
def _limit_calls(dtype):
    """(name, args) of every family's entry point on a batch of one utterance with U1 = 1025 labels columns; the output
    buffers - costs, reduced, gradient, frames, scores, workspace - hold sentinels and are returned as `outs`."""
    from edgedict_amd import _lib
    lib = _lib.load()
    Bn, Tn, U1, V = 1, 2, 1025, 8
    code = _lib.dtype_code(dtype)
    g = torch.Generator(device="cpu").manual_seed(1025)
    acts = torch.randn(Bn, Tn, U1, V, generator=g).to(dtype).cuda()
    acts_bf = acts.to(BF16)
    lab = torch.randint(1, V, (Bn, U1 - 1), generator=g, dtype=torch.int32).cuda()
    al, ll, off = _dev([Tn]), _dev([U1 - 1]), _dev([0], torch.int64)
    lo, hi = _dev(np.zeros((Bn, U1 - 1))), _dev(np.full((Bn, U1 - 1), Tn - 1))
    parts = torch.ones(Bn * Tn * U1, 1, 2, device="cuda")
    nbytes = lib.edgedict_rnnt_workspace_bytes(Bn, Tn, U1)
    # still defined behind the limit: room for three fp32 and two fp64 planes and the likelihoods, and no less than at 1024
    need = Bn * Tn * U1 * (3 * 4 + 2 * 8) + 2 * 8 * Bn
    assert need <= nbytes <= 2 * need and nbytes > lib.edgedict_rnnt_workspace_bytes(Bn, Tn, U1 - 1)
    outs = {
        "costs": torch.full((Bn,), 7.0, device="cuda"), "red": torch.full((1,), 7.0, device="cuda"),
        "grads": torch.full((Bn, Tn, U1, V), 7.0, dtype=dtype, device="cuda"),
        "frames": torch.full((Bn, U1 - 1), -7, dtype=torch.int32, device="cuda"),
        "scores": torch.full((Bn,), 7.0, device="cuda"),
        "ws": torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda"),
    }
    c, r, gr, fr, sc, ws = (outs[k] for k in ("costs", "red", "grads", "frames", "scores", "ws"))
    dims = (Bn, Tn, U1, V, 0)
    lens = (lab, al, ll)
    fwd = (c, r, 1.0, ws)
    bwd = (ws, 1.0, None, 0)
    calls = [
        ("rnnt_loss_forward", (acts, code) + lens + dims + fwd),
        ("rnnt_loss_forward_packed", (acts, code) + lens + (off,) + dims + fwd),
        ("rnnt_loss_forward_packed_parts", (acts_bf,) + lens + (off,) + dims + fwd + (parts, 1)),
        ("rnnt_loss_forward_ar", (acts, code) + lens + (lo, hi) + dims + fwd),
        ("rnnt_loss_forward_packed_ar", (acts, code) + lens + (lo, hi, off) + dims + fwd),
        ("rnnt_loss_forward_packed_parts_ar", (acts_bf,) + lens + (lo, hi, off) + dims + fwd + (parts, 1)),
        ("rnnt_align", (acts, code) + lens + dims + (fr, sc, ws)),
        ("rnnt_align_packed", (acts, code) + lens + (off,) + dims + (fr, sc, ws)),
        ("rnnt_align_packed_parts", (acts_bf,) + lens + (off,) + dims + (fr, sc, ws, parts, 1)),
        ("rnnt_align_ar", (acts, code) + lens + (lo, hi) + dims + (fr, sc, ws)),
        ("rnnt_align_packed_ar", (acts, code) + lens + (lo, hi, off) + dims + (fr, sc, ws)),
        ("rnnt_align_packed_parts_ar", (acts_bf,) + lens + (lo, hi, off) + dims + (fr, sc, ws, parts, 1)),
        ("rnnt_loss_backward", (acts, code, gr) + lens + dims + bwd),
        ("rnnt_loss_backward_packed", (acts, code, gr) + lens + (off,) + dims + bwd),
        ("rnnt_loss_backward_fe", (acts, code, gr) + lens + dims + bwd + (0.01,)),
        ("rnnt_loss_backward_packed_fe", (acts, code, gr) + lens + (off,) + dims + bwd + (0.01,)),
        ("rnnt_loss_backward_ar", (acts, code, gr) + lens + dims + bwd + (0.0,)),
        ("rnnt_loss_backward_packed_ar", (acts, code, gr) + lens + (off,) + dims + bwd + (0.0,)),
    ]
    return calls, outs, (acts, lab, al, ll)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_label_limit_is_1024_for_every_family(hip_lib, dtype):
    """U1 = 1024 is accepted by all of them (the cases above and tests/test_rnnt_align_gpu.py run there); U1 = 1025 is
    refused by each with the message that names 1024, before any launch: no output and no workspace byte changes."""
    from edgedict_amd import _lib
    from edgedict_amd.loss import RNNTLoss, rnnt_align
    calls, outs, (acts, lab, al, ll) = _limit_calls(dtype)
    before = {k: v.clone() for k, v in outs.items()}
    torch.cuda.synchronize()
    for name, args in calls:
        with pytest.raises(RuntimeError, match="maximum of 1024"):
            _lib.call(name, *args)
        torch.cuda.synchronize()
        for k, v in outs.items():
            assert torch.equal(v, before[k]), (name, k)
    with pytest.raises(RuntimeError, match="maximum of 1024"):
        RNNTLoss(reduction="none")(acts, lab, al, ll)
    with pytest.raises(RuntimeError, match="maximum of 1024"):
        rnnt_align(acts, lab, al, ll)
    torch.cuda.synchronize()
