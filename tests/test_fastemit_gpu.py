"""GPU: FastEmit in the RNN-T loss-gradient kernels (rnnt_grad / rnnt_grad_cs with FE = true) against the float64
restatement tests/fastemit_ref.py (pinned by tests/test_fastemit_host.py), through every route the gradient takes: the
dense operator, the packed lattice (fp32, bf16, bf16 with the logits product's log-sum-exp partials), utterance ranges,
the fused column sums, Transducer.forward on both of its loss paths and TrainEngine.

Bounds are those the existing tests hold the plain gradient to (tests/test_rnnt_loss_gpu.py,
tests/test_packed_lattice_gpu.py), times 1 + lambda: the gradient grows by at most that factor.  lambda = 0 through the
new entry points must be the old entry points bit for bit, and the costs never depend on lambda."""
import types

import numpy as np
import pytest
import torch

import fastemit_ref as FR
from oracle import packed_ref as PR

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
LAMBDAS = [0.01, 0.5]


def _case(seed, B, T, U1, V, ragged=True):
    """tests/test_rnnt_loss_gpu.py::_case"""
    rng = np.random.default_rng(seed)
    acts = rng.normal(size=(B, T, U1, V)).astype(np.float32)
    labels = rng.integers(1, V, size=(B, max(U1 - 1, 0))).astype(np.int32)
    if ragged:
        al = rng.integers(1, T + 1, size=B).astype(np.int32)
        ll = rng.integers(0, U1, size=B).astype(np.int32)
    else:
        al = np.full(B, T, np.int32)
        ll = np.full(B, U1 - 1, np.int32)
    al[0] = T
    ll[0] = U1 - 1
    return acts, labels, al, ll


def _run_hip(acts, labels, al, ll, dtype, lam, reduction="none"):
    from edgedict_amd.loss import RNNTLoss
    ta = torch.tensor(acts, device="cuda").to(dtype).requires_grad_(True)
    loss = RNNTLoss(blank=0, reduction=reduction, fastemit_lambda=lam)(
        ta, torch.tensor(labels, device="cuda"), torch.tensor(al, device="cuda"), torch.tensor(ll, device="cuda"))
    (loss.sum() if reduction == "none" else loss).backward()
    return loss.detach().clone(), ta.grad


# test_rnnt_loss_gpu.py::test_fp32_matches_oracle's shapes, plus T = 1 with labels and a batch with a U_b = 0 utterance
# beside longer ones (forced below)
DENSE_SHAPES = [
    (1, 1, 1, 7, False), (2, 5, 1, 16, True), (3, 7, 5, 11, True), (4, 33, 9, 64, True), (2, 40, 70, 128, True),
    (4, 84, 21, 2048, True),
    (3, 1, 5, 16, True),       # T = 1: every label on the only frame
    (4, 9, 6, 24, "u0"),       # utterance 1 has no labels
]


@pytest.mark.parametrize("B,T,U1,V,ragged", DENSE_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_dense_gradient_matches_oracle(hip_lib, B, T, U1, V, ragged, dtype):
    acts, labels, al, ll = _case(B * 1000 + T, B, T, U1, V, bool(ragged))
    if ragged == "u0":
        ll[1] = 0
    seen = torch.tensor(acts).to(dtype).double().numpy()             # bf16: the oracle sees the rounded logits
    cost0, g0 = _run_hip(acts, labels, al, ll, dtype, 0.0)
    for lam in LAMBDAS:
        costs, grads = FR.fastemit_loss(seen, labels, al, ll, lam)
        cost, g = _run_hip(acts, labels, al, ll, dtype, lam)
        assert torch.equal(cost, cost0), lam                         # the costs stay the plain ones, bit for bit
        err = np.abs(g.double().cpu().numpy() - grads)
        print("fastemit dense", (B, T, U1, V), dtype, lam, "max err %.3g" % err.max())
        if dtype == F32:
            np.testing.assert_allclose(cost.cpu().numpy(), costs, rtol=1e-5, atol=1e-4)
            assert (err <= (1 + lam) * (1e-3 * np.abs(grads) + 2e-5)).all(), (lam, err.max())
        else:
            np.testing.assert_allclose(cost.cpu().numpy(), costs, rtol=1e-4)
            assert (err <= (1 + lam) * 4e-3).all(), (lam, err.max())
        assert not torch.equal(g, g0) or U1 == 1                     # (no labels: FastEmit has nothing to scale)
        if U1 == 1:
            assert torch.equal(g, g0)
        # 'mean': shape (1,), gradient x 1 / B
        cm, gm = _run_hip(acts, labels, al, ll, dtype, lam, reduction="mean")
        assert cm.shape == (1,)
        errm = np.abs(gm.double().cpu().numpy() - grads / B)
        tol = (1e-3 * np.abs(grads / B) + 2e-5) if dtype == F32 else 4e-3
        assert (errm <= (1 + lam) * tol).all()


# --------------------------------------------------------------------------------------------------- packed routes
P_B, P_T, P_U1, P_J = 5, 23, 7, 128
P_AL, P_LL = [23, 20, 9, 23, 4], [6, 2, 6, 0, 5]       # test_backward_in_utterance_ranges_equals_one_pass's boxes


class _Packed:
    """One set of logits (those the logits product wrote, with its log-sum-exp partials) and the three forward routes'
    filled workspaces."""

    def __init__(self, lib, V, seed):
        from edgedict_amd import _lib
        from edgedict_amd.ops import _ll
        self.lib, self.V = lib, V
        B, T, U1, J = P_B, P_T, P_U1, P_J
        g = torch.Generator(device="cpu").manual_seed(seed)
        off, self.M = PR.offsets(P_AL, P_LL)
        self.al_d = torch.tensor(P_AL, dtype=torch.int32).cuda()
        self.ll_d = torch.tensor(P_LL, dtype=torch.int32).cuda()
        self.off, self.off_d = off, off.cuda()
        hid = torch.tanh(torch.randn(self.M, J, generator=g)).to(BF16).cuda()
        w2 = (torch.randn(V, J, generator=g) / 4).to(BF16).cuda()
        b2 = torch.randn(V, generator=g).cuda()
        self.labels = torch.randint(1, V, (B, U1 - 1), generator=g, dtype=torch.int32).cuda()
        slots = (V + 63) // 64
        parts = torch.full((self.M, slots, 2), float("nan"), device="cuda")
        self.logits = {BF16: torch.full((self.M, V), float("nan"), dtype=BF16, device="cuda")}
        _lib.call("gemm_nt_lse", hid, _ll(J), w2, _ll(J), self.logits[BF16], _ll(V), self.M, V, J, b2, parts)
        torch.cuda.synchronize()
        self.logits[F32] = self.logits[BF16].float()
        nbytes = lib.edgedict_rnnt_workspace_bytes(B, T, U1)
        self.ws, self.costs = {}, {}
        for route in ("f32", "bf16", "parts"):
            w = self.ws[route] = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
            c = self.costs[route] = torch.empty(B, device="cuda")
            red = torch.empty(1, device="cuda")
            if route == "parts":
                _lib.call("rnnt_loss_forward_packed_parts", self.logits[BF16], self.labels, self.al_d, self.ll_d,
                          self.off_d, B, T, U1, V, 0, c, red, 1.0 / B, w, parts, slots)
            else:
                dt = F32 if route == "f32" else BF16
                _lib.call("rnnt_loss_forward_packed", self.logits[dt], _lib.dtype_code(dt), self.labels, self.al_d,
                          self.ll_d, self.off_d, B, T, U1, V, 0, c, red, 1.0 / B, w)
        torch.cuda.synchronize()

    def dtype(self, route):
        return F32 if route == "f32" else BF16

    def backward(self, route, name, *tail, fill=float("nan")):
        """edgedict_rnnt_loss_<name> on the route's logits and workspace; `tail` = the arguments behind grad_scale_stride."""
        from edgedict_amd import _lib
        dt = self.dtype(route)
        out = torch.full((self.M, self.V), fill, dtype=dt, device="cuda")
        _lib.call("rnnt_loss_" + name, self.logits[dt], _lib.dtype_code(dt), out, self.labels, self.al_d, self.ll_d,
                  self.off_d, P_B, P_T, P_U1, self.V, 0, self.ws[route], 1.0 / P_B, None, 0, *tail)
        torch.cuda.synchronize()
        return out

    def oracle(self, lam):
        dense = PR.unpack(self.logits[F32].cpu().double(), P_AL, P_LL, T=P_T, U1=P_U1, fill=0.0)
        costs, grads = FR.fastemit_loss(dense.numpy(), self.labels.cpu().numpy(), P_AL, P_LL, lam)
        return costs, PR.pack(torch.tensor(grads), P_AL, P_LL) / P_B


@pytest.mark.parametrize("V", [264, 1024])            # both inside the fused column sums' limits (fp32: V <= 1024)
def test_packed_routes_match_oracle_and_each_other(hip_lib, V):
    from edgedict_amd import _lib
    lib = hip_lib
    pk = _Packed(lib, V, seed=V)
    B, T, U1 = P_B, P_T, P_U1
    for lam in LAMBDAS:
        _, want = pk.oracle(lam)
        want = want.cuda()
        for route in ("f32", "bf16", "parts"):
            dt = pk.dtype(route)
            code = _lib.dtype_code(dt)
            got = pk.backward(route, "backward_packed_fe", lam)
            # test_packed_loss_forward_and_backward's bounds (total row scale 1 / B), times 1 + lambda
            tol = (1e-3 * want.abs() + 2e-5 / B) if dt == F32 else torch.full_like(want, 4e-3 / B)
            err = (got.double() - want).abs()
            print("fastemit packed", V, route, lam, "max err %.3g" % err.max().item())
            assert (err <= (1 + lam) * tol).all(), (route, lam, err.max().item())
            # utterance ranges write exactly the one-pass gradient, other utterances' rows untouched
            parts = torch.full_like(got, 7.0)
            for b0, nb in ((0, 2), (2, 0), (2, 3)):
                _lib.call("rnnt_loss_backward_packed_range_fe", pk.logits[dt], code, parts, pk.labels, pk.al_d, pk.ll_d,
                          pk.off_d, B, T, U1, V, 0, pk.ws[route], 1.0 / B, None, 0, b0, nb, lam)
                if (b0, nb) == (0, 2):
                    torch.cuda.synchronize()
                    assert (parts[int(pk.off[2]):] == 7.0).all()
            torch.cuda.synchronize()
            assert torch.equal(parts, got), (route, lam)
            # fused column sums: the same matrix bit for bit, partial rows that add up to its column sums
            n = lib.edgedict_rnnt_grad_colsum_rows(code, B, T, U1, V)
            assert n > 0
            cs = torch.full((n, V), float("nan"), device="cuda")
            fused = pk.backward(route, "backward_packed_colsum_fe", cs, lam)
            assert torch.equal(fused, got), (route, lam)
            ctol = 1e-5 if dt == F32 else 2.0 ** -8
            assert ((cs.double().sum(0) - got.double().sum(0)).abs() <= ctol * got.double().abs().sum(0) + 1e-12).all()
            assert ((cs.double().sum(0) - want.sum(0)).abs() <= ctol * (1 + lam) * want.abs().sum(0) + 1e-12).all()
            if route == "parts":
                continue
            # packed == dense inside the boxes (same arithmetic per cell), exact zeros outside
            dense_logits = PR.unpack(pk.logits[dt].cpu(), P_AL, P_LL, T=T, U1=U1, fill=0.0).cuda().contiguous()
            ws = torch.zeros_like(pk.ws[route])
            costs, red = torch.empty(B, device="cuda"), torch.empty(1, device="cuda")
            _lib.call("rnnt_loss_forward", dense_logits, code, pk.labels, pk.al_d, pk.ll_d, B, T, U1, V, 0, costs, red,
                      1.0 / B, ws)
            dg = torch.full_like(dense_logits, float("nan"))
            _lib.call("rnnt_loss_backward_fe", dense_logits, code, dg, pk.labels, pk.al_d, pk.ll_d, B, T, U1, V, 0, ws,
                      1.0 / B, None, 0, lam)
            torch.cuda.synchronize()
            assert torch.equal(costs, pk.costs[route])
            assert torch.equal(PR.pack(dg.cpu(), P_AL, P_LL), got.cpu()), (route, lam)
            assert torch.equal(PR.unpack(got.cpu(), P_AL, P_LL, T=T, U1=U1, fill=0.0), dg.cpu())


@pytest.mark.parametrize("V", [264, 1024])
def test_lambda_zero_is_the_old_entry_point_bit_for_bit(hip_lib, V):
    from edgedict_amd import _lib
    lib = hip_lib
    pk = _Packed(lib, V, seed=3 + V)
    B, T, U1 = P_B, P_T, P_U1
    for route in ("f32", "bf16", "parts"):
        dt = pk.dtype(route)
        code = _lib.dtype_code(dt)
        old = pk.backward(route, "backward_packed")
        assert torch.isfinite(old.float()).all()
        assert torch.equal(pk.backward(route, "backward_packed_fe", 0.0), old)
        assert torch.equal(pk.backward(route, "backward_packed_range_fe", 0, B, 0.0), old)
        assert torch.equal(pk.backward(route, "backward_packed_range", 0, B), old)
        n = lib.edgedict_rnnt_grad_colsum_rows(code, B, T, U1, V)
        cs_old = torch.full((n, V), float("nan"), device="cuda")
        cs_new = torch.full((n, V), float("nan"), device="cuda")
        assert torch.equal(pk.backward(route, "backward_packed_colsum", cs_old), old)
        assert torch.equal(pk.backward(route, "backward_packed_colsum_fe", cs_new, 0.0), old)
        assert torch.isfinite(cs_old).all() and torch.equal(cs_old, cs_new)
        assert not torch.equal(pk.backward(route, "backward_packed_fe", 0.01), old)
    # dense operator: RNNTLoss(fastemit_lambda=0) against the native old entry point on the same logits
    acts, labels, al, ll = _case(77, 3, 12, 5, 64)
    for dt in (F32, BF16):
        cost, g = _run_hip(acts, labels, al, ll, dt, 0.0)
        ta = torch.tensor(acts, device="cuda").to(dt)
        ws = torch.zeros(lib.edgedict_rnnt_workspace_bytes(3, 12, 5), dtype=torch.uint8, device="cuda")
        costs, red = torch.empty(3, device="cuda"), torch.empty(1, device="cuda")
        args = (torch.tensor(labels).cuda(), torch.tensor(al).cuda(), torch.tensor(ll).cuda(), 3, 12, 5, 64, 0)
        _lib.call("rnnt_loss_forward", ta, _lib.dtype_code(dt), *args, costs, red, 1.0, ws)
        old, new = torch.empty_like(ta), torch.empty_like(ta)
        ones = torch.ones(3, device="cuda")
        _lib.call("rnnt_loss_backward", ta, _lib.dtype_code(dt), old, *args, ws, 1.0, ones, 1)
        _lib.call("rnnt_loss_backward_fe", ta, _lib.dtype_code(dt), new, *args, ws, 1.0, ones, 1, 0.0)
        torch.cuda.synchronize()
        assert torch.equal(old, new) and torch.equal(old, g) and torch.equal(costs, cost)


# --------------------------------------------------------------------------------------------------- full-size slice
def test_full_size_lattice_rows_sum_to_zero_and_gradient_is_linear_in_lambda(hip_lib):
    """E6D2 / B = 8 slice (T' = 201, U + 1 = 65, V = 2048; test_full_size_lattice_properties), too big for the Python
    oracle: size-independent properties.  Linearity: grad(lambda) = grad(0) + lambda (softmax_k - [k == y]) wl exactly, so
    g(0.5) - g(0) = 50 (g(0.01) - g(0)).  The kernel's relative error per element is a few 1e-7 (fp32 exp of an argument
    of magnitude <~ 20), 50 x that stays inside rtol 1e-3 where the element is the label's, and inside atol 2e-5 on the
    softmax part (softmax_k <= ~1e-2 at V = 2048 standard-normal logits)."""
    from edgedict_amd.loss import RNNTLoss
    B, T, U1, V = 8, 201, 65, 2048
    g = torch.Generator(device="cpu").manual_seed(0)
    acts = torch.randn(B, T, U1, V, generator=g).cuda()
    labels = torch.randint(4, V, (B, U1 - 1), generator=g, dtype=torch.int32).cuda()
    al = torch.randint(150, T + 1, (B,), generator=g, dtype=torch.int32)
    ll = torch.randint(32, U1, (B,), generator=g, dtype=torch.int32)
    al[0], ll[0] = T, U1 - 1
    al, ll = al.cuda(), ll.cuda()
    grads, costs = {}, {}
    for lam in (0.0, 0.01, 0.5):
        a = acts.clone().requires_grad_(True)
        loss = RNNTLoss(reduction="none", fastemit_lambda=lam)(a, labels, al, ll)
        loss.sum().backward()
        grads[lam], costs[lam] = a.grad, loss.detach().clone()
        rows = a.grad.sum(-1).abs().max().item()
        print("fastemit full size: lambda %g, max |row sum| %.3g" % (lam, rows))
        assert rows < 1e-4 * (1 + lam)
        assert torch.equal(costs[lam], costs[0.0])
        for b in range(B):
            assert a.grad[b, int(al[b]):].abs().max().item() == 0 if int(al[b]) < T else True
            assert a.grad[b, :, int(ll[b]) + 1:].abs().max().item() == 0 if int(ll[b]) + 1 < U1 else True
    big = grads[0.5] - grads[0.0]
    small = 50.0 * (grads[0.01] - grads[0.0])
    err = (big - small).abs()
    print("fastemit full size: linearity max err %.3g, max |g(0.5) - g(0)| %.3g" % (err.max().item(), big.abs().max().item()))
    assert big.abs().max().item() > 1e-2
    assert (err <= 1e-3 * big.abs() + 2e-5).all(), err.max().item()


# --------------------------------------------------------------------------------------------------- model level
def _tiny():
    from oracle import models_ref as M
    from oracle.make_golden import CASES
    cfg, B, T0, U, seed = CASES["tiny"]
    return cfg, M.make_state_dict(cfg, seed), M.make_batch(cfg, seed + 1, B, T0, U)


def _engine(cfg, sd, output_loss, lam):
    from edgedict_amd.models import Transducer
    m = Transducer(enc_dropout=0.0, dec_dropout=0.0, output_loss=output_loss, fastemit_lambda=lam, **cfg)
    m.load_state_dict(sd, strict=True)
    m = m.cuda()
    m.compute_dtype = "fp32"
    return m


def test_model_packed_and_dense_paths_agree_and_bias_gradient_is_the_oracles_column_sum(hip_lib):
    from edgedict_amd import config
    cfg, sd, (xs, ys, xlen, ylen) = _tiny()
    lam = 0.5
    packed = _engine(cfg, sd, True, lam)
    lp = packed(xs.cuda(), ys.cuda(), xlen, ylen)            # host lengths: _JointLossFn
    lp.backward()
    dense = _engine(cfg, sd, True, lam)
    saved = config.PACKED_LATTICE
    config.PACKED_LATTICE = False
    try:
        ld = dense(xs.cuda(), ys.cuda(), xlen, ylen)         # same call, dense logits + _RNNTLossFn
        ld.backward()
    finally:
        config.PACKED_LATTICE = saved
    plain = _engine(cfg, sd, True, 0.0)
    l0 = plain(xs.cuda(), ys.cuda(), xlen, ylen)
    l0.backward()
    assert lp.item() == ld.item() == l0.item()               # the loss does not see lambda
    # test_packed_lattice_path_matches_golden_loss_and_dense_gradients' bound
    for (n, a), (_, b) in zip(packed.named_parameters(), dense.named_parameters()):
        scale = max(b.grad.abs().max().item(), 1e-8)
        assert (a.grad - b.grad).abs().max().item() <= 2e-5 * scale, n
    moved = [n for (n, a), (_, b) in zip(packed.named_parameters(), plain.named_parameters()) if not torch.equal(a.grad, b.grad)]
    assert len(moved) > len(list(plain.parameters())) // 2
    assert not torch.equal(packed.joint.joint[2].bias.grad, plain.joint.joint[2].bias.grad)
    # the joint's output-bias gradient = column sum of the FastEmit gradient of the model's own logits (float64 oracle)
    logit_model = _engine(cfg, sd, False, 0.0)
    with torch.no_grad():
        logits = logit_model(xs.cuda(), ys.cuda(), xlen.cuda(), ylen.cuda())
        act = logit_model.scale_length(logits, xlen)
    B = xs.shape[0]
    U = int(ylen.max())
    _, grads = FR.fastemit_loss(logits.double().cpu().numpy(), ys[:, :U].numpy(), act.numpy(), ylen.numpy(), lam)
    ref = torch.tensor(grads.reshape(-1, grads.shape[-1]).sum(0) / B)
    for m in (packed, dense):
        got = m.joint.joint[2].bias.grad.double().cpu()
        err = (got - ref).abs().max().item()
        print("fastemit db2 err %.3g of max %.3g" % (err, ref.abs().max().item()))
        assert err <= 2e-5 * ref.abs().max().item()          # test_joint_loss_fn_fp32's bound


def _flags(lam=None):
    fl = types.SimpleNamespace(
        downsample=3, win_length=320, hop_length=160, n_fft=512, feature_size=80, dither=0.0,
        sample_rate=16000, lr=2e-3, gradclip=None, sub_batch_size=None, bpe_size=40,
        vocab_embed_size=8, enc_hidden_size=32, enc_layers=3, enc_dropout=0.0, enc_proj_size=24,
        dec_hidden_size=16, dec_layers=2, dec_dropout=0.0, dec_proj_size=16, joint_size=32,
        enc_time_reductions=[1], delta=False, T_mask=0, T_num_mask=0, F_mask=0, F_num_mask=0)
    if lam is not None:
        fl.fastemit_lambda = lam
    return fl


def test_train_engine_reads_the_flag(hip_lib):
    """TrainEngine built from flags carrying fastemit_lambda: the gradients of step 0 change, its reported loss does not."""
    from edgedict_amd.trainer import TrainEngine
    g = torch.Generator(device="cpu").manual_seed(5)
    wave = (0.1 * torch.randn(4, 9600, generator=g)).cuda()
    ys = torch.randint(4, 40, (4, 6), generator=g, dtype=torch.int32).cuda()
    ylen = torch.tensor([6, 4, 5, 6], dtype=torch.int32)
    out = {}
    for lam in (None, 0.0, 0.5):
        torch.manual_seed(0)
        eng = TrainEngine(_flags(lam), vocab_size=40, device="cuda", compute_dtype="fp32")
        try:
            assert eng.model.fastemit_lambda == (lam or 0.0)
            loss = eng.train_step(wave, None, ys, ylen)
            torch.cuda.synchronize()
            out[lam] = (loss.detach().clone(), {n: p.grad.detach().clone() for n, p in eng.model.named_parameters()})
        finally:
            eng.close()
    with pytest.raises(ValueError, match="fastemit_lambda"):
        TrainEngine(_flags(-1.0), vocab_size=40, device="cuda", compute_dtype="fp32")
    assert torch.equal(out[None][0], out[0.0][0]) and torch.equal(out[None][0], out[0.5][0])
    # Two engines on the same code path (no flag / lambda = 0) agree up to the order of the fp32 sums only (weight
    # gradients are accumulated with atomics and split-K on an auxiliary stream): 2e-5 of the tensor's largest entry,
    # test_packed_lattice_path_matches_golden_loss_and_dense_gradients' bound for that.  FastEmit moves a gradient by
    # O(lambda wl) of itself: "changed" means by more than 1e-3 of the largest entry, 50 x that noise bound.
    def rel(a, b):
        return (a - b).abs().max().item() / max(a.abs().max().item(), 1e-8)

    names = list(out[None][1])
    noise = {n: rel(out[None][1][n], out[0.0][1][n]) for n in names}
    moved = {n: rel(out[None][1][n], out[0.5][1][n]) for n in names}
    print("fastemit engine: max run-to-run %.3g, median FastEmit shift %.3g" % (max(noise.values()), sorted(moved.values())[len(names) // 2]))
    assert all(v <= 2e-5 for v in noise.values()), noise
    changed = [n for n in names if moved[n] > 1e-3]
    assert len(changed) > len(names) // 2, moved
