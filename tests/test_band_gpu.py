"""GPU: joint + loss packed onto the emission-window band (loss.rnnt_band_plan, the *_band entry points,
models._JointLossFn with a plan, Transducer.forward under config.BAND_LATTICE).

The yardstick is the box path under the same windows (the *_packed_ar entry points, tests/test_arloss_gpu.py): given the
same logits the band route must reproduce its costs, the alpha / beta / denominator planes on the live cells and its
gradient rows BIT FOR BIT; what is summed in another order (joint_hidden_bwd_band, the weight gradients) is held to the
bounds the box path's own tests use.  Layout and shapes: tests/band_ref.py, tests/test_band_host.py."""
import ctypes

import numpy as np
import pytest
import torch

import arloss_ref as AR
import band_ref as BR
import test_arloss_gpu as TA
import test_band_host as TH
import test_fastemit_gpu as TF
import test_packed_lattice_gpu as TP
from oracle import packed_ref as PR

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
P_B, P_T, P_U1, P_AL, P_LL = TH.P_B, TH.P_T, TH.P_U1, TH.P_AL, TH.P_LL
W_B, W_T, W_U1, W_AL, W_LL = TH.W_B, TH.W_T, TH.W_U1, TH.W_AL, TH.W_LL
GUARD, SENT = 8, 768.0
LAMBDAS = [0.0, 0.5]
_dev = TA._dev


def _plan(lo, hi, al, ll, T):
    from edgedict_amd import loss as L
    return L.rnnt_band_plan(_dev(lo), _dev(hi), _dev(al), _dev(ll), T)


def _guarded(m, n, dtype):
    buf = torch.full((m + GUARD, n), float("nan"), dtype=dtype, device="cuda")
    buf[m:] = SENT
    return buf


def _to_band(packed, al, ll, T, U1, band):
    """rows of the box-packed matrix [M, ...] gathered onto the band [M_band, ...]"""
    return BR.band_pack(PR.unpack(packed.cpu(), al, ll, T=T, U1=U1, fill=0.0), band).cuda().contiguous()


# ------------------------------------------------------------------------------------------------------------ 1. plan
@pytest.mark.parametrize("case", list(TH.all_cases()), ids=lambda c: c[0])
def test_plan_is_the_restatements(hip_lib, case):
    name, al, ll, T, U1, (lo, hi) = case
    plan = _plan(lo, hi, al, ll, T)
    band, cells = AR.band_table(lo, hi, al, ll, T)
    row_off, rows = BR.band_offsets(band)
    assert type(plan.rows) is int and plan.rows == rows == int(cells.sum())
    assert plan.band.dtype == torch.int32 and plan.band.cpu().numpy().tolist() == band.tolist()
    assert plan.cells.dtype == torch.int64 and plan.cells.cpu().numpy().tolist() == cells.tolist()
    assert plan.row_off.dtype == torch.int64 and plan.row_off.cpu().numpy().tolist() == row_off.tolist()
    assert plan.row_tu.dtype == torch.int32 and plan.row_tu.shape == (rows,)
    assert plan.row_tu.cpu().numpy().tolist() == BR.band_row_tu(band).tolist()


# --------------------------------------------------------------------------------------------- 2. joint_hidden_fwd_band
FWD_CASES = {"P-align21": (P_AL, P_LL, P_T, P_U1, lambda: TH.p_windows("align21", 264)),
             "P-infeasible": (P_AL, P_LL, P_T, P_U1, lambda: TH.p_windows("infeasible", 264)),
             "W-21": (W_AL, W_LL, W_T, W_U1, lambda: TH.w_windows(2, 1))}


@pytest.mark.parametrize("name", list(FWD_CASES))
@pytest.mark.parametrize("J", [128, 40])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_joint_hidden_fwd_band_is_the_packed_kernels_rows(hip_lib, name, J, dtype):
    from edgedict_amd import _lib
    from edgedict_amd.ops import _ll
    al, ll, T, U1, windows = FWD_CASES[name]
    lo, hi = windows()
    B = len(al)
    plan = _plan(lo, hi, al, ll, T)
    band = plan.band.cpu().numpy()
    g = torch.Generator(device="cpu").manual_seed(J + T)
    E1 = torch.randn(B, T, J, generator=g).to(dtype).cuda()
    D1 = torch.randn(B, U1, J, generator=g).to(dtype).cuda()
    box, m = TP._run_fwd_packed(E1, D1, al, ll)
    want = _to_band(box[:m], al, ll, T, U1, band)
    buf = _guarded(plan.rows, J, dtype)
    _lib.call("joint_hidden_fwd_band", _lib.dtype_code(dtype), E1, D1, buf, plan.band, plan.row_off, _ll(plan.rows),
              B, T, U1, J)
    torch.cuda.synchronize()
    assert 0 < plan.rows < m
    assert torch.equal(buf[:plan.rows], want)
    assert (buf[plan.rows:] == SENT).all()


# ------------------------------------------------------------------------------------------- 3 / 4. the loss on band rows
def _planes(lib, ws, B, T, U1):
    """(denom f32, alpha f64, beta f64) [B, T, U1] views of a workspace"""
    base = ws.data_ptr()
    out = []
    for which, dtype, esz in ((0, torch.float32, 4), (1, torch.float64, 8), (2, torch.float64, 8)):
        p = lib.edgedict_rnnt_workspace_view(ctypes.c_void_p(base), B, T, U1, which)
        off = (p - base) // esz
        out.append(ws.view(dtype)[off:off + B * T * U1].view(B, T, U1))
    return out


class _BandCase:
    """test_arloss_gpu._PackedAr under one set of windows, its logits and log-sum-exp pairs gathered onto the band, and
    the band forward's workspaces and costs for the three routes."""

    def __init__(self, lib, V, kind):
        from edgedict_amd import _lib
        B, T, U1 = P_B, P_T, P_U1
        self.V, self.kind = V, kind
        lo, hi = TA._packed_windows(kind, V)
        pk = self.pk = TA._PackedAr(lib, V, seed=V).restrict(lo, hi)
        plan = self.plan = _plan(lo, hi, P_AL, P_LL, T)
        self.band = plan.band.cpu().numpy()
        self.live = torch.tensor(AR.live_from_band(self.band, U1)).cuda()
        self.tables = (plan.band, plan.row_off, plan.row_tu, plan.cells)
        self.logits = {dt: _to_band(pk.logits[dt], P_AL, P_LL, T, U1, self.band) for dt in (F32, BF16)}
        self.parts = _to_band(pk.parts, P_AL, P_LL, T, U1, self.band)
        slots = (V + 63) // 64
        self.ws, self.costs = {}, {}
        for route in ("f32", "bf16", "parts"):
            w = self.ws[route] = torch.zeros_like(pk.ws[route])
            c = self.costs[route] = torch.full((B,), float("nan"), device="cuda")
            red = torch.empty(1, device="cuda")
            if route == "parts":
                _lib.call("rnnt_loss_forward_band_parts", self.logits[BF16], pk.labels, pk.al_d, pk.ll_d, pk.lo_d, pk.hi_d,
                          *self.tables, B, T, U1, V, 0, c, red, 1.0 / B, w, self.parts, slots)
            else:
                dt = pk.dtype(route)
                _lib.call("rnnt_loss_forward_band", self.logits[dt], _lib.dtype_code(dt), pk.labels, pk.al_d, pk.ll_d,
                          pk.lo_d, pk.hi_d, *self.tables, B, T, U1, V, 0, c, red, 1.0 / B, w)
        torch.cuda.synchronize()

    def backward(self, route, lam, colsum=None):
        from edgedict_amd import _lib
        pk, dt = self.pk, self.pk.dtype(route)
        out = _guarded(self.plan.rows, self.V, dt)
        head = (self.logits[dt], _lib.dtype_code(dt), out, pk.labels, pk.al_d, pk.ll_d) + self.tables[1:] + (
            P_B, P_T, P_U1, self.V, 0, self.ws[route], 1.0 / P_B, None, 0)
        if colsum is None:
            _lib.call("rnnt_loss_backward_band", *head, lam)
        else:
            _lib.call("rnnt_loss_backward_band_colsum", *head, colsum, lam)
        torch.cuda.synchronize()
        return out


_CASES = {}


def _band_case(lib, V, kind):
    if (V, kind) not in _CASES:
        _CASES[(V, kind)] = _BandCase(lib, V, kind)
    return _CASES[(V, kind)]


@pytest.mark.parametrize("kind", ["align", "infeasible"])
@pytest.mark.parametrize("V", [264, 1024])
def test_loss_forward_on_band_rows_is_the_box_paths(hip_lib, V, kind):
    bc = _band_case(hip_lib, V, kind)
    pk = bc.pk
    B, T, U1 = P_B, P_T, P_U1
    assert 0 < bc.plan.rows < pk.M
    inside = torch.tensor(PR.unpack(torch.ones(pk.M), P_AL, P_LL, T=T, U1=U1, fill=0.0).numpy() > 0).cuda()
    oracle, _, _ = pk.oracle_ar(0.0)
    for route in ("f32", "bf16", "parts"):
        dt = pk.dtype(route)
        print("band costs", V, kind, route, bc.costs[route].tolist())
        assert not torch.isnan(bc.costs[route]).any()
        assert torch.equal(bc.costs[route], pk.costs[route]), route
        den, alpha, beta = _planes(hip_lib, bc.ws[route], B, T, U1)
        den0, alpha0, beta0 = _planes(hip_lib, pk.ws[route], B, T, U1)
        live = bc.live
        assert torch.equal(alpha[live], alpha0[live]) and torch.equal(beta[live], beta0[live]), route
        assert torch.equal(den[live], den0[live]), route
        assert torch.isfinite(alpha[live]).all() and torch.isfinite(beta[live]).all()
        dead = inside & ~live
        ninf = float("-inf")
        assert ((alpha[dead] == ninf) | (beta[dead] == ninf)).all(), route
        assert not torch.isnan(alpha[inside]).any() and not torch.isnan(beta[inside]).any()
        np.testing.assert_allclose(bc.costs[route].cpu().numpy(), oracle, rtol=1e-5 if dt == F32 else 1e-4,
                                   atol=1e-4 if dt == F32 else 0.0)
        assert (kind == "infeasible") == (bc.costs[route][2].item() == float("inf"))
        assert torch.isfinite(bc.costs[route][[0, 1, 3, 4]]).all()


@pytest.mark.parametrize("V", [264, 1024])
def test_covering_windows_on_band_rows_are_the_plain_packed_costs(hip_lib, V):
    bc = _band_case(hip_lib, V, "cover")
    assert bc.plan.rows == bc.pk.M                                   # the band is the box
    for route in ("f32", "bf16", "parts"):
        assert torch.equal(bc.costs[route], bc.pk.costs_plain[route]), route


@pytest.mark.parametrize("kind", ["align", "infeasible"])
@pytest.mark.parametrize("V", [264, 1024])
def test_loss_backward_on_band_rows_is_the_box_paths(hip_lib, V, kind):
    from edgedict_amd import _lib
    bc = _band_case(hip_lib, V, kind)
    pk = bc.pk
    B, T, U1 = P_B, P_T, P_U1
    M = bc.plan.rows
    for lam in LAMBDAS:
        _, oracle, _ = pk.oracle_ar(lam)
        oracle = _to_band(oracle, P_AL, P_LL, T, U1, bc.band).cpu().numpy()
        for route in ("f32", "bf16", "parts"):
            dt = pk.dtype(route)
            box = pk.backward(route, "backward_packed_ar", lam)
            want = _to_band(box, P_AL, P_LL, T, U1, bc.band)
            buf = bc.backward(route, lam)
            assert (buf[M:] == SENT).all(), (route, lam)
            got = buf[:M]
            assert torch.isfinite(got.float()).all()
            assert torch.equal(got, want), (route, lam, (got.float() - want.float()).abs().max().item())
            # fused column sums: the same matrix bit for bit, every partial row written, rows that add up
            n = hip_lib.edgedict_rnnt_grad_colsum_rows(_lib.dtype_code(dt), B, T, U1, V)
            assert n > 0
            cs = torch.full((n, V), float("nan"), device="cuda")
            fused = bc.backward(route, lam, colsum=cs)
            assert (fused[M:] == SENT).all() and torch.equal(fused[:M], got), (route, lam)
            assert torch.isfinite(cs).all()
            ctol = 1e-5 if dt == F32 else 2.0 ** -8
            assert ((cs.double().sum(0) - got.double().sum(0)).abs() <= ctol * got.double().abs().sum(0) + 1e-12).all()
            # the float64 oracle, test_arloss_gpu._check's bounds (row scale 1 / B)
            TA._check(None, got, None, oracle, dt, lam, "band %d %s %s" % (V, kind, route), scale=1.0 / B)


# --------------------------------------------------------------------------------------------- 5. joint_hidden_bwd_band
S_AL, S_LL, S_T, S_U1 = [8, 5, 8], [149, 90, 30], 8, 150      # few frames, many labels: ONE slab of 8 frames spans > 72 columns


def _s_windows():
    frames = AR.random_alignment(np.random.default_rng(2), S_AL, S_LL, S_U1 - 1)
    lo, hi = AR.windows_from_frames(frames, S_AL, S_LL, 2, 1, Tm=S_T)
    return lo.astype(np.int32), hi.astype(np.int32)


def _slab_spans(band, B, T, J):
    """live-column span of every (utterance, slab of frames) of joint_hidden_bwd_band, by the host code's slab formula"""
    jblocks = (J + 63) // 64
    tslabs = max(1, min((1280 + B * jblocks - 1) // (B * jblocks), (T + 7) // 8))
    tpb = (T + tslabs - 1) // tslabs
    spans = []
    for b in range(B):
        for t0 in range(0, T, tpb):
            rows = [r for r in band[b, t0:t0 + tpb] if r[1] >= r[0]]
            spans.append(max(r[1] for r in rows) - min(r[0] for r in rows) + 1 if rows else 0)
    return spans


BWD_CASES = {"W-21": (W_AL, W_LL, W_T, W_U1, lambda: TH.w_windows(2, 1)),
             "S-span150": (S_AL, S_LL, S_T, S_U1, _s_windows),
             "P-infeasible": (P_AL, P_LL, P_T, P_U1, lambda: TH.p_windows("infeasible", 264))}


@pytest.mark.parametrize("name", list(BWD_CASES))
@pytest.mark.parametrize("J", [128, 40])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_joint_hidden_bwd_band(hip_lib, name, J, dtype):
    from edgedict_amd import _lib
    from edgedict_amd.ops import _ll
    al, ll, T, U1, windows = BWD_CASES[name]
    lo, hi = windows()
    B = len(al)
    plan = _plan(lo, hi, al, ll, T)
    band = plan.band.cpu().numpy()
    M = plan.rows
    g = torch.Generator(device="cpu").manual_seed(3 * J + T)
    hid = torch.tanh(torch.randn(M, J, generator=g)).to(dtype).cuda()
    dhid = torch.randn(M, J, generator=g).to(dtype).cuda()
    dE1 = torch.full((B, T, J), float("nan"), device="cuda")
    dD1 = torch.full((B, U1, J), float("nan"), device="cuda")
    _lib.call("joint_hidden_bwd_band", _lib.dtype_code(dtype), dhid, hid, dE1, dD1, plan.band, plan.row_off, _ll(M),
              B, T, U1, J)
    torch.cuda.synchronize()
    dpre = dhid.double().cpu() * (1.0 - hid.double().cpu() ** 2)      # float64 of the operands as stored
    dense = BR.band_unpack(dpre, band, 0.0, U1)
    rE, rD = dense.sum(2), dense.sum(1)
    dE1, dD1 = dE1.cpu().double(), dD1.cpu().double()
    # test_joint_hidden_bwd_packed's bound
    tolE = 1e-4 * max(1.0, rE.abs().max().item())
    tolD = 1e-4 * max(1.0, rD.abs().max().item())
    print("joint_hidden_bwd_band", name, J, dtype, (dE1 - rE).abs().max().item(), (dD1 - rD).abs().max().item())
    assert ((dE1 - rE).abs() <= tolE).all(), ((dE1 - rE).abs().max().item(), tolE)
    assert ((dD1 - rD).abs() <= tolD).all(), ((dD1 - rD).abs().max().item(), tolD)
    live = torch.tensor(AR.live_from_band(band, U1))
    frame_dead, col_dead = ~live.any(2), ~live.any(1)
    assert frame_dead.any() and col_dead.any()
    assert (dE1[frame_dead] == 0).all() and (dD1[col_dead] == 0).all()
    for b in range(B):
        assert (dE1[b, al[b]:] == 0).all()
        if int(plan.cells[b]) == 0:
            assert (dE1[b] == 0).all() and (dD1[b] == 0).all()
    assert ("infeasible" in name) == bool((plan.cells == 0).any())
    # the label passes: 72 positions each, counted from the slab's first live column
    spans = _slab_spans(band, B, T, J)
    print("   slab spans up to", max(spans))
    if name.startswith("S-"):
        assert max(spans) > 144 and 72 < sorted(spans)[-2] <= 144      # three passes, and two
    else:
        assert max(spans) <= 72


# ------------------------------------------------------------------------------- 6. _JointLossFn with and without a plan
def _record_calls(monkeypatch):
    return TA._record_calls(monkeypatch)


def _band_route(names):
    """the band entry points among the recorded calls (rnnt_band itself is the box path's table, not a route)"""
    return [n for n in names if "_band" in n and n != "rnnt_band"]


def _joint_loss(plan, lo, hi, names):
    from edgedict_amd import ops
    from edgedict_amd.models import _JointLossFn
    B, T, U1, P, J, V = W_B, W_T, W_U1, TP.E_P, 128, 264
    g = torch.Generator(device="cpu").manual_seed(17)
    rnd = lambda *s: torch.randn(*s, generator=g)
    enc = rnd(B, T, P).to(BF16).cuda().requires_grad_(True)
    dec = rnd(B, U1, P).to(BF16).cuda().requires_grad_(True)
    w1 = torch.nn.Parameter((rnd(J, 2 * P) / (2 * P) ** 0.5).cuda())
    b1 = torch.nn.Parameter((0.1 * rnd(J)).cuda())
    w2 = torch.nn.Parameter((rnd(V, J) / J ** 0.5).cuda())
    b2 = torch.nn.Parameter((0.1 * rnd(V)).cuda())
    labels = torch.randint(1, V, (B, U1 - 1), generator=g, dtype=torch.int32).cuda()
    del names[:]
    loss = _JointLossFn.apply(enc, dec, w1, b1, w2, b2, labels, torch.tensor(W_AL, dtype=torch.int32),
                              torch.tensor(W_LL, dtype=torch.int32), 0, BF16, 0.5, _dev(lo), _dev(hi), plan)
    loss.backward()
    torch.cuda.synchronize()
    out = dict(denc=enc.grad, ddec=dec.grad, dW1=w1.grad, db1=b1.grad, dW2=w2.grad, db2=b2.grad)
    out = {k: v.detach().double().cpu() for k, v in out.items()}
    out["costs"] = ops.LAST["joint_costs"].detach().double().cpu()
    return loss.detach().clone(), out, list(names), ops.LAST["joint_rows"], ops.LAST["joint_packed_rows"]


@pytest.mark.parametrize("slack", [(5, 5), (0, 0)], ids=["slack55", "slack00"])
@pytest.mark.parametrize("fused", [True, False], ids=["fused_lse", "plain_lse"])
def test_joint_loss_fn_with_a_plan_is_the_box_path(hip_lib, monkeypatch, slack, fused):
    from edgedict_amd import config
    lo, hi = TH.w_windows(*slack)
    plan = _plan(lo, hi, W_AL, W_LL, W_T)
    names = _record_calls(monkeypatch)
    saved = config.FUSED_LSE
    config.FUSED_LSE = fused
    try:
        l_box, g_box, n_box, rows_box, packed_box = _joint_loss(None, lo, hi, names)
        l_band, g_band, n_band, rows_band, packed_band = _joint_loss(plan, lo, hi, names)
    finally:
        config.FUSED_LSE = saved
    assert rows_box == rows_band == packed_box == 4843
    assert packed_band == plan.rows < rows_band and plan.rows == {(5, 5): 1363, (0, 0): 232}[slack]
    assert not _band_route(n_box)
    want_fwd = "rnnt_loss_forward_band_parts" if fused and plan.rows >= 256 else "rnnt_loss_forward_band"
    assert {"joint_hidden_fwd_band", want_fwd, "rnnt_loss_backward_band_colsum", "joint_hidden_bwd_band"} <= set(n_band)
    assert not [n for n in n_band if n.startswith("rnnt_loss_backward_packed") or n.startswith("rnnt_loss_forward_packed")
                or n.startswith("joint_hidden_fwd_packed") or n.startswith("joint_hidden_bwd_packed")]
    assert ("rnnt_loss_forward_packed_parts_ar" in n_box) == fused
    print("band _JointLossFn", slack, fused, l_box.item(), l_band.item())
    assert torch.isfinite(l_band).all()
    np.testing.assert_allclose(l_band.item(), l_box.item(), rtol=1e-4)
    np.testing.assert_allclose(g_band["costs"].numpy(), g_box["costs"].numpy(), rtol=1e-4)
    # test_joint_loss_fn_bf16's bound (packed against its reference), here band against box
    for k in ("denc", "ddec", "dW1", "db1", "dW2", "db2"):
        err = (g_band[k] - g_box[k]).abs().max().item()
        ref = g_box[k].abs().max().item()
        print("   ", k, "%.3g of %.3g" % (err, ref))
        assert err <= 4 * TP.E_BF16_MEASURED[k] * ref, (k, err, ref)


# ------------------------------------------------------------------------------------------------------ 7. model level
def _model_windows(model, xs, ys, xlen, ylen):
    from edgedict_amd.loss import alignment_windows
    model.eval()
    frames, _ = model.align(xs.cuda(), ys.cuda(), xlen, ylen)
    model.train()
    with torch.no_grad():
        act = model.scale_length(model.encoder(xs[:, :xlen.max()].cuda())[0], xlen)
    return alignment_windows(frames, act.to(torch.int32).cuda(), ylen.to(torch.int32).cuda(), 1, 1), act


def _model_run(cfg, sd, batch, lam, windows, flag, names=None):
    from edgedict_amd import config, ops
    xs, ys, xlen, ylen = batch
    m = TF._engine(cfg, sd, True, lam)
    saved = config.BAND_LATTICE
    config.BAND_LATTICE = flag
    try:
        if names is not None:
            del names[:]
        loss = m(xs.cuda(), ys.cuda(), xlen, ylen) if windows is None else m(xs.cuda(), ys.cuda(), xlen, ylen, windows=windows)
        loss.backward()
        torch.cuda.synchronize()
    finally:
        config.BAND_LATTICE = saved
    return m, loss.detach().clone(), (list(names) if names is not None else None), dict(ops.LAST)


def _grads_close(a, b):
    for (n, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert torch.isfinite(p.grad).all(), n
        scale = max(q.grad.abs().max().item(), 1e-8)
        assert (p.grad - q.grad).abs().max().item() <= 2e-5 * scale, n          # the existing packed-against-dense bound


def test_model_with_the_flag_on_is_the_box_path(hip_lib, monkeypatch):
    cfg, sd, batch = TF._tiny()
    xs, ys, xlen, ylen = batch
    lam = 0.5
    windows, act = _model_windows(TF._engine(cfg, sd, True, lam), xs, ys, xlen, ylen)
    names = _record_calls(monkeypatch)
    box, l_box, n_box, _ = _model_run(cfg, sd, batch, lam, windows, False, names)
    band, l_band, n_band, last = _model_run(cfg, sd, batch, lam, windows, True, names)
    assert not _band_route(n_box) and [n for n in n_box if n.endswith("_packed_ar") or "_packed_colsum_ar" in n]
    assert {"rnnt_band", "rnnt_band_offsets", "rnnt_band_rows", "joint_hidden_fwd_band", "joint_hidden_bwd_band"} <= set(n_band)
    assert not [n for n in n_band if n.endswith("_ar") or n.startswith(("rnnt_loss_forward_packed", "rnnt_loss_backward_packed",
                                                                        "joint_hidden_fwd_packed", "joint_hidden_bwd_packed"))]
    assert 0 < last["joint_packed_rows"] < last["joint_rows"] and int(last["joint_band_rows"]) == last["joint_packed_rows"]
    # the loss is the oracle's on the model's own logits
    logit_model = TF._engine(cfg, sd, False, 0.0)
    with torch.no_grad():
        logits = logit_model(xs.cuda(), ys.cuda(), xlen.cuda(), ylen.cuda())
    U = int(ylen.max())
    lo, hi = windows[0].cpu().numpy(), windows[1].cpu().numpy()
    costs, _, _ = AR.ar_loss(logits.double().cpu().numpy(), ys[:, :U].numpy(), act.numpy(), ylen.numpy(), lo, hi, lam)
    print("band model", l_band.item(), l_box.item(), costs.mean())
    np.testing.assert_allclose(l_band.item(), costs.mean(), rtol=1e-5, atol=1e-4)
    np.testing.assert_allclose(l_box.item(), costs.mean(), rtol=1e-5, atol=1e-4)
    _grads_close(band, box)
    # one utterance without an alignment: +inf, the other utterances' gradient
    B = xs.shape[0]
    b = int(np.argmax(ylen.numpy() >= 2))
    lo2, hi2 = lo.copy(), hi.copy()
    lo2[b], hi2[b] = TA._infeasible(lo[b], hi[b], int(act[b]), int(ylen[b]), "order")
    assert not AR.band_one(int(act[b]), int(ylen[b]), lo2[b], hi2[b])[1]
    w2 = (_dev(lo2), _dev(hi2))
    box2, l_box2, _, _ = _model_run(cfg, sd, batch, lam, w2, False)
    band2, l_band2, n2, last2 = _model_run(cfg, sd, batch, lam, w2, True, names)
    assert l_box2.item() == float("inf") and l_band2.item() == float("inf")
    assert "joint_hidden_fwd_band" in n2 and 0 < last2["joint_packed_rows"] < last["joint_packed_rows"]
    _grads_close(band2, box2)
    # every utterance without one: +inf, nothing launched on the joint, exact zeros
    assert int(ylen.min()) >= 1
    w3 = (_dev(np.full_like(lo, 10 ** 6)), _dev(np.full_like(hi, 10 ** 6)))
    band3, l_band3, n3, last3 = _model_run(cfg, sd, batch, lam, w3, True, names)
    assert l_band3.item() == float("inf") and last3["joint_packed_rows"] == 0
    assert not [n for n in n3 if "joint_hidden" in n or "rnnt_loss" in n or n == "gemm_nt_lse"]
    for n, p in band3.named_parameters():
        assert torch.isfinite(p.grad).all(), n
        if n.startswith("joint."):
            assert (p.grad == 0).all(), n
    # no windows: the flag changes nothing
    _, l_off, n_off, _ = _model_run(cfg, sd, batch, lam, None, False, names)
    _, l_on, n_on, last_on = _model_run(cfg, sd, batch, lam, None, True, names)
    assert n_on == n_off and torch.equal(l_on, l_off) and not _band_route(n_on)
    assert last_on["joint_packed_rows"] == last_on["joint_rows"]


def test_train_engine_steps_on_the_band(hip_lib, monkeypatch):
    """train_step(..., windows=) with host-side sample counts (the packed path), whole and in sub-batches: the band
    entry points run, the loss is the box path's, the parameters move."""
    from edgedict_amd import config, ops
    from edgedict_amd.trainer import TrainEngine
    g = torch.Generator(device="cpu").manual_seed(5)
    wave = (0.1 * torch.randn(4, 9600, generator=g)).cuda()
    wave_len = torch.tensor([9600, 9600, 8640, 9600], dtype=torch.int32)         # on the HOST
    ys = torch.randint(4, 40, (4, 6), generator=g, dtype=torch.int32).cuda()
    ylen = torch.tensor([6, 4, 5, 6], dtype=torch.int32)
    lo = (torch.arange(6, dtype=torch.int32) // 2).repeat(4, 1).contiguous().cuda()
    hi = (lo + 4).contiguous()
    names = _record_calls(monkeypatch)
    saved = config.BAND_LATTICE
    losses = {}
    for sub in (None, 2):
        for flag in (False, True):
            eng = None
            try:
                config.BAND_LATTICE = flag
                torch.manual_seed(0)
                fl = TF._flags()
                fl.sub_batch_size = sub
                eng = TrainEngine(fl, vocab_size=40, device="cuda", compute_dtype="fp32")
                before = [p.detach().clone() for p in eng.model.parameters()]
                del names[:]
                loss = eng.train_step(wave, wave_len, ys, ylen, windows=(lo, hi))
                torch.cuda.synchronize()
                losses[(sub, flag)] = loss.detach().clone()
                assert torch.isfinite(loss).all()
                route = _band_route(names)
                if flag:
                    assert {"rnnt_band_offsets", "rnnt_band_rows", "joint_hidden_fwd_band", "joint_hidden_bwd_band"} <= set(route)
                    assert names.count("joint_hidden_fwd_band") == (1 if sub is None else 2)
                    assert not [n for n in names if n.endswith("_ar")]
                    assert 0 < ops.LAST["joint_packed_rows"] < ops.LAST["joint_rows"]
                else:
                    assert not route and [n for n in names if n.endswith("_packed_ar")]
                moved = [not torch.equal(a, p.detach()) for a, p in zip(before, eng.model.parameters())]
                assert all(torch.isfinite(p).all() for p in eng.model.parameters()) and sum(moved) > len(moved) // 2
            finally:
                config.BAND_LATTICE = saved
                if eng is not None:
                    eng.close()
        # fp32, same logits per cell: the band loss is the box loss up to the order of the mean's fp32 sum
        assert torch.allclose(losses[(sub, True)], losses[(sub, False)], rtol=1e-5, atol=1e-4), (sub, losses)
