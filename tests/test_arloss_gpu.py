"""GPU: the alignment-restricted RNN-T loss (per-label emission windows) against the float64 restatement
tests/arloss_ref.py (pinned by tests/test_arloss_host.py), through every route the loss takes: the dense operator, the
packed lattice (fp32, bf16, bf16 with the logits product's log-sum-exp partials), utterance ranges, the fused column sums,
the forced aligner, Transducer.forward / align on both of their paths and TrainEngine.

Bounds are those the project holds the plain and the FastEmit gradient to (tests/test_fastemit_gpu.py): fp32 cost
rtol 1e-5 / atol 1e-4, gradient (1 + lambda) (1e-3 |g| + 2e-5); bf16 cost rtol 1e-4, gradient (1 + lambda) 4e-3, the
oracle seeing the bf16-rounded logits.  Windows that cover every frame must be the plain entry points bit for bit."""
import numpy as np
import pytest
import torch

import arloss_ref as AR
import fastemit_ref as FR
import test_fastemit_gpu as TF
from oracle import packed_ref as PR

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
LAMBDAS = [0.0, 0.5]
SLACKS = [(0, 0), (2, 1)]


def _dev(a, dtype=torch.int32):
    return torch.tensor(np.asarray(a), dtype=dtype, device="cuda").contiguous()


def _dense_case(B, T, U1, V, ragged):
    acts, labels, al, ll = TF._case(B * 1000 + T, B, T, U1, V, bool(ragged))
    if ragged == "u0":
        ll[1] = 0
    return acts, labels, al, ll


def _run(acts, labels, al, ll, dtype, lam, windows, reduction="none"):
    """(costs, gradient) of RNNTLoss on the device; windows = (lo, hi) numpy arrays or None."""
    from edgedict_amd.loss import RNNTLoss
    ta = torch.tensor(acts, device="cuda").to(dtype).requires_grad_(True)
    w = None if windows is None else (_dev(windows[0]), _dev(windows[1]))
    loss = RNNTLoss(blank=0, reduction=reduction, fastemit_lambda=lam)(ta, _dev(labels), _dev(al), _dev(ll), windows=w)
    (loss.sum() if reduction == "none" else loss).backward()
    return loss.detach().clone(), ta.grad


def _check(cost, g, costs, grads, dtype, lam, what, scale=1.0):
    """the project's bounds; `scale` = the factor on the whole gradient (1 / B under 'mean')"""
    err = np.abs(g.double().cpu().numpy() - grads)
    print("arloss", what, dtype, "lambda", lam, "max err %.3g" % err.max())
    if cost is not None:
        np.testing.assert_allclose(cost.cpu().numpy(), costs, rtol=1e-5 if dtype == F32 else 1e-4,
                                   atol=1e-4 if dtype == F32 else 0.0)
    if dtype == F32:
        assert (err <= (1 + lam) * (1e-3 * np.abs(grads) + 2e-5 * scale)).all(), (what, lam, err.max())
    else:
        assert (err <= (1 + lam) * 4e-3 * scale).all(), (what, lam, err.max())


def _infeasible(lo, hi, T, U, how):
    """windows of one utterance made impossible: 'cross' = lo > hi on one label; 'order' = the first label not before
    the last frame, the second not after the first (needs T, U >= 2)."""
    lo, hi = lo.copy(), hi.copy()
    if how == "cross":
        lo[U // 2], hi[U // 2] = min(T - 1, 1), min(T - 1, 1) - 1
    else:
        lo[0], hi[0], lo[1], hi[1] = T - 1, T - 1, 0, 0
    return lo, hi


# ------------------------------------------------------------------------------------------------------------ dense
@pytest.mark.parametrize("B,T,U1,V,ragged", TF.DENSE_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_dense_cost_gradient_and_live_cells(hip_lib, B, T, U1, V, ragged, dtype):
    from edgedict_amd import loss as L
    acts, labels, al, ll = _dense_case(B, T, U1, V, ragged)
    U = U1 - 1
    seen = torch.tensor(acts).to(dtype).double().numpy()             # bf16: the oracle sees the rounded logits
    rng = np.random.default_rng(B * 100 + T)
    frames = AR.random_alignment(rng, al, ll, U)
    al_d, ll_d, ta = _dev(al), _dev(ll), torch.tensor(acts, device="cuda").to(dtype)
    kinds = []
    for left, right in SLACKS:
        lo_d, hi_d = L.alignment_windows(_dev(frames), al_d, ll_d, left, right)
        lo, hi = AR.windows_from_frames(frames, al, ll, left, right, Tm=T)
        assert lo_d.cpu().numpy().tolist() == lo.tolist() and hi_d.cpu().numpy().tolist() == hi.tolist()
        kinds.append(("align%d%d" % (left, right), lo, hi))
    kinds.append(("cover", np.zeros((B, U), np.int32), np.full((B, U), T - 1, np.int32)))
    for name, lo, hi in kinds:
        # live cells: isfinite(alpha) & isfinite(beta) of the workspace = the band table = the oracle's
        _, _, alphas, betas, lls = L.rnnt_loss_debug(ta, _dev(labels), al_d, ll_d, windows=(_dev(lo), _dev(hi)))
        band, cells = L.rnnt_band(_dev(lo), _dev(hi), al_d, ll_d, T)
        inside = (np.arange(T)[None, :, None] < al[:, None, None]) & (np.arange(U1)[None, None, :] <= ll[:, None, None])
        live_ws = (torch.isfinite(alphas) & torch.isfinite(betas)).cpu().numpy() & inside
        want_band, want_cells = AR.band_table(lo, hi, al, ll, T)
        assert band.cpu().numpy().tolist() == want_band.tolist(), name
        assert cells.dtype == torch.int64 and cells.cpu().numpy().tolist() == want_cells.tolist()
        assert (AR.live_from_band(band.cpu().numpy(), U1) == live_ws).all(), name
        assert live_ws.sum((1, 2)).tolist() == want_cells.tolist()
        for lam in LAMBDAS:
            costs, grads, live = AR.ar_loss(seen, labels, al, ll, lo, hi, lam)
            assert (live == live_ws).all()
            cost, g = _run(acts, labels, al, ll, dtype, lam, (lo, hi))
            assert torch.isfinite(g.float()).all() and torch.isfinite(cost).all()
            _check(cost, g, costs, grads, dtype, lam, "dense %s %s" % ((B, T, U1, V), name))
            assert (g.cpu()[torch.tensor(~live)] == 0).all()         # dead cells and cells outside the boxes: exact zeros
            if name == "cover" and lam == 0.0:
                c0, g0 = _run(acts, labels, al, ll, dtype, 0.0, None)
                assert torch.equal(cost, c0) and torch.equal(g, g0)  # covering windows: the plain loss, bit for bit
            if name == "align00":
                for b in range(B):                                   # one path per utterance: its score is the cost
                    lpb, lpl = FR.cell_logprobs(seen[b], labels[b], int(al[b]), int(ll[b]))
                    want = -FR.path_score(lpb, lpl, frames[b, :int(ll[b])])
                    np.testing.assert_allclose(cost[b].item(), want, rtol=1e-5 if dtype == F32 else 1e-4, atol=1e-4)
        if name == "align21":
            lam = 0.5
            cm, gm = _run(acts, labels, al, ll, dtype, lam, (lo, hi), reduction="mean")
            assert cm.shape == (1,)
            np.testing.assert_allclose(cm.item(), costs.mean(), rtol=1e-5 if dtype == F32 else 1e-4, atol=1e-4)
            _check(None, gm, None, grads / B, dtype, lam, "dense mean", scale=1.0 / B)


@pytest.mark.parametrize("B,T,U1,V,ragged", [s for s in TF.DENSE_SHAPES if s[0] > 1 and s[2] > 1], ids=lambda v: str(v))
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_infeasible_utterance_is_inf_zero_and_leaves_the_others_alone(hip_lib, B, T, U1, V, ragged, dtype):
    acts, labels, al, ll = _dense_case(B, T, U1, V, ragged)
    U = U1 - 1
    rng = np.random.default_rng(7 + T)
    frames = AR.random_alignment(rng, al, ll, U)
    lo, hi = AR.windows_from_frames(frames, al, ll, 2, 1, Tm=T)
    hows = ["cross"] + (["order"] if T >= 2 and U >= 2 else [])       # utterance 0 has T frames and U labels
    for lam in LAMBDAS:
        c_ok, g_ok = _run(acts, labels, al, ll, dtype, lam, (lo, hi))
        for how in hows:
            lo2, hi2 = lo.copy(), hi.copy()
            lo2[0], hi2[0] = _infeasible(lo[0], hi[0], T, U, how)
            assert not AR.band_one(T, U, lo2[0], hi2[0])[1]
            for reduction in ("none", "mean"):
                c, g = _run(acts, labels, al, ll, dtype, lam, (lo2, hi2), reduction=reduction)
                assert not torch.isnan(g.float()).any() and not torch.isnan(c).any()
                assert (g[0] == 0).all()
                if reduction == "none":
                    assert c[0].item() == float("inf")
                    assert torch.equal(c[1:], c_ok[1:]) and torch.equal(g[1:], g_ok[1:])
                else:
                    assert c.item() == float("inf")
                    tol = (1e-3 * g_ok[1:].abs() / B + 2e-5 / B) if dtype == F32 else 4e-3 / B
                    assert ((g[1:].float() - g_ok[1:].float() / B).abs() <= (1 + lam) * tol).all()
    # the aligner on the same windows: score -inf and frames of all -1 for that row, the others untouched
    from edgedict_amd.loss import rnnt_align
    ta = torch.tensor(acts, device="cuda").to(dtype)
    f_ok, s_ok = rnnt_align(ta, _dev(labels), _dev(al), _dev(ll), windows=(_dev(lo), _dev(hi)))
    f, s = rnnt_align(ta, _dev(labels), _dev(al), _dev(ll), windows=(_dev(lo2), _dev(hi2)))
    assert s[0].item() == float("-inf") and (f[0] == -1).all()
    assert torch.equal(f[1:], f_ok[1:]) and torch.equal(s[1:], s_ok[1:]) and torch.isfinite(s_ok).all()


@pytest.mark.parametrize("B,T,U1,V", [(3, 7, 5, 11), (4, 33, 9, 64)], ids=lambda v: str(v))
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_dense_dead_rows_are_not_read(hip_lib, B, T, U1, V, dtype):
    """NaN in the logits of every dead cell (chosen by the band table) between the forward and the backward call: the
    gradient is the one of the clean logits, bit for bit."""
    from edgedict_amd import _lib, loss as L
    acts, labels, al, ll = _dense_case(B, T, U1, V, True)
    rng = np.random.default_rng(3)
    frames = AR.random_alignment(rng, al, ll, U1 - 1)
    lo, hi = AR.windows_from_frames(frames, al, ll, 1, 1, Tm=T)
    lo[B - 1], hi[B - 1] = T - 1, 0                                  # and one utterance without any alignment
    if ll[B - 1] == 0:
        ll[B - 1] = 1
    ta = torch.tensor(acts, device="cuda").to(dtype)
    args = (_dev(labels), _dev(al), _dev(ll))
    code = _lib.dtype_code(dtype)
    ws = torch.zeros(hip_lib.edgedict_rnnt_workspace_bytes(B, T, U1), dtype=torch.uint8, device="cuda")
    costs = torch.empty(B, device="cuda")
    _lib.call("rnnt_loss_forward_ar", ta, code, *args, _dev(lo), _dev(hi), B, T, U1, V, 0, costs, None, 1.0, ws)
    band, cells = L.rnnt_band(_dev(lo), _dev(hi), args[1], args[2], T)
    live = torch.tensor(AR.live_from_band(band.cpu().numpy(), U1), device="cuda")
    assert int(cells[B - 1]) == 0 and 0 < int(live.sum()) < int((args[1] * (args[2] + 1)).sum())
    poisoned = ta.clone()
    poisoned[~live] = float("nan")
    for lam in LAMBDAS:
        clean, dirty = torch.full_like(ta, 7.0), torch.full_like(ta, 7.0)
        _lib.call("rnnt_loss_backward_ar", ta, code, clean, *args, B, T, U1, V, 0, ws, 1.0, None, 0, lam)
        _lib.call("rnnt_loss_backward_ar", poisoned, code, dirty, *args, B, T, U1, V, 0, ws, 1.0, None, 0, lam)
        torch.cuda.synchronize()
        assert torch.isfinite(dirty.float()).all() and torch.equal(clean, dirty)
        assert (dirty[~live] == 0).all() and costs[B - 1].item() == float("inf")
        seen = ta.double().cpu().numpy()
        _, grads, _ = AR.ar_loss(seen, labels, al, ll, lo, hi, lam)
        _check(None, dirty, None, grads, dtype, lam, "poisoned dense")


# --------------------------------------------------------------------------------------------------- packed routes
P_B, P_T, P_U1 = TF.P_B, TF.P_T, TF.P_U1
P_AL, P_LL = TF.P_AL, TF.P_LL


class _PackedAr(TF._Packed):
    """test_fastemit_gpu._Packed (logits of the logits product, the three plain forward routes) plus the three routes
    of the restricted forward under one set of windows."""

    def restrict(self, lo, hi):
        from edgedict_amd import _lib
        self.lo, self.hi = lo, hi
        self.lo_d, self.hi_d = _dev(lo), _dev(hi)
        self.ws_plain, self.costs_plain = self.ws, self.costs
        self.ws, self.costs = {}, {}
        B, T, U1, V = P_B, P_T, P_U1, self.V
        slots = (V + 63) // 64
        # log-sum-exp partials of the stored logits (_Packed does not keep the product's own); the plain partials
        # route is run again on them, so that the plain and the restricted workspace come from the same inputs
        hidless = torch.full((self.M, slots, 2), float("nan"), device="cuda")
        self._parts_from_logits(hidless)
        self.ws_plain["parts"] = torch.zeros_like(self.ws_plain["f32"])
        _lib.call("rnnt_loss_forward_packed_parts", self.logits[BF16], self.labels, self.al_d, self.ll_d, self.off_d,
                  B, T, U1, V, 0, self.costs_plain["parts"], torch.empty(1, device="cuda"), 1.0 / B,
                  self.ws_plain["parts"], hidless, slots)
        for route in ("f32", "bf16", "parts"):
            w = self.ws[route] = torch.zeros_like(self.ws_plain[route])
            c = self.costs[route] = torch.empty(B, device="cuda")
            red = torch.empty(1, device="cuda")
            if route == "parts":
                _lib.call("rnnt_loss_forward_packed_parts_ar", self.logits[BF16], self.labels, self.al_d, self.ll_d,
                          self.lo_d, self.hi_d, self.off_d, B, T, U1, V, 0, c, red, 1.0 / B, w, hidless, slots)
            else:
                dt = self.dtype(route)
                _lib.call("rnnt_loss_forward_packed_ar", self.logits[dt], _lib.dtype_code(dt), self.labels, self.al_d,
                          self.ll_d, self.lo_d, self.hi_d, self.off_d, B, T, U1, V, 0, c, red, 1.0 / B, w)
        torch.cuda.synchronize()
        self.parts = hidless
        return self

    def _parts_from_logits(self, out):
        """(max, sum exp(x - max)) of every 64-column slot of the stored bf16 logits: the layout the product's epilogue
        writes (gemm_nt_lse), formed from the logits the oracle sees."""
        x = self.logits[BF16].float()
        V = self.V
        slots = (V + 63) // 64
        pad = slots * 64 - V
        if pad:
            x = torch.cat([x, torch.full((self.M, pad), float("-inf"), device="cuda")], 1)
        x = x.view(self.M, slots, 64)
        m = x.max(-1).values
        out[:, :, 0] = m
        out[:, :, 1] = torch.exp(x - m[..., None]).sum(-1)

    def oracle_ar(self, lam):
        dense = PR.unpack(self.logits[F32].cpu().double(), P_AL, P_LL, T=P_T, U1=P_U1, fill=0.0)
        costs, grads, live = AR.ar_loss(dense.numpy(), self.labels.cpu().numpy(), P_AL, P_LL, self.lo, self.hi, lam)
        return costs, PR.pack(torch.tensor(grads), P_AL, P_LL) / P_B, PR.pack(torch.tensor(live), P_AL, P_LL)


def _packed_windows(kind, seed):
    rng = np.random.default_rng(seed)
    U = P_U1 - 1
    frames = AR.random_alignment(rng, P_AL, P_LL, U)
    if kind == "cover":
        return np.zeros((P_B, U), np.int32), np.full((P_B, U), P_T - 1, np.int32)
    lo, hi = AR.windows_from_frames(frames, P_AL, P_LL, 2, 1, Tm=P_T)
    if kind == "infeasible":
        lo[2], hi[2] = _infeasible(lo[2], hi[2], P_AL[2], P_LL[2], "order")
    return lo.astype(np.int32), hi.astype(np.int32)


@pytest.mark.parametrize("V", [264, 1024])            # both inside the fused column sums' limits (fp32: V <= 1024)
def test_packed_routes_match_oracle_and_each_other(hip_lib, V):
    from edgedict_amd import _lib
    lib = hip_lib
    B, T, U1 = P_B, P_T, P_U1
    for kind in ("align", "infeasible"):
        pk = _PackedAr(lib, V, seed=V).restrict(*_packed_windows(kind, V))
        for lam in LAMBDAS:
            costs, want, live = pk.oracle_ar(lam)
            want, live = want.cuda(), live.cuda()
            for route in ("f32", "bf16", "parts"):
                dt = pk.dtype(route)
                code = _lib.dtype_code(dt)
                np.testing.assert_allclose(pk.costs[route].cpu().numpy(), costs, rtol=1e-5 if dt == F32 else 1e-4,
                                           atol=1e-4 if dt == F32 else 0.0)
                assert (kind == "infeasible") == (pk.costs[route][2].item() == float("inf"))
                got = pk.backward(route, "backward_packed_ar", lam)
                assert torch.isfinite(got.float()).all()
                # test_fastemit_gpu's bounds (total row scale 1 / B), times 1 + lambda
                tol = (1e-3 * want.abs() + 2e-5 / B) if dt == F32 else torch.full_like(want, 4e-3 / B)
                err = (got.double() - want).abs()
                print("arloss packed", V, kind, route, lam, "max err %.3g" % err.max().item())
                assert (err <= (1 + lam) * tol).all(), (route, lam, err.max().item())
                assert (got[~live] == 0).all()
                # dead rows are not read: NaN logits there, the same gradient bit for bit
                saved = pk.logits[dt]
                pk.logits[dt] = saved.clone()
                pk.logits[dt][~live] = float("nan")
                try:
                    assert torch.equal(pk.backward(route, "backward_packed_ar", lam), got)
                    n = lib.edgedict_rnnt_grad_colsum_rows(code, B, T, U1, V)
                    cs_dirty = torch.full((n, V), float("nan"), device="cuda")
                    assert torch.equal(pk.backward(route, "backward_packed_colsum_ar", cs_dirty, lam), got)
                    assert torch.isfinite(cs_dirty).all()
                finally:
                    pk.logits[dt] = saved
                # utterance ranges write exactly the one-pass gradient, other utterances' rows untouched
                parts = torch.full_like(got, 7.0)
                for b0, nb in ((0, 2), (2, 0), (2, 3)):
                    _lib.call("rnnt_loss_backward_packed_range_ar", pk.logits[dt], code, parts, pk.labels, pk.al_d,
                              pk.ll_d, pk.off_d, B, T, U1, V, 0, pk.ws[route], 1.0 / B, None, 0, b0, nb, lam)
                    if (b0, nb) == (0, 2):
                        torch.cuda.synchronize()
                        assert (parts[int(pk.off[2]):] == 7.0).all()
                torch.cuda.synchronize()
                assert torch.equal(parts, got), (route, lam)
                # fused column sums: the same matrix bit for bit, partial rows that add up to its column sums
                assert n > 0
                cs = torch.full((n, V), float("nan"), device="cuda")
                fused = pk.backward(route, "backward_packed_colsum_ar", cs, lam)
                assert torch.equal(fused, got), (route, lam)
                assert torch.equal(cs, cs_dirty)
                ctol = 1e-5 if dt == F32 else 2.0 ** -8
                assert ((cs.double().sum(0) - got.double().sum(0)).abs() <= ctol * got.double().abs().sum(0) + 1e-12).all()
                assert ((cs.double().sum(0) - want.sum(0)).abs() <= ctol * (1 + lam) * want.abs().sum(0) + 1e-12).all()
                if route == "parts":
                    continue
                # packed == dense inside the boxes (same arithmetic per cell), exact zeros outside
                dense_logits = PR.unpack(pk.logits[dt].cpu(), P_AL, P_LL, T=T, U1=U1, fill=0.0).cuda().contiguous()
                ws = torch.zeros_like(pk.ws[route])
                dcosts, red = torch.empty(B, device="cuda"), torch.empty(1, device="cuda")
                _lib.call("rnnt_loss_forward_ar", dense_logits, code, pk.labels, pk.al_d, pk.ll_d, pk.lo_d, pk.hi_d, B, T,
                          U1, V, 0, dcosts, red, 1.0 / B, ws)
                dg = torch.full_like(dense_logits, float("nan"))
                _lib.call("rnnt_loss_backward_ar", dense_logits, code, dg, pk.labels, pk.al_d, pk.ll_d, B, T, U1, V, 0, ws,
                          1.0 / B, None, 0, lam)
                torch.cuda.synchronize()
                assert torch.equal(dcosts, pk.costs[route])
                assert torch.equal(PR.pack(dg.cpu(), P_AL, P_LL), got.cpu()), (route, lam)
                assert torch.equal(PR.unpack(got.cpu(), P_AL, P_LL, T=T, U1=U1, fill=0.0), dg.cpu())
        # the aligner's packed entry points under the same windows
        for route in ("f32", "bf16", "parts"):
            dt = pk.dtype(route)
            frames = torch.full((B, U1 - 1), 99, dtype=torch.int32, device="cuda")
            scores = torch.empty(B, device="cuda")
            ws = torch.zeros_like(pk.ws[route])
            if route == "parts":
                _lib.call("rnnt_align_packed_parts_ar", pk.logits[BF16], pk.labels, pk.al_d, pk.ll_d, pk.lo_d, pk.hi_d,
                          pk.off_d, B, T, U1, V, 0, frames, scores, ws, pk.parts, (V + 63) // 64)
            else:
                _lib.call("rnnt_align_packed_ar", pk.logits[dt], _lib.dtype_code(dt), pk.labels, pk.al_d, pk.ll_d, pk.lo_d,
                          pk.hi_d, pk.off_d, B, T, U1, V, 0, frames, scores, ws)
            fr, sc = frames.cpu().numpy(), scores.cpu().numpy()
            dense = PR.unpack(pk.logits[F32].cpu().double(), P_AL, P_LL, T=T, U1=U1, fill=0.0).numpy()
            for b in range(B):
                Tb, Ub = P_AL[b], P_LL[b]
                lpb, lpl = FR.cell_logprobs(dense[b], pk.labels[b].cpu().numpy(), Tb, Ub)
                want, _ = AR.ar_viterbi_one(lpb, lpl, pk.lo[b], pk.hi[b])
                assert (fr[b, Ub:] == -1).all()
                if want == -np.inf:
                    assert sc[b] == -np.inf and (fr[b] == -1).all() and kind == "infeasible" and b == 2
                    continue
                assert AR.respects(fr[b, :Ub], pk.lo[b], pk.hi[b]) and (np.diff(fr[b, :Ub]) >= 0).all()
                np.testing.assert_allclose(sc[b], want, rtol=1e-5 if dt == F32 else 1e-4, atol=1e-4)
                np.testing.assert_allclose(FR.path_score(lpb, lpl, fr[b, :Ub]), want, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("V", [264, 1024])
def test_covering_windows_are_the_plain_entry_points_bit_for_bit(hip_lib, V):
    from edgedict_amd import _lib
    lib = hip_lib
    pk = _PackedAr(lib, V, seed=3 + V).restrict(*_packed_windows("cover", V))
    B, T, U1 = P_B, P_T, P_U1
    for route in ("f32", "bf16", "parts"):
        assert torch.equal(pk.costs[route], pk.costs_plain[route])
        assert torch.equal(pk.ws[route], pk.ws_plain[route])         # the whole workspace: denominators, alpha, beta, L
        dt = pk.dtype(route)
        code = _lib.dtype_code(dt)
        ar_ws, pk.ws = pk.ws, pk.ws_plain
        old = pk.backward(route, "backward_packed")
        n = lib.edgedict_rnnt_grad_colsum_rows(code, B, T, U1, V)
        cs_old = torch.full((n, V), float("nan"), device="cuda")
        assert torch.equal(pk.backward(route, "backward_packed_colsum", cs_old), old)
        pk.ws = ar_ws
        assert torch.isfinite(old.float()).all()
        assert torch.equal(pk.backward(route, "backward_packed_ar", 0.0), old)
        assert torch.equal(pk.backward(route, "backward_packed_range_ar", 0, B, 0.0), old)
        cs_new = torch.full((n, V), float("nan"), device="cuda")
        assert torch.equal(pk.backward(route, "backward_packed_colsum_ar", cs_new, 0.0), old)
        assert torch.isfinite(cs_old).all() and torch.equal(cs_old, cs_new)


# ---------------------------------------------------------------------------------------------------------- aligner
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_aligner_respects_the_windows(hip_lib, dtype):
    from edgedict_amd.loss import rnnt_align
    B, T, U1, V = 6, 6, 4, 9
    rng = np.random.default_rng(11)
    acts = (2.0 * rng.normal(size=(B, T, U1, V))).astype(np.float32)
    labels = rng.integers(1, V, size=(B, U1 - 1)).astype(np.int32)
    al = np.array([6, 5, 6, 3, 1, 4], np.int32)
    ll = np.array([3, 2, 0, 3, 2, 1], np.int32)
    ta = torch.tensor(acts, device="cuda").to(dtype)
    seen = ta.double().cpu().numpy()
    args = (ta, _dev(labels), _dev(al), _dev(ll))
    given = AR.random_alignment(rng, al, ll, U1 - 1)
    plain_f, plain_s = rnnt_align(*args)
    for left, right in [(0, 0), (1, 1), (2, 0)]:
        lo, hi = AR.windows_from_frames(given, al, ll, left, right, Tm=T)
        if (left, right) == (1, 1):
            lo[0], hi[0] = _infeasible(lo[0], hi[0], T, 3, "order")
        f, s = rnnt_align(*args, windows=(_dev(lo), _dev(hi)))
        f, s = f.cpu().numpy(), s.cpu().numpy()
        for b in range(B):
            Tb, Ub = int(al[b]), int(ll[b])
            lpb, lpl = FR.cell_logprobs(seen[b], labels[b], Tb, Ub)
            _, best, arg, n = AR.ar_enumerate(lpb, lpl, lo[b, :Ub], hi[b, :Ub])
            assert (f[b, Ub:] == -1).all()
            if n == 0:
                assert s[b] == -np.inf and (f[b] == -1).all() and b == 0
                continue
            assert AR.respects(f[b, :Ub], lo[b], hi[b])
            np.testing.assert_allclose(s[b], best, rtol=1e-5 if dtype == F32 else 1e-4, atol=1e-4)
            np.testing.assert_allclose(FR.path_score(lpb, lpl, f[b, :Ub]), best, rtol=1e-4, atol=1e-4)
            if (left, right) == (0, 0):
                assert f[b, :Ub].tolist() == given[b, :Ub].tolist()
    cover = (_dev(np.zeros((B, U1 - 1))), _dev(np.full((B, U1 - 1), T - 1)))
    f, s = rnnt_align(*args, windows=cover)
    assert torch.equal(f, plain_f) and torch.equal(s, plain_s)


# ------------------------------------------------------------------------------------------------- model and engine
def _record_calls(monkeypatch):
    from edgedict_amd import _lib
    names = []
    real = _lib.call

    def call(name, *args):
        names.append(name)
        return real(name, *args)

    monkeypatch.setattr(_lib, "call", call)
    return names


def test_model_packed_and_dense_paths_agree_under_windows(hip_lib, monkeypatch):
    from edgedict_amd import config, ops
    from edgedict_amd.loss import alignment_windows
    cfg, sd, (xs, ys, xlen, ylen) = TF._tiny()
    lam = 0.5
    packed = TF._engine(cfg, sd, True, lam)
    names = _record_calls(monkeypatch)
    ops.LAST.pop("joint_band_rows", None)
    l0 = packed(xs.cuda(), ys.cuda(), xlen, ylen)                    # windows=None: the parent's entry points only
    assert not [n for n in names if n.endswith("_ar") or n in ("rnnt_band", "rnnt_alignment_windows")]
    assert "rnnt_loss_forward_packed" in names or "rnnt_loss_forward_packed_parts" in names
    assert "joint_band_rows" not in ops.LAST
    packed.eval()
    frames, scores = packed.align(xs.cuda(), ys.cuda(), xlen, ylen)
    assert not [n for n in names if n.endswith("_ar")]
    packed.train()
    with torch.no_grad():
        act = packed.scale_length(packed.encoder(xs[:, :xlen.max()].cuda())[0], xlen)
    U = int(ylen.max())
    windows = alignment_windows(frames, act.to(torch.int32).cuda(), ylen.to(torch.int32).cuda(), 1, 1)
    packed.zero_grad()
    del names[:]
    lp = packed(xs.cuda(), ys.cuda(), xlen, ylen, windows=windows)   # host lengths: _JointLossFn
    lp.backward()
    assert [n for n in names if n.endswith("_ar")] and "rnnt_band" in names
    rows, band_rows = ops.LAST["joint_rows"], ops.LAST["joint_band_rows"]
    assert torch.is_tensor(band_rows) and band_rows.is_cuda and 0 < int(band_rows) < rows
    dense = TF._engine(cfg, sd, True, lam)
    saved = config.PACKED_LATTICE
    config.PACKED_LATTICE = False
    try:
        ld = dense(xs.cuda(), ys.cuda(), xlen, ylen, windows=windows)    # same call, dense logits + _RNNTLossFn
        ld.backward()
        dense.eval()
        f_d, s_d = dense.align(xs.cuda(), ys.cuda(), xlen, ylen, windows=windows)
    finally:
        config.PACKED_LATTICE = saved
    assert lp.item() == ld.item() and torch.isfinite(lp).all()
    assert lp.item() > l0.item()                                     # fewer alignments: a strictly larger cost
    # test_packed_lattice_path_matches_golden_loss_and_dense_gradients' bound
    for (n, a), (_, b) in zip(packed.named_parameters(), dense.named_parameters()):
        scale = max(b.grad.abs().max().item(), 1e-8)
        assert (a.grad - b.grad).abs().max().item() <= 2e-5 * scale, n
    # the loss is the oracle's on the model's own logits
    logit_model = TF._engine(cfg, sd, False, 0.0)
    with torch.no_grad():
        logits = logit_model(xs.cuda(), ys.cuda(), xlen.cuda(), ylen.cuda())
    lo, hi = windows[0].cpu().numpy(), windows[1].cpu().numpy()
    costs, grads, _ = AR.ar_loss(logits.double().cpu().numpy(), ys[:, :U].numpy(), act.numpy(), ylen.numpy(), lo, hi, lam)
    np.testing.assert_allclose(lp.item(), costs.mean(), rtol=1e-5, atol=1e-4)
    B = xs.shape[0]
    ref = torch.tensor(grads.reshape(-1, grads.shape[-1]).sum(0) / B)
    for m in (packed, dense):
        got = m.joint.joint[2].bias.grad.double().cpu()
        assert (got - ref).abs().max().item() <= 2e-5 * ref.abs().max().item()   # test_joint_loss_fn_fp32's bound
    # align under the windows: both paths, frames inside the windows
    packed.eval()
    f_p, s_p = packed.align(xs.cuda(), ys.cuda(), xlen, ylen, windows=windows)
    assert torch.equal(f_p, f_d) and torch.allclose(s_p, s_d, rtol=1e-5, atol=1e-4)
    for b in range(B):
        assert AR.respects(f_p[b, :int(ylen[b])].cpu().numpy(), lo[b], hi[b])
    assert (s_p <= scores + 1e-4).all()


def test_train_engine_passes_the_windows_on(hip_lib):
    """train_step(..., windows=) with and without sub_batch_size returns the model's restricted loss."""
    from edgedict_amd.trainer import TrainEngine
    g = torch.Generator(device="cpu").manual_seed(5)
    wave = (0.1 * torch.randn(4, 9600, generator=g)).cuda()
    ys = torch.randint(4, 40, (4, 6), generator=g, dtype=torch.int32).cuda()
    ylen = torch.tensor([6, 4, 5, 6], dtype=torch.int32)
    lo = (torch.arange(6, dtype=torch.int32) // 2).repeat(4, 1).contiguous().cuda()
    hi = (lo + 4).contiguous()
    out = {}
    for sub in (None, 2):
        for windows in (None, (lo, hi)):
            torch.manual_seed(0)
            fl = TF._flags()
            fl.sub_batch_size = sub
            eng = TrainEngine(fl, vocab_size=40, device="cuda", compute_dtype="fp32")
            try:
                # the model's own loss on the engine's features, sub-batch by sub-batch as train_step cuts them
                eng.model.train()
                want = 0.0
                starts = list(range(0, 4, sub or 4))
                with torch.no_grad():
                    for s in starts:
                        e = s + (sub or 4)
                        xs, xlen = eng._front_end(wave[s:e], None)
                        kw = {} if windows is None else {"windows": (lo[s:e], hi[s:e])}
                        want = want + eng.model(xs, ys[s:e], xlen, ylen[s:e], **kw) / len(starts)
                loss = eng.train_step(wave, None, ys, ylen) if windows is None else eng.train_step(wave, None, ys, ylen, windows=windows)
                torch.cuda.synchronize()
                out[(sub, windows is not None)] = loss.detach().clone()
                assert torch.allclose(loss, want, rtol=1e-5, atol=1e-4), (sub, loss, want)
                for p in eng.model.parameters():
                    assert torch.isfinite(p.grad).all()
            finally:
                eng.close()
    for sub in (None, 2):                                            # fewer alignments: a strictly larger cost
        assert torch.isfinite(out[(sub, True)]).all() and out[(sub, True)].item() > out[(sub, False)].item()
