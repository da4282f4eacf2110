"""GPU: the forced aligner (edgedict_rnnt_align*, loss.rnnt_align, Transducer.align) - the Viterbi walk over the
lattice of the loss and its back-trace - against the float64 restatement tests/fastemit_ref.py (pinned against the
enumeration of every alignment by tests/test_fastemit_host.py).

Near-ties may legitimately resolve differently in the kernel (fp32 log-probabilities) and in float64, so on random
logits the GPU's path is RE-SCORED in float64 and must be as good as the best one within the cost tolerance of the
loss tests; on the planted case, where the best path wins by a wide margin, the frames must be exactly the planted
ones."""
import numpy as np
import pytest
import torch

import fastemit_ref as FR
import rnnt_walk_cases as WC
from oracle import packed_ref as PR

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
ROUTES = [("dense", F32), ("dense", BF16), ("packed", F32), ("packed", BF16), ("parts", BF16)]
# The Viterbi walk rnnt_alpha_beta<C, true> at C = 4, 8, 16 label columns per lane (U1 = 129, 257, 513 and the limit,
# 1024; U1 = 70 above is C = 2): the batches of tests/rnnt_walk_cases.py, whose lengths sit on the edges of each walk's
# prefetch ring and of its last live lane
WALK_SHAPES = [(WC.B_WALK, WC.T_WALK, U1, 8) for U1 in (129, 257, 513, 1024)]
# (B, T, U1, V): row 0 is the full box (U_b = U_max), row 1 one frame, row 2 no labels, the others random
SHAPES = [(5, 12, 6, 32), (4, 33, 70, 64), (6, 40, 9, 264), (3, 1, 4, 16)] + WALK_SHAPES


def _lens(seed, B, T, U1):
    if (B, T, U1, 8) in WALK_SHAPES:
        return WC.length_rows(T, U1, rotate=3 if U1 in (257, 1024) else 0)
    rng = np.random.default_rng(seed)
    al = rng.integers(1, T + 1, size=B).astype(np.int32)
    ll = rng.integers(0, U1, size=B).astype(np.int32)
    al[0], ll[0] = T, U1 - 1
    al[1] = 1
    ll[2] = 0
    return al, ll


def _lse_parts(logits):
    """What the logits product's epilogue leaves per 64-column slot: (max, sum exp(x - max)) in fp32 - here taken from the
    stored logits themselves."""
    M, V = logits.shape
    slots = (V + 63) // 64
    x = torch.full((M, slots * 64), float("-inf"), device=logits.device)
    x[:, :V] = logits.float()
    x = x.view(M, slots, 64)
    mx = x.max(-1).values
    return torch.stack([mx, torch.exp(x - mx[..., None]).sum(-1)], -1).contiguous(), slots


def _align(route, acts, labels, al, ll, blank=0):
    """(frames [B, U1-1], scores [B]) of dense logits `acts` [B, T, U1, V] (already in the route's dtype) by `route`."""
    from edgedict_amd import _lib
    from edgedict_amd.loss import rnnt_align
    B, T, U1, V = acts.shape
    lab_d, al_d, ll_d = (torch.tensor(x).cuda() for x in (labels, al, ll))
    if route == "dense":
        return rnnt_align(acts, lab_d, al_d, ll_d, blank)
    off, M = PR.offsets(al, ll)
    packed = PR.pack(acts.cpu(), al, ll).cuda().contiguous()
    ws = torch.full((_lib.load().edgedict_rnnt_workspace_bytes(B, T, U1),), 0xFF, dtype=torch.uint8, device="cuda")
    frames = torch.full((B, U1 - 1), -7, dtype=torch.int32, device="cuda")
    scores = torch.full((B,), float("nan"), device="cuda")
    if route == "packed":
        _lib.call("rnnt_align_packed", packed, _lib.dtype_code(acts.dtype), lab_d, al_d, ll_d, off.cuda(), B, T, U1, V,
                  blank, frames, scores, ws)
    else:
        parts, slots = _lse_parts(packed)
        _lib.call("rnnt_align_packed_parts", packed, lab_d, al_d, ll_d, off.cuda(), B, T, U1, V, blank, frames, scores,
                  ws, parts, slots)
    torch.cuda.synchronize()
    return frames, scores


def _costs(route, acts, labels, al, ll):
    """costs [B] of the loss on the log-probabilities the route's aligner saw (the parts route takes its denominators
    from the partials, in another summation order than the pass over the logits)."""
    from edgedict_amd import _lib
    from edgedict_amd.loss import RNNTLoss
    lab_d, al_d, ll_d = (torch.tensor(x).cuda() for x in (labels, al, ll))
    if route != "parts":
        with torch.no_grad():
            return RNNTLoss(reduction="none")(acts, lab_d, al_d, ll_d)
    B, T, U1, V = acts.shape
    off, M = PR.offsets(al, ll)
    packed = PR.pack(acts.cpu(), al, ll).cuda().contiguous()
    parts, slots = _lse_parts(packed)
    ws = torch.zeros(_lib.load().edgedict_rnnt_workspace_bytes(B, T, U1), dtype=torch.uint8, device="cuda")
    costs, red = torch.empty(B, device="cuda"), torch.empty(1, device="cuda")
    _lib.call("rnnt_loss_forward_packed_parts", packed, lab_d, al_d, ll_d, off.cuda(), B, T, U1, V, 0, costs, red, 1.0,
              ws, parts, slots)
    torch.cuda.synchronize()
    return costs


def _close(got, want, dtype):
    """the cost tolerances of tests/test_rnnt_loss_gpu.py: rtol 1e-5, atol 1e-4 (fp32); rtol 1e-4 (bf16)"""
    return abs(got - want) <= (1e-4 + 1e-5 * abs(want) if dtype == F32 else 1e-4 * abs(want))


@pytest.mark.parametrize("B,T,U1,V", SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("route,dtype", ROUTES, ids=[r + "-" + ("f32" if d == F32 else "bf16") for r, d in ROUTES])
def test_random_ragged_batches(hip_lib, route, dtype, B, T, U1, V):
    rng = np.random.default_rng(B * 1000 + T)
    al, ll = _lens(B + T + U1, B, T, U1)
    labels = rng.integers(1, V, size=(B, U1 - 1)).astype(np.int32)
    acts = torch.tensor(2.0 * rng.normal(size=(B, T, U1, V)), dtype=torch.float32).to(dtype).cuda()
    seen = acts.double().cpu().numpy()                        # bf16: rounded first, then upcast
    frames, scores = _align(route, acts, labels, al, ll)
    costs = _costs(route, acts, labels, al, ll)
    assert (scores <= -costs).all(), (scores, costs)          # one path against the sum over all of them
    frames, scores, costs = frames.cpu().numpy(), scores.cpu().numpy(), costs.cpu().numpy()
    assert frames.shape == (B, U1 - 1) and frames.dtype == np.int32
    for b in range(B):
        Tb, Ub = int(al[b]), int(ll[b])
        lpb, lpl = FR.cell_logprobs(seen[b], labels[b], Tb, Ub)
        best, _ = FR.viterbi_one(lpb, lpl)
        fr = frames[b]
        assert (fr[Ub:] == -1).all(), (b, fr)
        assert (fr[:Ub] >= 0).all() and (fr[:Ub] < Tb).all() and (np.diff(fr[:Ub]) >= 0).all(), (b, fr)
        rescored = FR.path_score(lpb, lpl, fr[:Ub])
        print("align", route, dtype, (B, T, U1, V), b, "score %.6f best %.6f rescored %.6f" % (scores[b], best, rescored))
        assert _close(float(scores[b]), best, dtype), (b, scores[b], best)
        assert _close(rescored, best, dtype), (b, rescored, best)
        if Ub == 0:
            # one alignment only: the score IS the log-likelihood (same fp64 sum of the same fp32 terms, one rounding)
            assert abs(float(scores[b]) + float(costs[b])) <= 2.0 ** -22 * abs(float(costs[b])), (scores[b], costs[b])


@pytest.mark.parametrize("route,dtype", ROUTES, ids=[r + "-" + ("f32" if d == F32 else "bf16") for r, d in ROUTES])
def test_planted_alignment_is_recovered_exactly(hip_lib, route, dtype):
    """+10 on the transitions of a chosen alignment over noise of scale 1: leaving it costs a step of log-probability
    ~ -10 against ~ -0.003 per step on it, so it is the best path by a margin no rounding bridges."""
    _planted(route, dtype, 6, 40, 9, 264)


@pytest.mark.parametrize("route,dtype", ROUTES, ids=[r + "-" + ("f32" if d == F32 else "bf16") for r, d in ROUTES])
def test_planted_alignment_is_recovered_exactly_on_the_long_axis(hip_lib, route, dtype):
    """The same at U1 = 513: 16 label columns per lane, a prefetch ring of one step, a back-trace of up to 528 steps."""
    _planted(route, dtype, WC.B_WALK, WC.T_WALK, 513, 8)


def _planted(route, dtype, B, T, U1, V):
    rng = np.random.default_rng(42)
    al, ll = _lens(9, B, T, U1)
    labels = rng.integers(1, V, size=(B, U1 - 1)).astype(np.int32)
    acts = rng.normal(size=(B, T, U1, V)).astype(np.float32)
    planted = np.full((B, U1 - 1), -1, dtype=np.int32)
    for b in range(B):
        Tb, Ub = int(al[b]), int(ll[b])
        fr = np.sort(rng.integers(0, Tb, size=Ub))
        planted[b, :Ub] = fr
        t = 0
        for u in range(Ub):
            while t < fr[u]:
                acts[b, t, u, 0] += 10.0
                t += 1
            acts[b, t, u, labels[b, u]] += 10.0
        while t < Tb:
            acts[b, t, Ub, 0] += 10.0
            t += 1
    frames, scores = _align(route, torch.tensor(acts).to(dtype).cuda(), labels, al, ll)
    assert np.array_equal(frames.cpu().numpy(), planted), (frames.cpu().numpy(), planted)
    assert torch.isfinite(scores).all() and (scores > -5.0).all()


def test_ties_take_the_blank_predecessor_and_empty_utterances_get_minus_infinity(hip_lib):
    """Constant logits: every alignment scores the same and the documented rule emits every label on frame 0.  A raw
    C-ABI caller's empty utterance (T_b <= 0; the Python shim's callers never have one): score -inf, frames -1."""
    from edgedict_amd import _lib
    B, T, U1, V = 3, 5, 4, 8
    acts = torch.zeros(B, T, U1, V, device="cuda")
    labels = torch.ones(B, U1 - 1, dtype=torch.int32, device="cuda")
    al = torch.tensor([5, 0, 3], dtype=torch.int32).cuda()
    ll = torch.tensor([3, 2, 1], dtype=torch.int32).cuda()
    ws = torch.zeros(_lib.load().edgedict_rnnt_workspace_bytes(B, T, U1), dtype=torch.uint8, device="cuda")
    frames = torch.full((B, U1 - 1), -7, dtype=torch.int32, device="cuda")
    scores = torch.full((B,), float("nan"), device="cuda")
    _lib.call("rnnt_align", acts, 0, labels, al, ll, B, T, U1, V, 0, frames, scores, ws)
    torch.cuda.synchronize()
    assert frames.cpu().tolist() == [[0, 0, 0], [-1, -1, -1], [0, -1, -1]]
    want = torch.tensor([-8 * np.log(8.0), -np.inf, -4 * np.log(8.0)])
    assert scores[1].item() == -np.inf
    assert torch.allclose(scores.cpu()[[0, 2]], want[[0, 2]].float(), rtol=1e-6)


def test_transducer_align_equals_rnnt_align_on_the_models_dense_logits(hip_lib):
    from edgedict_amd.loss import rnnt_align
    from edgedict_amd.models import Transducer
    from oracle import models_ref as M
    from oracle.make_golden import CASES
    cfg, B, T0, U, seed = CASES["tiny"]
    sd = M.make_state_dict(cfg, seed)
    xs, ys, xlen, ylen = M.make_batch(cfg, seed + 1, B, T0, U)
    m = Transducer(enc_dropout=0.0, dec_dropout=0.0, output_loss=False, **cfg)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    m.compute_dtype = "fp32"
    tokens0, score0 = m.greedy_decode(xs.cuda(), xlen.cuda())
    with torch.no_grad():
        logits = m(xs.cuda(), ys.cuda(), xlen.cuda(), ylen.cuda())
        act = m.scale_length(logits, xlen)
    Um = int(ylen.max())
    want_f, want_s = rnnt_align(logits.contiguous(), ys[:, :Um].to(torch.int32).cuda().contiguous(), act.int().cuda(),
                                ylen.int().cuda())
    for lens in ((xlen, ylen), (xlen.cuda(), ylen.cuda())):           # host lengths: packed lattice; device: dense logits
        frames, scores = m.align(xs.cuda(), ys.cuda(), *lens)
        assert frames.dtype == torch.int32 and frames.shape == (B, Um) and scores.shape == (B,)
        assert torch.equal(frames, want_f)
        assert torch.allclose(scores, want_s, rtol=1e-5, atol=1e-4)
    for b in range(B):
        fr = frames[b, :int(ylen[b])]
        assert (fr >= 0).all() and (fr < int(act[b])).all() and (fr[1:] >= fr[:-1]).all()
        assert (frames[b, int(ylen[b]):] == -1).all()
    # align leaves no state behind: the greedy search is what it was
    tokens1, score1 = m.greedy_decode(xs.cuda(), xlen.cuda())
    assert all(np.array_equal(a, b) for a, b in zip(tokens0, tokens1)) and torch.equal(score0, score1)
