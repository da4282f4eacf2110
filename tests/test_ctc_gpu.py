"""GPU: the CTC auxiliary head - loss kernels, greedy decoder, the model's joint loss, the training engine - against the
float64 restatement tests/ctc_ref.py (pinned on the CPU by test_ctc_host.py).

Bounds: those the project holds the RNN-T loss to (tests/test_fastemit_gpu.py) - fp32 cost rtol 1e-5 / atol 1e-4 and
gradient 1e-3 |g| + 2e-5, bf16 cost rtol 1e-4 and gradient 4e-3 - the same arithmetic (fp32 log-sum-exp, fp64 lattice
carry with an fp32 correction term, exp(alpha + beta - ll) in fp32).  Every test prints its maximum error."""
import functools
import types

import numpy as np
import pytest
import torch

import ctc_ref as CR

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])

# (B, U, V): the state counts 2U+1 = 63 / 65 / 127 / 129 / 257 / 515 around the lane and states-per-lane boundaries,
# a V that takes the scalar path (29), the workload's V (4096)
SHAPES = [(1, 0, 8), (1, 1, 8), (3, 4, 29), (2, 31, 32), (2, 32, 32), (2, 63, 40), (2, 64, 40), (2, 128, 520),
          (4, 9, 4096), (2, 257, 16)]
SHAPE_IDS = ["%dx%dx%d" % s for s in SHAPES]


@functools.lru_cache(maxsize=None)
def _case(B, U, V):
    """Logits, labels from a 3-symbol alphabet (adjacent repeats everywhere) with V - 1 forced in, ragged lengths:
    row 1 has half the labels and T - 3 frames, row 2 (B >= 3) no labels and one frame.  T = max(U_b + repeats_b) + 5:
    random T at this alphabet is infeasible."""
    rng = np.random.default_rng(1000 * B + 10 * U + V)
    labels = rng.integers(1, 4, size=(B, U)).astype(np.int32)
    if U:
        labels[0, U // 2] = V - 1
    lab = np.full(B, U, dtype=np.int32)
    if B >= 2:
        lab[1] = U // 2
    if B >= 3:
        lab[2] = 0
    need = [int(lab[b]) + CR.repeats(list(labels[b, :lab[b]])) for b in range(B)]
    T = max(need) + 5
    act = np.full(B, T, dtype=np.int32)
    if B >= 2:
        act[1] = T - 3
    if B >= 3:
        act[2] = 1
    if B >= 4:
        act[3] = T - 1
    assert all(act[b] >= max(1, need[b]) for b in range(B))
    z = (2.0 * rng.normal(size=(B, T, V))).astype(np.float32)
    return z, labels, act, lab, need


@functools.lru_cache(maxsize=None)
def _oracle(B, U, V, dtype):
    z, labels, act, lab, _ = _case(B, U, V)
    seen = torch.tensor(z).to(dtype).double().numpy()                 # bf16: the oracle sees the rounded logits
    return CR.ctc_batch(seen, labels, act, lab)


def _dev(*arrays):
    return [torch.tensor(a, device="cuda") for a in arrays]


def _run(z, labels, act, lab, dtype, reduction="none", grad_out=None, zero_infinity=False, check_lengths=True):
    from edgedict_amd.loss import CTCLoss
    tz = torch.tensor(z, device="cuda").to(dtype).requires_grad_(True)
    tl, ta, tb = _dev(labels, act, lab)
    loss = CTCLoss(blank=0, reduction=reduction, zero_infinity=zero_infinity, check_lengths=check_lengths)(tz, tl, ta, tb)
    if grad_out is not None:
        loss.backward(grad_out)
    else:
        (loss.sum() if reduction == "none" else loss).backward()
    return loss.detach().clone(), tz.grad


def _assert_grad(err, ref, dtype, what):
    if dtype == F32:
        assert (err <= 1e-3 * np.abs(ref) + 2e-5).all(), (what, err.max())
    else:
        assert (err <= 4e-3).all(), (what, err.max())


@pytest.mark.parametrize("B,U,V", SHAPES, ids=SHAPE_IDS)
@DTYPES
def test_costs_gradient_zeros_determinism_and_liveness(hip_lib, B, U, V, dtype):
    """Checks 1, 3, 5, 6: costs and gradient against the oracle; exact zeros behind T_b and no effect of padding labels;
    two runs bit-identical; isfinite(alpha) & isfinite(beta) = the oracle's reachable states."""
    from edgedict_amd.loss import ctc_loss_debug
    z, labels, act, lab, _ = _case(B, U, V)
    costs, grads, _, lives = _oracle(B, U, V, dtype)
    assert np.isfinite(costs).all()
    cost, g = _run(z, labels, act, lab, dtype)
    err = np.abs(g.double().cpu().numpy() - grads)
    cerr = np.abs(cost.double().cpu().numpy() - costs)
    print("ctc", (B, U, V), dtype, "T %d: max cost err %.3g (rel %.3g), max grad err %.3g"
          % (z.shape[1], cerr.max(), (cerr / costs).max(), err.max()))
    if dtype == F32:
        np.testing.assert_allclose(cost.cpu().numpy(), costs, rtol=1e-5, atol=1e-4)
    else:
        np.testing.assert_allclose(cost.cpu().numpy(), costs, rtol=1e-4)
    _assert_grad(err, grads, dtype, "grad")
    assert g.dtype == dtype
    for b in range(B):
        if act[b] < z.shape[1]:
            assert g[b, int(act[b]):].abs().max().item() == 0
    # padding labels behind label_lens: no effect
    other = labels.copy()
    for b in range(B):
        other[b, lab[b]:] = V - 2
    cost_p, g_p = _run(z, other, act, lab, dtype)
    assert torch.equal(cost_p, cost) and torch.equal(g_p, g)
    # determinism
    cost2, g2 = _run(z, labels, act, lab, dtype)
    assert torch.equal(cost2, cost) and torch.equal(g2, g)
    # liveness
    tz = torch.tensor(z, device="cuda").to(dtype)
    dcost, lse, alphas, betas, ll = ctc_loss_debug(tz, *_dev(labels, act, lab))
    assert torch.equal(dcost, cost)
    np.testing.assert_allclose(ll[:, 1].cpu().numpy(), ll[:, 0].cpu().numpy(), rtol=1e-6, atol=1e-5)
    live = (torch.isfinite(alphas) & torch.isfinite(betas)).cpu().numpy()
    for b in range(B):
        Tb, Sb = int(act[b]), 2 * int(lab[b]) + 1
        assert (live[b, :Tb, :Sb] == lives[b]).all(), b


@pytest.mark.parametrize("B,U,V", [(3, 4, 29), (2, 63, 40), (4, 9, 4096)], ids=["3x4x29", "2x63x40", "4x9x4096"])
@DTYPES
def test_reductions_and_grad_output(hip_lib, B, U, V, dtype):
    """Check 2: 'none' / 'sum' / 'mean' values and gradient scales, a non-unit grad_output per utterance."""
    z, labels, act, lab, _ = _case(B, U, V)
    costs, grads, _, _ = _oracle(B, U, V, dtype)
    cost, g = _run(z, labels, act, lab, dtype)
    for reduction, scale in (("sum", 1.0), ("mean", 1.0 / B)):
        red, gr = _run(z, labels, act, lab, dtype, reduction=reduction)
        assert red.shape == (1,)
        np.testing.assert_allclose(red.item(), scale * costs.sum(), rtol=1e-5 if dtype == F32 else 1e-4, atol=1e-4)
        np.testing.assert_allclose(red.item(), scale * cost.double().sum().item(), rtol=1e-6)
        err = np.abs(gr.double().cpu().numpy() - scale * grads)
        _assert_grad(err, scale * grads, dtype, reduction)
        red3, gr3 = _run(z, labels, act, lab, dtype, reduction=reduction, grad_out=torch.tensor([3.0], device="cuda"))
        err = np.abs(gr3.double().cpu().numpy() - 3.0 * scale * grads)
        assert (err <= 3.0 * ((1e-3 * np.abs(scale * grads) + 2e-5) if dtype == F32 else 4e-3)).all(), err.max()
    w = np.linspace(0.5, 2.0, B)
    _, gw = _run(z, labels, act, lab, dtype, grad_out=torch.tensor(w, device="cuda", dtype=F32))
    ref = w[:, None, None] * grads
    err = np.abs(gw.double().cpu().numpy() - ref)
    print("ctc grad_output", (B, U, V), dtype, "max err %.3g" % err.max())
    assert (err <= w[:, None, None] * ((1e-3 * np.abs(grads) + 2e-5) if dtype == F32 else 4e-3)).all(), err.max()


@pytest.mark.parametrize("B,U,V", SHAPES, ids=SHAPE_IDS)
@DTYPES
def test_infeasible_row(hip_lib, B, U, V, dtype):
    """Check 4: row 0 gets T_b = U_b + repeats_b - 1 frames: cost +inf, gradient exact zeros, the other rows unchanged;
    zero_infinity: cost 0 and a finite mean."""
    z, labels, act, lab, need = _case(B, U, V)
    cost, g = _run(z, labels, act, lab, dtype)
    short = act.copy()
    short[0] = need[0] - 1
    cost_i, g_i = _run(z, labels, short, lab, dtype, check_lengths=False)
    assert cost_i[0].item() == float("inf")
    assert g_i[0].abs().max().item() == 0
    assert torch.equal(cost_i[1:], cost[1:]) and torch.equal(g_i[1:], g[1:])
    assert not torch.isnan(g_i).any()
    cost_z, g_z = _run(z, labels, short, lab, dtype, zero_infinity=True, check_lengths=False)
    assert cost_z[0].item() == 0 and torch.equal(cost_z[1:], cost[1:]) and torch.equal(g_z, g_i)
    mean_i, _ = _run(z, labels, short, lab, dtype, reduction="mean", check_lengths=False)
    mean_z, gm = _run(z, labels, short, lab, dtype, reduction="mean", zero_infinity=True, check_lengths=False)
    assert mean_i.item() == float("inf") and np.isfinite(mean_z.item())
    np.testing.assert_allclose(mean_z.item(), cost[1:].double().sum().item() / B, rtol=1e-6, atol=1e-30)
    assert gm[0].abs().max().item() == 0 and torch.isfinite(gm).all()


def _greedy_logits(B, T, V, dtype):
    """Logits with runs of a boosted symbol (blank, 1, 2, V - 1), quantised so that ties occur; utterance 0 all blank."""
    rng = np.random.default_rng(7 * B + T + V)
    z = np.round(2.0 * rng.normal(size=(B, T, V))) / 2.0
    for b in range(B):
        t = 0
        while t < T:
            run = int(rng.integers(1, 4))
            k = 0 if b == 0 else int(rng.choice([0, 1, 2, V - 1]))
            z[b, t:t + run, k] += 30.0 if b == 0 else 2.5
            t += run
    act = np.full(B, T, dtype=np.int32)
    if B >= 2:
        act[1] = 1                                   # a T_b = 1 utterance
    if B >= 3:
        act[2] = max(1, T - 3)
    return torch.tensor(z, device="cuda").to(dtype), act


@pytest.mark.parametrize("B,U,V", SHAPES, ids=SHAPE_IDS)
@DTYPES
def test_greedy(hip_lib, B, U, V, dtype):
    """Check 7: tokens, counts, frames exactly the numpy collapse of the arg max of the device logits read back (lowest
    index on ties), neglogp against fp64; an all-blank utterance and a T_b = 1 utterance are in."""
    from edgedict_amd.loss import ctc_greedy
    T = U + 7
    z, act = _greedy_logits(max(B, 3), T, V, dtype)
    Bz = z.shape[0]
    tokens, counts, frames, neglogp = ctc_greedy(z, torch.tensor(act, device="cuda"))
    want = CR.greedy(z.double().cpu().numpy(), act)
    tokens, counts, frames = tokens.cpu().numpy(), counts.cpu().numpy(), frames.cpu().numpy()
    assert tokens.shape == frames.shape == (Bz, T) and tokens.dtype == np.int32
    for b in range(Bz):
        toks, frs, nl = want[b]
        n = toks.size
        assert counts[b] == n, b
        assert (tokens[b, :n] == toks).all() and (frames[b, :n] == frs).all(), b
        assert (tokens[b, n:] == -1).all() and (frames[b, n:] == -1).all(), b
    assert counts[0] == 0 and neglogp[0].item() == 0            # all blank
    ref = np.array([w[2] for w in want])
    got = neglogp.double().cpu().numpy()
    print("ctc greedy", (Bz, T, V), dtype, "kept", counts.tolist(), "max rel err %.3g"
          % (np.abs(got - ref) / np.maximum(ref, 1e-30)).max())
    np.testing.assert_allclose(got, ref, rtol=1e-5 if dtype == F32 else 1e-3)
    if T > 8:
        assert counts.max() > 1


# --------------------------------------------------------------------------------------------------- model level
def _tiny(name):
    from oracle import models_ref as M
    from oracle.make_golden import CASES
    cfg, B, T0, U, seed = CASES[name]
    return cfg, M.make_state_dict(cfg, seed), M.make_batch(cfg, seed + 1, B, T0, U)


def _model(cfg, sd, cd, w, output_loss=True):
    from edgedict_amd.models import Transducer
    torch.manual_seed(11)
    m = Transducer(enc_dropout=0.0, dec_dropout=0.0, output_loss=output_loss, ctc_weight=w, **cfg)
    missing = m.load_state_dict(sd, strict=False)
    assert sorted(missing.missing_keys) == (["ctc_head.bias", "ctc_head.weight"] if w > 0 else [])
    assert not missing.unexpected_keys
    m = m.cuda()
    m.compute_dtype = cd
    return m


def _lens(t, device_lengths):
    return t.cuda() if device_lengths else t


@pytest.mark.parametrize("device_lengths", [False, True], ids=["host_lens", "device_lens"])
@pytest.mark.parametrize("cd", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["tiny", "gru_tiny"])
def test_model_loss_parts_head_gradients_decode_and_windows(hip_lib, name, cd, device_lengths):
    """Check 8 (all but linearity): loss = parts[0] + w * parts[1]; parts[0] bit-identical to the model at weight 0;
    parts[1] and the head's gradients against the oracle fed the read-back h_enc and head parameters; ctc_greedy_decode =
    ctc_greedy on the model's own head logits; windows= with the head."""
    from edgedict_amd.loss import ctc_greedy
    cfg, sd, (xs, ys, xlen, ylen) = _tiny(name)
    w = 0.3
    dtype = F32 if cd == "fp32" else BF16
    m = _model(cfg, sd, cd, w)
    xl, yl = _lens(xlen, device_lengths), _lens(ylen, device_lengths)
    loss = m(xs.cuda(), ys.cuda(), xl, yl)
    loss.backward()
    rnnt, ctc = m.loss_parts
    assert loss.shape == (1,) and rnnt.shape == (1,) and ctc.shape == (1,)
    assert not rnnt.requires_grad and not ctc.requires_grad
    np.testing.assert_allclose(loss.item(), rnnt.item() + w * ctc.item(), rtol=1e-6)
    gW, gb = m.ctc_head.weight.grad.double().cpu().numpy(), m.ctc_head.bias.grad.double().cpu().numpy()
    # weight 0 on the same model: the launches of a model without the head
    m.ctc_weight = 0.0
    m.loss_parts = None
    m.zero_grad()
    plain = m(xs.cuda(), ys.cuda(), xl, yl)
    assert torch.equal(plain, rnnt) and m.loss_parts is None
    assert torch.equal(plain, _model(cfg, sd, cd, 0.0)(xs.cuda(), ys.cuda(), xl, yl))
    m.ctc_weight = w
    # the oracle on the read-back encoder output and head parameters (rounded as the product reads / writes them)
    with torch.no_grad():
        h_enc, _ = m.encoder(xs[:, :int(xlen.max())].contiguous().cuda())
        act = m.scale_length(h_enc, xlen).numpy()
        head_logits = m._ctc_logits(h_enc).contiguous()
    H = h_enc.to(dtype).double().cpu().numpy()
    W = m.ctc_head.weight.detach().to(dtype).double().cpu().numpy()
    bias = m.ctc_head.bias.detach().double().cpu().numpy()
    logits = H @ W.T + bias
    seen = torch.tensor(logits).to(dtype).double().numpy()
    B, T, V = seen.shape
    U = int(ylen.max())
    labels = ys[:, :U].numpy()
    costs, grads, _, _ = CR.ctc_batch(seen, labels, act, ylen.numpy())
    finite = np.isfinite(costs)
    want = np.where(finite, costs, 0.0).sum() / B                       # zero_infinity, 'mean' = sum / B
    print("ctc model", name, cd, "device_lens" if device_lengths else "host_lens", "ctc %.6g, oracle %.6g" % (ctc.item(), want))
    np.testing.assert_allclose(ctc.item(), want, rtol=1e-5 if cd == "fp32" else 1e-4, atol=1e-4 if cd == "fp32" else 0)
    # dW = G^T H, db = colsum G with G = w x the 'mean' gradient, what ctc_grad writes: every element of G within the loss kernels' bound, so
    # |dW err| <= E_rel |G|^T |H| + E_abs 1^T |H| (fp32: 1e-3, 2e-5; bf16: 0, 4e-3), |db err| likewise with H = 1
    G = (w * grads / B).reshape(B * T, V)
    H2 = H.reshape(B * T, -1)
    rows = (np.arange(T)[None, :] < act[:, None]).reshape(-1)            # frames behind T_b carry exact zeros
    e_rel, e_abs = (1e-3, 2e-5) if cd == "fp32" else (0.0, 4e-3)
    bound_W = e_rel * np.abs(G).T @ np.abs(H2) + e_abs * np.abs(H2[rows]).sum(0)[None, :]
    bound_b = e_rel * np.abs(G).sum(0) + e_abs * rows.sum()
    errW, errb = np.abs(gW - G.T @ H2), np.abs(gb - G.sum(0))
    print("ctc model head grads: max dW err %.3g (bound %.3g), max db err %.3g (bound %.3g)"
          % (errW.max(), bound_W.min(), errb.max(), bound_b.min()))
    assert np.abs(G.T @ H2).max() > 1e-3
    assert (errW <= bound_W).all() and (errb <= bound_b).all()
    # ctc_greedy_decode = ctc_greedy on the model's own head logits
    m.eval()
    hyps, nl = m.ctc_greedy_decode(xs.cuda(), xl)
    tokens, counts, _, nl2 = ctc_greedy(head_logits, torch.tensor(act, dtype=torch.int32, device="cuda"), m.blank)
    assert len(hyps) == B and torch.equal(nl, nl2)
    for b in range(B):
        assert hyps[b].dtype == np.int64
        assert (hyps[b] == tokens[b, :int(counts[b])].cpu().numpy()).all()
    m.train()
    # windows= with the head: runs, and is the sum of its parts
    lo = torch.zeros(B, U, dtype=torch.int32, device="cuda")
    hi = torch.full((B, U), T - 1, dtype=torch.int32, device="cuda")
    lw = m(xs.cuda(), ys.cuda(), xl, yl, windows=(lo, hi))
    r2, c2 = m.loss_parts
    np.testing.assert_allclose(lw.item(), r2.item() + w * c2.item(), rtol=1e-6)
    assert torch.equal(c2, ctc)
    lw.backward()
    # output_loss=False returns the joint logits as before
    assert _model(cfg, sd, cd, w, output_loss=False)(xs.cuda(), ys.cuda(), xl, yl).dim() == 4


@pytest.mark.parametrize("device_lengths", [False, True], ids=["host_lens", "device_lens"])
@pytest.mark.parametrize("name", ["tiny", "gru_tiny"])
def test_model_encoder_gradient_is_linear_in_ctc_weight(hip_lib, name, device_lengths):
    """Check 8, linearity (fp32, dropout 0): for every encoder parameter g(0.6) - g(0) = 2 (g(0.3) - g(0)) within the fp32
    gradient bound, and g(0.3) - g(0) is not zero."""
    cfg, sd, (xs, ys, xlen, ylen) = _tiny(name)
    m = _model(cfg, sd, "fp32", 0.3)
    xl, yl = _lens(xlen, device_lengths), _lens(ylen, device_lengths)
    g = {}
    for w in (0.0, 0.3, 0.6):
        m.ctc_weight = w
        m.zero_grad()
        m(xs.cuda(), ys.cuda(), xl, yl).backward()
        g[w] = {n: p.grad.detach().clone() for n, p in m.encoder.named_parameters()}
    assert g[0.0]
    worst = 0.0
    for n in g[0.0]:
        small = g[0.3][n] - g[0.0][n]
        big = g[0.6][n] - g[0.0][n]
        assert small.abs().max().item() > 0, n
        err = (big - 2.0 * small).abs()
        worst = max(worst, err.max().item())
        assert (err <= 1e-3 * big.abs() + 2e-5).all(), (n, err.max().item())
    print("ctc linearity", name, "max err %.3g" % worst)


# --------------------------------------------------------------------------------------------------- training engine
def _flags(ctc_weight=None):
    # test_fastemit_gpu._flags()
    fl = types.SimpleNamespace(
        downsample=3, win_length=320, hop_length=160, n_fft=512, feature_size=80, dither=0.0,
        sample_rate=16000, lr=2e-3, gradclip=None, sub_batch_size=None, bpe_size=40,
        vocab_embed_size=8, enc_hidden_size=32, enc_layers=3, enc_dropout=0.0, enc_proj_size=24,
        dec_hidden_size=16, dec_layers=2, dec_dropout=0.0, dec_proj_size=16, joint_size=32,
        enc_time_reductions=[1], delta=False, T_mask=0, T_num_mask=0, F_mask=0, F_num_mask=0)
    if ctc_weight is not None:
        fl.ctc_weight = ctc_weight
    return fl


def test_train_engine_carries_the_head(hip_lib, tmp_path):
    """Check 9: the head's tensors are in the flat buffer and a bucket, one step changes them, save / load round-trips
    them; flags without ctc_weight give today's state-dict keys."""
    from edgedict_amd.trainer import TrainEngine
    g = torch.Generator(device="cpu").manual_seed(5)
    wave = (0.1 * torch.randn(4, 9600, generator=g)).cuda()
    ys = torch.randint(4, 40, (4, 6), generator=g, dtype=torch.int32).cuda()
    ylen = torch.tensor([6, 4, 5, 6], dtype=torch.int32)
    torch.manual_seed(0)
    plain = TrainEngine(_flags(), vocab_size=40, device="cuda", compute_dtype="fp32")
    try:
        keys = list(plain.model.state_dict().keys())
        assert not hasattr(plain.model, "ctc_head") and plain.model.ctc_weight == 0.0
        assert not any("ctc" in k for k in keys)
    finally:
        plain.close()
    torch.manual_seed(0)
    eng = TrainEngine(_flags(0.3), vocab_size=40, device="cuda", compute_dtype="fp32")
    try:
        head = eng.model.ctc_head
        assert eng.model.ctc_weight == 0.3
        assert list(eng.model.state_dict().keys()) == keys + ["ctc_head.weight", "ctc_head.bias"]
        for p in (head.weight, head.bias):
            assert any(p is q for q in eng.flat.params)
            assert id(p) in eng.reducer.param_bucket
        assert eng.flat.params[-1] is head.bias and eng.flat.params[-2] is head.weight
        assert eng.reducer.param_bucket[id(head.weight)] == 0          # the end of the flat buffer: issued first
        before = [head.weight.detach().clone(), head.bias.detach().clone()]
        loss = eng.train_step(wave, None, ys, ylen)
        torch.cuda.synchronize()
        assert loss.shape == (1,) and torch.isfinite(loss).all()
        rnnt, ctc = eng.model.loss_parts
        np.testing.assert_allclose(loss.item(), rnnt.item() + 0.3 * ctc.item(), rtol=1e-6)
        assert not torch.equal(head.weight, before[0]) and not torch.equal(head.bias, before[1])
        path = str(tmp_path / "ctc.pt")
        eng.save(path)
        after = [head.weight.detach().clone(), head.bias.detach().clone()]
        with torch.no_grad():
            head.weight.zero_()
            head.bias.zero_()
        eng.load(path)
        assert torch.equal(head.weight, after[0]) and torch.equal(head.bias, after[1])
    finally:
        eng.close()
    with pytest.raises(ValueError, match="ctc_weight"):
        TrainEngine(_flags(-1.0), vocab_size=40, device="cuda", compute_dtype="fp32")
