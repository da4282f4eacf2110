"""GPU: MWER training from the kernel up.  The risk kernel (csrc/mwer.hip) against the float64 oracle tests/mwer_ref.py
(pinned by tests/test_mwer_host.py) with its errors coming from metrics.edit_distance itself; the autograd wrappers; the
packed joint's per-row costs against the dense joint + RNNTLoss(reduction='none'); Transducer.mwer_loss against a form
composed of validated pieces (dense joint on repeated encoder rows, RNNTLoss('none'), tests/edit_distance_ref.py, a torch
float64 softmax-risk); the searched lists; TrainEngine.mwer_step.

Bounds.  The kernel's outputs are fp32 roundings of fp64 values: rtol 2**-22, plus atol 1e-12 * max(1, max errs) for the
cancellation in d - dbar (and for posteriors below fp32's normal range); exactly 0 where the definition says 0.  Packed
against dense: tests/test_fastemit_gpu.py::test_model_packed_and_dense_paths_agree...'s - equal costs, gradients within
2e-5 of the tensor's largest entry."""
import types

import numpy as np
import pytest
import torch

import edit_distance_ref as ER
import mwer_ref as MR

pytestmark = pytest.mark.gpu

F32 = torch.float32
RTOL = 2.0 ** -22
SHAPES = [(1, 1), (1, 32), (3, 5), (70, 32)]


def _close(got, want, max_err, what):
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    err = np.abs(got - want)
    tol = RTOL * np.abs(want) + 1e-12 * max(1.0, float(max_err))
    print("%s: max err %.3g (max |want| %.3g)" % (what, err.max() if err.size else 0.0, np.abs(want).max() if want.size else 0.0))
    assert (err <= tol).all(), (what, float(err.max()))
    assert (got[want == 0] == 0).all(), what                # exactly 0 where the definition says 0


def _native(costs, errs, n_hyp=None, ref=None, nll=0.0, scale=1.0, reduced=True):
    """One edgedict_mwer_risk call on device tensors: (risk, post, coef, reduced)."""
    import ctypes
    from edgedict_amd import _lib
    B, N = costs.shape
    dev = costs.device
    risk = torch.full((B,), float("nan"), dtype=F32, device=dev)
    post = torch.full((B, N), float("nan"), dtype=F32, device=dev)
    coef = torch.full((B, N), float("nan"), dtype=F32, device=dev)
    red = torch.full((1,), float("nan"), dtype=F32, device=dev) if reduced else None
    _lib.call("mwer_risk", costs, errs, 4 if errs.dim() == 3 else 1, n_hyp, ref, B, N, ctypes.c_double(nll),
              ctypes.c_double(scale), risk, post, coef, red)
    return risk, post, coef, red


def _errors(seed, B, N, n_hyp=None):
    """[B, N, 4] error counts from metrics.edit_distance on random short sequences (device tensor)."""
    from edgedict_amd import metrics
    rng = np.random.default_rng(seed)
    hyps = torch.tensor(rng.integers(0, 4, size=(B, N, 9)).astype(np.int32), device="cuda")
    hl = torch.tensor(rng.integers(0, 10, size=(B, N)).astype(np.int32), device="cuda")
    refs = torch.tensor(rng.integers(0, 4, size=(B, 7)).astype(np.int32), device="cuda")
    rl = torch.tensor(rng.integers(0, 8, size=B).astype(np.int32), device="cuda")
    return metrics.edit_distance(hyps, hl, refs, rl, n_hyp)


def _variants(seed, B, N):
    """(name, costs [B, N] float32 numpy, n_hyp or None, equal_errors)"""
    rng = np.random.default_rng(seed)
    base = rng.uniform(0.5, 12.0, size=(B, N)).astype(np.float32)
    ragged = rng.integers(0, N + 1, size=B).astype(np.int32)
    ragged[B // 2] = 0                                       # an utterance without a live slot
    if B > 1:
        ragged[0] = N
    holed = base.copy()
    holed[rng.random((B, N)) < 0.3] = np.inf
    holed[B - 1] = np.inf                                    # one utterance that is all +inf
    far = (1e4 * rng.integers(0, 4, size=(B, N))).astype(np.float32) + base
    return [("plain", base, None, False), ("ragged", base, ragged, False), ("none_live", base, np.zeros(B, np.int32), False),
            ("inf", holed, None, False), ("inf_ragged", holed, ragged, False), ("far", far, None, False),
            ("equal_costs", np.full((B, N), 3.25, np.float32), None, False), ("equal_errs", base, None, True)]


@pytest.mark.parametrize("B,N", SHAPES, ids=lambda v: str(v))
def test_risk_kernel_matches_the_oracle(hip_lib, B, N):
    for k, (name, costs, n_hyp, equal_errs) in enumerate(_variants(7 * B + N, B, N)):
        nh = None if n_hyp is None else torch.tensor(n_hyp, device="cuda")
        errs4 = _errors(100 * B + N + k, B, N, nh)
        if equal_errs:
            errs4 = errs4.clone()
            errs4[:, :, 0] = 6
        errs1 = errs4[:, :, 0].contiguous()
        e_host = errs1.cpu().numpy()
        if n_hyp is not None:                                # the slots behind n_hyp hold edit_distance's -1
            assert (e_host[np.arange(N)[None, :] >= n_hyp[:, None]] == -1).all()
        live = MR.live_mask(costs, n_hyp)
        max_err = int(e_host[live].max()) if live.any() else 0
        c = torch.tensor(costs, device="cuda")
        ref = np.random.default_rng(k).uniform(1.0, 30.0, size=B).astype(np.float32)
        for scale, nll, use_ref in ((1.0, 0.0, False), (1.0 / B, 0.3, True), (1.0, 0.3, False)):
            want_risk, want_post, want_coef = MR.risk(costs, e_host, n_hyp, scale)
            want_red = MR.reduced(want_risk, scale, nll, ref if use_ref else None)
            outs = []
            for errs in (errs1, errs4):                      # err stride 1 and 4
                r = torch.tensor(ref, device="cuda") if use_ref else None
                first = _native(c, errs, nh, r, nll, scale)
                again = _native(c, errs, nh, r, nll, scale)
                assert all(torch.equal(a, b) for a, b in zip(first, again)), name       # bit-equal from run to run
                outs.append(first)
            assert all(torch.equal(a, b) for a, b in zip(*outs)), name                  # the stride changes nothing
            risk, post, coef, red = (t.cpu().numpy() for t in outs[0])
            tag = "mwer %s B=%d N=%d scale=%.3g" % (name, B, N, scale)
            _close(risk, want_risk, max_err, tag + " risk")
            _close(post, want_post, 1, tag + " post")
            _close(coef, want_coef, max_err, tag + " coef")
            print("%s reduced %.9g want %.9g" % (tag, red[0], want_red))
            assert abs(float(red[0]) - want_red) <= RTOL * abs(want_red), tag
            if equal_errs or N == 1:
                assert (coef == 0).all(), tag
            if name == "none_live":
                assert (risk == 0).all() and (post == 0).all() and (coef == 0).all(), tag
            if name == "far":                                # costs 1e4 apart: finite everywhere, rows still sum to 1
                assert np.isfinite(risk).all() and np.isfinite(coef).all()
                np.testing.assert_allclose(post.sum(1), 1.0, rtol=1e-6)
    # `reduced` may be null: the per-utterance outputs are those of the call with it
    c = torch.tensor(_variants(1, B, N)[0][1], device="cuda")
    errs = _errors(5, B, N)
    with_red, without = _native(c, errs), _native(c, errs, reduced=False)
    assert without[3] is None and all(torch.equal(a, b) for a, b in zip(with_red[:3], without[:3]))


def test_autograd_wrappers(hip_lib):
    from edgedict_amd.loss import MWERLoss, mwer_risk
    B, N = 6, 7
    _, costs_np, n_hyp, _ = _variants(3, B, N)[4]            # +inf entries and a ragged n_hyp
    nh = torch.tensor(n_hyp, device="cuda")
    errs = _errors(11, B, N, nh)
    costs = torch.tensor(costs_np, device="cuda", requires_grad=True)
    risk, post = mwer_risk(costs, errs, nh)
    assert risk.requires_grad and not post.requires_grad
    want_risk, want_post, want_coef, _ = _native(costs.detach(), errs, nh)
    assert torch.equal(risk.detach(), want_risk) and torch.equal(post, want_post)
    g = torch.tensor([1.0, -2.0, 0.0, 0.5, 3.0, 1.5], device="cuda")
    risk.backward(g)
    assert torch.equal(costs.grad, g[:, None] * want_coef)
    # the [B, N] form of the errors and no n_hyp
    c2 = torch.tensor(costs_np, device="cuda", requires_grad=True)
    e2 = errs[:, :, 0].contiguous().clamp_(min=0)
    r2, _ = mwer_risk(c2, e2)
    r2.sum().backward()
    assert torch.equal(c2.grad, _native(c2.detach(), e2)[2])
    # the module: mean, sum and none, with the reference term
    ref_np = np.random.default_rng(2).uniform(5.0, 20.0, size=B).astype(np.float32)
    for reduction, scale in (("mean", 1.0 / B), ("sum", 1.0)):
        for nll in (0.0, 0.5):
            c = torch.tensor(costs_np, device="cuda", requires_grad=True)
            ref = torch.tensor(ref_np, device="cuda", requires_grad=True)
            crit = MWERLoss(nll, reduction)
            loss = crit(c, errs, nh, ref)
            assert tuple(loss.shape) == (1,)
            w_risk, w_post, w_coef, w_red = _native(c.detach(), errs, nh, ref.detach(), nll, scale)
            assert torch.equal(loss.detach(), w_red)
            assert torch.equal(crit.last_risk, w_risk) and torch.equal(crit.last_posterior, w_post)
            assert loss.requires_grad and not crit.last_risk.requires_grad and not crit.last_posterior.requires_grad
            loss.backward()
            assert torch.equal(c.grad, w_coef)
            assert torch.equal(ref.grad, torch.full((B,), scale * nll, dtype=F32, device="cuda"))
    c = torch.tensor(costs_np, device="cuda", requires_grad=True)
    ref = torch.tensor(ref_np, device="cuda", requires_grad=True)
    out = MWERLoss(0.5, "none")(c, errs, nh, ref)
    assert tuple(out.shape) == (B,) and torch.equal(out.detach(), want_risk + 0.5 * ref.detach())
    out.backward(g)
    assert torch.equal(c.grad, g[:, None] * want_coef) and torch.equal(ref.grad, 0.5 * g)
    # without ref_costs the weight-0 module takes none
    assert torch.equal(MWERLoss()(c.detach(), errs, nh), _native(c.detach(), errs, nh, None, 0.0, 1.0 / B)[3])


# ------------------------------------------------------------------------------------------ per-row packed costs
def _tiny():
    """tests/test_fastemit_gpu.py::_tiny"""
    from oracle import models_ref as M
    from oracle.make_golden import CASES
    cfg, B, T0, U, seed = CASES["tiny"]
    return cfg, M.make_state_dict(cfg, seed), M.make_batch(cfg, seed + 1, B, T0, U)


def _model(cfg, sd):
    from edgedict_amd.models import Transducer
    m = Transducer(enc_dropout=0.0, dec_dropout=0.0, **cfg)
    m.load_state_dict(sd, strict=True)
    m = m.cuda()
    m.compute_dtype = "fp32"
    return m


def _grads_close(got, want, what):
    """tests/test_fastemit_gpu.py::test_model_packed_and_dense_paths_agree...'s bound"""
    scale = max(want.abs().max().item(), 1e-8)
    err = (got - want).abs().max().item()
    print("%s: max err %.3g of max %.3g" % (what, err, scale))
    assert err <= 2e-5 * scale, what


@pytest.mark.parametrize("fused_db2", [True, False], ids=["db2_fused", "db2_plain"])
def test_packed_joint_row_costs_match_the_dense_path(hip_lib, fused_db2):
    from edgedict_amd import config
    from edgedict_amd.loss import RNNTLoss
    from edgedict_amd.models import _JointLossFn
    cfg, sd, (xs, ys, xlen, ylen) = _tiny()
    pick = [0, 1, 2, 0, 1]                                   # R = 5 rows, ragged, one without labels
    xs5, xlen5 = xs[pick].cuda(), xlen[pick].clone()
    g = torch.Generator(device="cpu").manual_seed(9)
    labels = torch.randint(4, cfg["vocab_size"], (5, 5), generator=g, dtype=torch.int32)
    ll = torch.tensor([5, 0, 3, 2, 4], dtype=torch.int32)
    gout = torch.tensor([1.0, 0.5, 0.0, -2.0, 0.25], device="cuda")    # one entry 0, one negative
    saved = config.FUSED_DB2
    config.FUSED_DB2 = fused_db2
    try:
        packed, dense = _model(cfg, sd), _model(cfg, sd)
        out = {}
        for name, m in (("packed", packed), ("dense", dense)):
            h_enc, _ = m.encoder(xs5)
            h_dec, _ = m.decoder(labels.cuda())
            h_enc.retain_grad()
            h_dec.retain_grad()
            act = m.scale_length(h_enc, xlen5)
            l1, l2 = m.joint.joint[0], m.joint.joint[2]
            if name == "packed":
                costs = _JointLossFn.apply(h_enc, h_dec, l1.weight, l1.bias, l2.weight, l2.bias, labels.cuda(), act, ll,
                                           m.blank, F32, 0.0, None, None, None, True)
            else:
                costs = RNNTLoss(blank=m.blank, reduction="none")(m.joint(h_enc, h_dec), labels.cuda(), act.cuda(),
                                                                   ll.cuda())
            assert tuple(costs.shape) == (5,) and costs.requires_grad
            costs.backward(gout)
            out[name] = (costs.detach().clone(), h_enc.grad, h_dec.grad)
        print("row costs packed %s dense %s" % (out["packed"][0].tolist(), out["dense"][0].tolist()))
        assert torch.equal(out["packed"][0], out["dense"][0])
        _grads_close(out["packed"][1], out["dense"][1], "enc")
        _grads_close(out["packed"][2], out["dense"][2], "dec")
        for (n, a), (_, b) in zip(packed.named_parameters(), dense.named_parameters()):
            _grads_close(a.grad, b.grad, n)
        assert out["dense"][1][2].abs().max().item() == 0 and out["packed"][1][2].abs().max().item() == 0   # gout 0
        # today's path on the same batch: the mean loss is Transducer.forward's, and the mean of these costs
        plain = _model(cfg, sd)
        with torch.no_grad():
            h_enc, _ = plain.encoder(xs5)
            h_dec, _ = plain.decoder(labels.cuda())
            l1, l2 = plain.joint.joint[0], plain.joint.joint[2]
            mean = _JointLossFn.apply(h_enc, h_dec, l1.weight, l1.bias, l2.weight, l2.bias, labels.cuda(),
                                      plain.scale_length(h_enc, xlen5), ll, plain.blank, F32, 0.0)
            fwd = plain(xs5, labels.cuda(), xlen5, ll)
        assert tuple(mean.shape) == (1,) and torch.equal(mean, fwd)
        assert abs(mean.item() - out["packed"][0].double().mean().item()) <= 1e-6 * abs(mean.item())
    finally:
        config.FUSED_DB2 = saved


# ------------------------------------------------------------------------------------------ model, handwritten lists
def _handwritten(ys, ylen):
    """1 to 4 hypotheses per utterance, near-copies of the reference: a substitution, a deletion, an insertion, the
    empty sequence."""
    refs = [ys[b, :int(ylen[b])].numpy().astype(np.int64) for b in range(ys.shape[0])]
    r0, r1, r2 = refs
    sub0 = r0.copy()
    sub0[1] = 4 if r0[1] != 4 else 5
    sub1 = r1.copy()
    sub1[0] = 6 if r1[0] != 6 else 7
    lists = [[sub0, np.delete(r0, 2), np.insert(r0, 3, 9), np.zeros(0, dtype=np.int64)],
             [r1.copy(), sub1],
             [np.delete(r2, 0)]]
    return lists, refs


def _composed(model, xs, xlen, lists, refs, nll_weight):
    """The loss from validated pieces: dense joint on the repeated encoder rows, RNNTLoss('none'), the errors of
    tests/edit_distance_ref.py, torch float64 softmax-risk.  Returns (loss, costs per utterance, errors, risk)."""
    from edgedict_amd.loss import RNNTLoss
    B = len(lists)
    seqs = [(b, t) for b in range(B) for t in lists[b]]
    if nll_weight > 0:
        seqs += [(b, refs[b]) for b in range(B)]
    U = max(1, max(t.size for _, t in seqs))
    labels = torch.zeros(len(seqs), U, dtype=torch.int32)
    for r, (_, t) in enumerate(seqs):
        labels[r, :t.size] = torch.from_numpy(t.astype(np.int32))
    ll = torch.tensor([t.size for _, t in seqs], dtype=torch.int32)
    utt = torch.tensor([b for b, _ in seqs])
    h_enc, _ = model.encoder(xs[:, :xlen.max()].contiguous())
    act = model.scale_length(h_enc, xlen)
    h_dec, _ = model.decoder(labels.cuda())
    logits = model.joint(h_enc[utt.cuda()].contiguous(), h_dec)
    costs = RNNTLoss(blank=model.blank, reduction="none", check_lengths=False)(
        logits, labels.cuda(), act[utt].cuda().contiguous(), ll.cuda())
    total, per_utt, errors, risks, r = 0.0, [], [], [], 0
    for b in range(B):
        n = len(lists[b])
        c = costs[r:r + n].double()
        e = torch.tensor([ER.counts(t.tolist(), refs[b].tolist())[0] for t in lists[b]], dtype=torch.float64, device="cuda")
        risk = (torch.softmax(-c, 0) * e).sum()
        total = total + risk
        per_utt.append(costs[r:r + n].detach())
        errors.append(e.cpu().numpy().astype(np.int64))
        risks.append(risk.item())
        r += n
    if nll_weight > 0:
        total = total + nll_weight * costs[r:].double().sum()
    return total / B, per_utt, errors, risks


@pytest.mark.parametrize("nll_weight", [0.0, 0.5])
def test_mwer_loss_on_handwritten_lists_matches_the_composed_form(hip_lib, nll_weight):
    cfg, sd, (xs, ys, xlen, ylen) = _tiny()
    lists, refs = _handwritten(ys, ylen)
    ours, theirs = _model(cfg, sd), _model(cfg, sd)
    want, want_costs, want_errs, want_risk = _composed(theirs, xs.cuda(), xlen, lists, refs, nll_weight)
    want.backward()
    # the comparison shows something only if the risk has a gradient: two utterances hold two live hypotheses with
    # different error counts, and the composed form's gradient reaches the joint
    assert sum(len(set(e.tolist())) >= 2 for e in want_errs) >= 2
    assert theirs.joint.joint[0].weight.grad.abs().max().item() > 1e-6
    loss = ours.mwer_loss(xs.cuda(), ys, xlen, ylen, nbest=lists, nll_weight=nll_weight)
    assert tuple(loss.shape) == (1,) and loss.dtype == F32
    loss.backward()
    last = ours.last_mwer
    print("mwer loss %.9g composed %.9g" % (loss.item(), want.item()))
    assert abs(loss.item() - want.item()) <= RTOL * abs(want.item())
    assert [[t.tolist() for t in own] for own in last["lists"]] == [[t.tolist() for t in own] for own in lists]
    assert last["n_hyp"].tolist() == [4, 2, 1]
    N = 4
    assert tuple(last["costs"].shape) == (3, N) and tuple(last["errors"].shape) == (3, N, 4)
    for b in range(3):
        n = len(lists[b])
        assert torch.equal(last["costs"][b, :n], want_costs[b]), b           # the packed rows' costs are the dense ones
        assert torch.isinf(last["costs"][b, n:]).all() and (last["costs"][b, n:] > 0).all()
        assert last["errors"][b, :n, 0].tolist() == want_errs[b].tolist()
        assert (last["errors"][b, n:] == -1).all()
        p = torch.softmax(-want_costs[b].double(), 0).cpu().numpy()
        _close(last["posterior"][b, :n].cpu().numpy(), p, 1, "posterior %d" % b)
        assert (last["posterior"][b, n:] == 0).all()
    _close(last["risk"].cpu().numpy(), np.array(want_risk), max(int(e.max()) for e in want_errs), "risk")
    for (n, a), (_, b) in zip(ours.named_parameters(), theirs.named_parameters()):
        _grads_close(a.grad, b.grad, n)
    # duplicates in a given list change nothing; NBestResult lists are taken as they are
    from edgedict_amd.decode import NBestResult
    again = _model(cfg, sd)
    doubled = [own + [own[0].copy()] + own[::-1] for own in lists]
    l2 = again.mwer_loss(xs.cuda(), ys.cuda(), xlen, ylen, nbest=doubled, nll_weight=nll_weight)
    assert torch.equal(l2, loss.detach())
    assert [[t.tolist() for t in own] for own in again.last_mwer["lists"]] == [[t.tolist() for t in own] for own in lists]
    boxed = [NBestResult(own, [np.zeros(t.size, np.int32) for t in own], [np.zeros(t.size) for t in own],
                         np.zeros(len(own))) for own in lists]
    assert torch.equal(again.mwer_loss(xs.cuda(), ys, xlen, ylen, nbest=boxed, nll_weight=nll_weight), loss.detach())
    with pytest.raises(ValueError, match="one list per utterance"):
        again.mwer_loss(xs.cuda(), ys, xlen, ylen, nbest=lists[:2])
    with pytest.raises(ValueError, match="on the host"):
        again.mwer_loss(xs.cuda(), ys, xlen.cuda(), ylen, nbest=lists)


# ------------------------------------------------------------------------------------------ model, searched lists
# (the tiny model's flat distributions make the legacy search pop often: tests/test_beam_gpu.py's max_expansions)
@pytest.mark.parametrize("search,kw", [("sync_beam", {}), ("beam", dict(max_expansions=400))], ids=["sync_beam", "beam"])
def test_mwer_loss_searches_its_own_lists(hip_lib, search, kw):
    from edgedict_amd import decode, metrics
    cfg, sd, (xs, ys, xlen, ylen) = _tiny()
    m = _model(cfg, sd).eval()
    W = 4
    loss = m.mwer_loss(xs.cuda(), ys, xlen, ylen, W=W, search=search, **kw)     # the search arguments pass through
    assert torch.isfinite(loss).all()
    loss.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
    last = m.last_mwer
    with torch.no_grad():
        enc, _ = m.encoder(xs.cuda())
        lens = m.scale_length(enc, xlen).numpy().astype(np.int32)
        if search == "sync_beam":
            found = decode.sync_beam_search_nbest_enc(m, enc, lens, W)
        else:
            found = [r.ranked(merge=True) for r in decode.beam_search_nbest_enc(m, enc, lens, W, **kw)]
    assert [[t.tolist() for t in own] for own in last["lists"]] == \
        [[t.tolist() for t in r.tokens] or [[]] for r in found]
    assert last["n_hyp"].tolist() == [len(own) for own in last["lists"]]
    # the risk is metrics.expected_errors of the lists under the costs the loss worked with
    costs = last["costs"].cpu().numpy()
    results = [decode.NBestResult(own, [np.zeros(t.size, np.int32) for t in own], [np.zeros(t.size) for t in own],
                                  -costs[b, :len(own)].astype(np.float64)) for b, own in enumerate(last["lists"])]
    refs = [ys[b, :int(ylen[b])].numpy() for b in range(ys.shape[0])]
    want = metrics.expected_errors(results, refs)
    got = last["risk"].cpu().numpy()
    print("mwer searched (%s): risk %s expected_errors %s" % (search, got.tolist(), want.tolist()))
    np.testing.assert_allclose(got, want, rtol=1e-6)
    assert abs(loss.item() - want.mean()) <= 1e-6 * want.mean()


# ------------------------------------------------------------------------------------------ trainer
def _flags():
    """tests/test_train_step_gpu.py::_flags"""
    return types.SimpleNamespace(
        downsample=3, win_length=320, hop_length=160, n_fft=512, feature_size=80, dither=0.0,
        sample_rate=16000, lr=1e-3, gradclip=None, sub_batch_size=None, bpe_size=40,
        vocab_embed_size=8, enc_hidden_size=64, enc_layers=3, enc_dropout=0.0, enc_proj_size=24,
        dec_hidden_size=32, dec_layers=2, dec_dropout=0.0, dec_proj_size=16, joint_size=32,
        enc_time_reductions=[1], delta=False)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_train_engine_mwer_step(hip_lib, dtype):
    from edgedict_amd.trainer import TrainEngine
    g = torch.Generator(device="cpu").manual_seed(4)
    wave = (0.1 * torch.randn(4, 12000, generator=g)).cuda()
    wlen = torch.tensor([12000, 11000, 9000, 12000], dtype=torch.int32)
    ys = torch.randint(4, 40, (4, 6), generator=g, dtype=torch.int32)
    ylen = torch.tensor([6, 4, 5, 6], dtype=torch.int32)
    losses = []
    for _ in range(2):                                       # two engines fed identically
        torch.manual_seed(0)
        eng = TrainEngine(_flags(), vocab_size=40, device="cuda", compute_dtype=dtype)
        try:
            before = eng.flat.data.clone()
            loss = eng.mwer_step(wave, wlen, ys, ylen, W=3, nll_weight=0.1)
            torch.cuda.synchronize()
            eng.check()
            assert tuple(loss.shape) == (1,) and torch.isfinite(loss).all() and not loss.requires_grad
            assert eng.step_count == 1 and not torch.equal(eng.flat.data, before)
            assert torch.isfinite(eng.flat.data).all()
            assert sorted(eng.model.last_mwer) == ["costs", "errors", "lists", "n_hyp", "posterior", "risk"]
            nxt = eng.train_step(wave, wlen, ys.cuda(), ylen)              # a following train_step works
            torch.cuda.synchronize()
            assert torch.isfinite(nxt).all() and eng.step_count == 2
            losses.append(loss.clone())
        finally:
            eng.close()
    print("mwer_step (%s): loss %.6g" % (dtype, losses[0].item()))
    assert torch.equal(losses[0], losses[1])
