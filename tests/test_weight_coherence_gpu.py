"""GPU: cached weight images follow their fp32 masters.

No kernel reads a master parameter directly: each reads an image kept in a cache (models.WEIGHTS, the encoder stack's
packed layers, the streaming decoder's bound chunk plan), keyed by address, version counter and the engine-wide parameter
epoch.  A training run that read images one step old would still see its loss fall.  Here every step of a run, every
search after it and every way of changing a weight is compared with a WITNESS (tests/coherence_ref.py): a model rebuilt
from a state-dict snapshot into new Parameter objects, running the same kernels on the same inputs, with no cache cleared.

Witness against witness (two witnesses of one snapshot, same batch; measured on an MI355X, both compute dtypes, and
re-asserted by ``test_two_witnesses_of_one_snapshot_agree``): the forward loss is bit-identical in bf16 and in fp32; the
gradients are not quite - max |g_a - g_b| = 1.2e-7 (bf16) and 9.5e-7 (fp32) at max|g| = 14.0, i.e. 8e-9 and 7e-8 of it,
against a bound of 2.8e-4.  Engine against witness the gradients differ by up to 5.7e-6 (the engine accumulates in
place on the auxiliary stream, the witness goes through autograd).
The forward loss is therefore asserted with ``==``; gradients with the project's bound for fp32 sums that atomics reorder,
2e-5 x max|g| (tests/test_train_step_gpu.py).  Every comparison has its control: the witness of the snapshot from ONE STEP
EARLIER must differ in loss, and in gradients by at least 100 x the bound - without it a stale image could not fail."""
import gc

import numpy as np
import pytest
import torch
from torch import nn

import coherence_ref as C

pytestmark = pytest.mark.gpu
DTYPES = ["bf16", "fp32"]


# ------------------------------------------------------------------------------------------------ batches
def _batches(n=3, seed=11, B=5):
    g = torch.Generator(device="cpu").manual_seed(seed)
    out = []
    for i in range(n):
        wave = (0.1 * torch.randn(B, 16000, generator=g)).cuda()
        wlen = torch.tensor([16000, 15000 - 500 * i, 12000, 16000, 9000 + 300 * i][:B], dtype=torch.int32)
        ys = torch.randint(4, C.V, (B, 7), generator=g, dtype=torch.int32).cuda()
        ylen = torch.tensor([7, 5, 6, 3, 7][:B], dtype=torch.int32)
        out.append((wave, wlen, ys, ylen))
    return out


def _engine(fl, dtype, seed=3):
    from edgedict_amd.trainer import TrainEngine
    torch.manual_seed(seed)
    return TrainEngine(fl, vocab_size=C.V, device="cuda", compute_dtype=dtype)


def _slices(eng, batch):
    """What train_step will feed the model: the features of each sub-batch slice (dither 0: computed again, they are the same)."""
    wave, wlen, ys, ylen = batch
    B = wave.shape[0]
    sub = eng.sub_batch_size or B
    out = []
    for s in range(0, B, sub):
        e = min(B, s + sub)
        xs, xlen = eng.features(wave[s:e], wlen[s:e])
        out.append((xs, ys[s:e], xlen, ylen[s:e]))
    return out


def _names(eng):
    by_id = {id(p): n for n, p in eng.model.named_parameters()}
    return [by_id[id(p)] for p in eng.flat.params]


class _Run:
    """Steps an engine and checks every step against the witness of the snapshot taken right before it."""

    def __init__(self, eng, dtype, expect_stack_modes=None):
        self.eng, self.dtype = eng, dtype
        self.prev = None                  # the snapshot one step earlier
        self.modes = (dtype == "bf16") if expect_stack_modes is None else expect_stack_modes
        self.margins = []

    def step(self, batch, **kw):
        from edgedict_amd import encoder_stack
        eng = self.eng
        sd = C.snapshot(eng.model)
        slices = _slices(eng, batch)
        loss = eng.train_step(*batch, **kw)
        if self.modes:
            # the kernels bench.py times: launch-persistent forward, split-K weights-stationary BPTT
            assert encoder_stack.last_mode(False)[0] == 1 and encoder_stack.last_mode(True)[0] == 2
        torch.cuda.synchronize()
        eng.check()
        got_loss, got = loss.item(), C.flat_grads(eng.flat)
        want_loss, want = C.loss_and_grads(C.transducer(sd, eng.flags, self.dtype), slices)
        names = _names(eng)
        print("step %d: loss %.9g witness %.9g, grad diff %.3e (bound %.3e)"
              % (eng.step_count, got_loss, want_loss, C.max_grad_diff(got, want), C.grad_bound(want)))
        assert got_loss == want_loss, "step %d read weights that are not the ones the previous step wrote" % eng.step_count
        C.assert_same_grads(names, got, want, "step %d:" % eng.step_count)
        if self.prev is not None:
            # the control: had the step read the images of one step earlier, this is what it would have computed
            old_loss, old = C.loss_and_grads(C.transducer(self.prev, eng.flags, self.dtype), slices)
            margin = C.max_grad_diff(got, old) / C.grad_bound(want)
            print("         stale witness: loss %.9g, grad diff / bound = %.1f" % (old_loss, margin))
            assert old_loss != got_loss
            assert margin >= 100.0, "the control cannot tell a stale step from a fresh one (margin %.1f): raise lr" % margin
            self.margins.append(margin)
        self.prev = sd
        return got_loss


# ------------------------------------------------------------------------------------------------ 1. the witness itself
@pytest.mark.parametrize("dtype", DTYPES)
def test_two_witnesses_of_one_snapshot_agree(hip_lib, dtype):
    """The measurement behind the module docstring's rule: loss bit-identical, gradients within the atomics bound."""
    eng = _engine(C.flags(), dtype)
    sd = C.snapshot(eng.model)
    slices = _slices(eng, _batches(1)[0])
    la, ga = C.loss_and_grads(C.transducer(sd, eng.flags, dtype), slices)
    lb, gb = C.loss_and_grads(C.transducer(sd, eng.flags, dtype), slices)
    print("witness vs witness (%s): loss %.9g / %.9g, max grad diff %.3e, bound %.3e, max|g| %.3e"
          % (dtype, la, lb, C.max_grad_diff(ga, gb), C.grad_bound(ga), max(g.abs().max().item() for g in ga)))
    assert la == lb
    C.assert_same_grads(_names(eng), ga, gb, "witness vs witness:")
    eng.close()


# ------------------------------------------------------------------------------------------------ 2. training steps
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_training_step_reads_what_the_previous_step_wrote(hip_lib, dtype):
    """Four steps over three batches: loss == witness, gradients within the bound, and the stale control >= 100 x."""
    eng = _engine(C.flags(), dtype)
    run = _Run(eng, dtype)
    b = _batches()
    losses = [run.step(b[i]) for i in (0, 1, 2, 1)]
    assert len(run.margins) == 3 and all(x == x and x > 0 for x in losses)
    eng.close()


def _variant(dtype, steps=3, order=(0, 1, 2), prefetch=False, **over):
    eng = _engine(C.flags(**over), dtype)
    run = _Run(eng, dtype)
    b = _batches()
    for i, k in enumerate(order[:steps]):
        nxt = None
        if prefetch and i + 1 < steps:
            nb = b[order[i + 1]]
            nxt = (nb[0], nb[1])
        run.step(b[k], **({"next_batch": nxt} if prefetch else {}))
    assert len(run.margins) == steps - 1
    eng.close()
    return run


@pytest.mark.parametrize("dtype", DTYPES)
def test_steps_with_the_next_batch_prefetched(hip_lib, dtype):
    _variant(dtype, prefetch=True)


@pytest.mark.parametrize("dtype", DTYPES)
def test_steps_in_sub_batches_two_forwards_one_refresh(hip_lib, dtype):
    _variant(dtype, steps=2, sub_batch_size=2)


@pytest.mark.parametrize("dtype", DTYPES)
def test_steps_with_gradient_clipping(hip_lib, dtype):
    _variant(dtype, steps=2, gradclip=0.5)


@pytest.mark.parametrize("dtype", DTYPES)
def test_steps_with_the_ctc_head(hip_lib, dtype):
    _variant(dtype, steps=2, ctc_weight=0.3)


def test_steps_on_the_per_layer_encoder_in_bf16(hip_lib, monkeypatch):
    from edgedict_amd import config
    monkeypatch.setattr(config, "USE_ENCODER_STACK", False)
    eng = _engine(C.flags(), "bf16")
    run = _Run(eng, "bf16", expect_stack_modes=False)
    b = _batches()
    for k in (0, 1, 2):
        run.step(b[k])
    eng.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_steps_with_weight_gradients_through_autograd(hip_lib, monkeypatch, dtype):
    from edgedict_amd import config
    monkeypatch.setattr(config, "DEFER_WEIGHT_GRADS", False)
    _variant(dtype, steps=2)


def test_steps_with_the_adam_guard_at_its_default(hip_lib, monkeypatch):
    monkeypatch.delenv("EDGEDICT_ADAM_GUARD", raising=False)
    eng = _engine(C.flags(), "bf16")
    assert eng._guard                                    # the optimiser step reads the stack's give-up words
    run = _Run(eng, "bf16")
    b = _batches()
    run.step(b[0])
    run.step(b[1])
    eng.close()


def test_two_engines_stepping_alternately(hip_lib):
    """The prepack events and the parameter epoch are process-global: engine A's refresh must not stand in for engine B's."""
    a, b = _engine(C.flags(), "bf16", seed=3), _engine(C.flags(), "bf16", seed=4)
    ra, rb = _Run(a, "bf16"), _Run(b, "bf16")
    bt = _batches()
    for k in (0, 1, 2):
        ra.step(bt[k])
        rb.step(bt[(k + 1) % 3])
    assert len(ra.margins) == 2 and len(rb.margins) == 2
    a.close()
    b.close()


def test_back_to_back_steps_without_a_synchronise(hip_lib):
    """The per-step checks above read a snapshot before every step and synchronise after it: by the next forward pass the
    auxiliary stream's prepack has long finished, so they cannot see a missing wait for it.  Here five steps are enqueued
    with nothing in between and compared with the same five steps synchronised one by one.

    Bound, from reasoning: a forward pass that read images of the step before is off by about what one step changes the
    loss by - 10 % or more at this lr (63.0 -> 53.3 -> 48.3 above).  Two correct runs can differ only through fp32 sums
    that atomics reorder in the gradients (relative 2e-5 at most, the bound of this module); Adam can turn that into a
    different update only for elements whose gradient is itself about zero, which move the loss by g x dw ~ nothing.  So
    every loss must agree to 1e-4 relative - a thousand times below the effect looked for - and the final masters on
    average to lr / 100 per element (a stale step moves most elements by a good part of lr)."""
    def run(sync):
        eng = _engine(C.flags(), "bf16")
        b = _batches()
        losses = []
        for k in (0, 1, 2, 1, 0):
            losses.append(eng.train_step(*b[k]))
            if sync:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        eng.check()
        out = [x.item() for x in losses], eng.flat.data.clone()
        eng.close()
        return out

    stepwise, w_stepwise = run(True)
    queued, w_queued = run(False)
    print("stepwise %s\nqueued   %s\nmean |dw| %.3e" % (stepwise, queued, (w_stepwise - w_queued).abs().mean().item()))
    assert all(x == x and x > 0 for x in stepwise)
    for a, q in zip(stepwise, queued):
        assert abs(a - q) <= 1e-4 * abs(a), (stepwise, queued)
    assert (w_stepwise - w_queued).abs().mean().item() <= C.flags().lr / 100


LM_CFG = {True: dict(args=(C.V, 32, 32, 2), tied=True), False: dict(args=(C.V, 16, 32, 2), tied=False)}


def _lm_batch(seed):
    from edgedict_amd.lm import seq_collate
    g = torch.Generator(device="cpu").manual_seed(seed)
    sents = [torch.randint(2, C.V, (n,), generator=g) for n in (9, 5, 7, 3)]
    return seq_collate(sents)


def _lm_trainer(cfg, dtype, seed=5, lr=3e-3):
    from edgedict_amd.lm import LMModel, LMTrainer
    torch.manual_seed(seed)
    m = LMModel(*cfg["args"], dropout=0.0, tie_weights=cfg["tied"]).cuda()
    return LMTrainer(m, lr=lr, dtype=dtype)


def _lm_names(tr):
    by_id = {id(p): n for n, p in tr.model.named_parameters()}
    return [by_id[id(p)] for p in tr.optimizer.flat.params]


def _lm_steps(tr, cfg, dtype, n=3):
    prev = None
    for k in range(n):
        inputs, targets = _lm_batch(20 + k)
        sd = C.snapshot(tr.model)
        loss = tr.train_step(inputs, targets)
        torch.cuda.synchronize()
        got_loss, got = loss.item(), C.flat_grads(tr.optimizer.flat)
        want_loss, want = C.lm_loss_and_grads(C.lm(sd, cfg, dtype), inputs, targets)
        assert got_loss == want_loss, "LM step %d" % k
        C.assert_same_grads(_lm_names(tr), got, want, "LM step %d:" % k)
        if prev is not None:
            old_loss, old = C.lm_loss_and_grads(C.lm(prev, cfg, dtype), inputs, targets)
            margin = C.max_grad_diff(got, old) / C.grad_bound(want)
            print("LM step %d: stale margin %.1f" % (k, margin))
            assert old_loss != got_loss and margin >= 100.0, margin
        prev = sd


@pytest.mark.parametrize("tied", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
def test_lm_trainer_steps(hip_lib, dtype, tied):
    cfg = LM_CFG[tied]
    _lm_steps(_lm_trainer(cfg, dtype), cfg, dtype)


# ------------------------------------------------------------------------------------------------ 3. inference after training
def _same_seqs(a, b, what):
    assert len(a) == len(b), what
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x), np.asarray(y)), (what, x, y)


def _same_scores(a, b, what):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    assert a.shape == b.shape and np.array_equal(a, b), (what, a, b)


def _same_nbest(a, b, what):
    assert len(a) == len(b), what
    for i, (x, y) in enumerate(zip(a, b)):
        assert len(x) == len(y), (what, i)
        _same_seqs(x.tokens, y.tokens, (what, i, "tokens"))
        _same_seqs(x.frames, y.frames, (what, i, "frames"))
        _same_seqs(x.token_logp, y.token_logp, (what, i, "token_logp"))
        _same_scores(x.logp, y.logp, (what, i, "logp"))


@pytest.mark.parametrize("dtype", DTYPES)
def test_searches_after_in_place_training_use_the_trained_weights(hip_lib, dtype):
    """Every search, warmed on the weights before the last training steps (an evaluation between steps), then run after
    them: tokens, frames and N-best lists equal those of the witness of the final snapshot, scores bit for bit.  The
    control: the same searches on the witness of the snapshot before those steps give something else.

    ``beam_search_batch`` and ``sync_beam_search`` are run through their ``_nbest`` forms: the same ``_SearchNet`` /
    ``FusionLM`` bundles and kernels, and the whole list is compared (entry 0 is what the plain forms return)."""
    from edgedict_amd import decode
    from edgedict_amd.stream import BatchedStreamDecoder, chunk_geometry
    fl = C.flags(ctc_weight=0.3, lr=1e-2)
    eng = _engine(fl, dtype)
    m = eng.model
    b = _batches()
    S, W = 5, 4
    xs, xlen = eng.features(b[2][0], b[2][1])
    win, hop = chunk_geometry(fl, 2)
    chunks = [b[1][0][:4, k * hop:k * hop + win].contiguous() for k in range(2)]
    cfg = LM_CFG[False]
    lm_tr = _lm_trainer(cfg, dtype, lr=1e-2)

    def offline(model, lm):
        model.eval()
        lm.eval()
        with torch.no_grad():
            out = dict(greedy=model.greedy_decode(xs, xlen),
                       beam=model.beam_search_nbest(xs, xlen, W=W),
                       sync=model.sync_beam_search_nbest(xs, xlen, W=W),
                       ctc=model.ctc_beam_search(xs, xlen, W=W),
                       fused=model.beam_search_nbest(xs, xlen, W=W, lm=lm, lm_weight=0.3))
        torch.cuda.synchronize()
        return out

    def searches(model):
        return dict(beam=decode.StreamingBeamSearch(model, S, W=W, detail=True),
                    sync=decode.StreamingSyncBeamSearch(model, S, W=W),
                    ctc=decode.StreamingCTCBeamSearch(S, C.V, W=W, cand=8, blank=model.blank))

    def streamed(model, sb, dec):
        model.eval()
        with torch.no_grad():
            enc, _ = model.encoder(xs)
            enc = enc.contiguous()
            T = enc.shape[1]
            assert T >= 4
            for t0, t1 in ((0, T // 2), (T // 2, T)):
                part = enc[:, t0:t1].contiguous()
                sb["beam"].advance(part)
                sb["sync"].advance(part)
                sb["ctc"].advance(model._ctc_logits(part).contiguous())
            dec.reset()
            toks = dec.decode(chunks[1].clone())
        torch.cuda.synchronize()
        return dict(beam=sb["beam"].nbest(), sync=sb["sync"].nbest(), ctc=sb["ctc"].nbest(), chunk=toks.cpu().numpy())

    # an evaluation in the middle of training: every inference-side image exists, built from the weights of now
    eng.train_step(*b[0])
    before = C.snapshot(m)
    lm_before = C.snapshot(lm_tr.model)
    warm = offline(m, lm_tr.model)
    sb = searches(m)
    dec = BatchedStreamDecoder(m, fl, 4, dither=0)
    dec.decode(chunks[0].clone())
    if dtype == "bf16":
        assert dec._plan is not None and dec._plan.ok
    # ... training goes on, in place
    for k in (1, 2, 0, 1):
        eng.train_step(*b[k])
    for k in range(4):
        lm_tr.train_step(*_lm_batch(30 + k))
    torch.cuda.synchronize()
    eng.check()
    got = offline(m, lm_tr.model)
    got_s = streamed(m, sb, dec)
    if dtype == "bf16":
        assert dec._plan is not None and dec._plan.ok          # the fused chunk path, rebuilt for the new weights
    after, lm_after = C.snapshot(m), C.snapshot(lm_tr.model)

    def witness(sd, lm_sd):
        wm, wl = C.transducer(sd, fl, dtype, train=False), C.lm(lm_sd, cfg, dtype, train=False)
        return offline(wm, wl), streamed(wm, searches(wm), BatchedStreamDecoder(wm, fl, 4, dither=0))

    want, want_s = witness(after, lm_after)
    _same_seqs(got["greedy"][0], want["greedy"][0], "greedy tokens")
    _same_scores(got["greedy"][1], want["greedy"][1], "greedy scores")
    for k in ("beam", "sync", "ctc", "fused"):
        _same_nbest(got[k], want[k], k)
    for k in ("beam", "sync", "ctc"):
        _same_nbest(got_s[k], want_s[k], "streaming " + k)
    assert np.array_equal(got_s["chunk"], want_s["chunk"])
    # the control: stale images would have given the scores of the weights before those steps
    old, old_s = witness(before, lm_before)
    assert not np.array_equal(got["greedy"][1].cpu().numpy(), old["greedy"][1].cpu().numpy())
    _same_scores(warm["greedy"][1], old["greedy"][1], "the warm-up is the old witness")
    for k in ("beam", "sync", "ctc", "fused"):
        assert any(not np.array_equal(x.logp, y.logp) for x, y in zip(got[k], old[k])), k
    for k in ("beam", "sync", "ctc"):
        assert any(not np.array_equal(x.logp, y.logp) for x, y in zip(got_s[k], old_s[k])), k
    # the LM alone: the fused search with the TRAINED transducer but the LM of before differs too
    stale_lm = offline(C.transducer(after, fl, dtype, train=False), C.lm(lm_before, cfg, dtype, train=False))
    assert any(not np.array_equal(x.logp, y.logp) for x, y in zip(got["fused"], stale_lm["fused"]))
    eng.close()


# ------------------------------------------------------------------------------------------------ 4. every way of changing a weight
def _plain_model(dtype, seed=7):
    from edgedict_amd.flags import model_kwargs
    from edgedict_amd.models import Transducer
    torch.manual_seed(seed)
    m = Transducer(**model_kwargs(C.flags(), vocab_size=C.V)).cuda()
    m.compute_dtype = dtype
    return m


def _inputs(seed=2):
    g = torch.Generator(device="cpu").manual_seed(seed)
    xs = torch.randn(5, 34, 240, generator=g).cuda()
    xlen = torch.tensor([34, 31, 25, 34, 19], dtype=torch.int32)
    ys = torch.randint(4, C.V, (5, 7), generator=g, dtype=torch.int32).cuda()
    ylen = torch.tensor([7, 5, 6, 3, 7], dtype=torch.int32)
    return xs, ys, xlen, ylen


def _use(m, inp, grads=None):
    """forward + backward + one greedy decode: (loss, gradients, tokens, scores).  ``grads``: where to read the gradients
    (default: fresh ``.grad`` tensors from autograd)."""
    xs, ys, xlen, ylen = inp
    m.train()
    if grads is None:
        for p in m.parameters():
            p.grad = None
    loss = m(xs, ys, xlen, ylen)
    loss.backward()
    m.eval()
    toks, score = m.greedy_decode(xs, xlen)
    torch.cuda.synchronize()
    return loss.item(), (grads() if grads else [p.grad.detach().clone() for p in m.parameters()]), toks, score.cpu()


def _check_against_witness(m, inp, dtype, warm, what, grads=None):
    got = _use(m, inp, grads)
    want = _use(C.transducer(C.snapshot(m), C.flags(), dtype), inp)
    assert got[0] != warm[0], "%s: the change did not reach the loss at all - nothing is being tested" % what
    assert got[0] == want[0], "%s: loss %.9g, witness of the new state dict %.9g (before the change %.9g)" % (
        what, got[0], want[0], warm[0])
    C.assert_same_grads([n for n, _ in m.named_parameters()], got[1], want[1], what + ":")
    _same_seqs(got[2], want[2], what + ": tokens")
    _same_scores(got[3], want[3], what + ": greedy scores")
    return got


def _each_param(m):
    return [(mod, name, p) for mod in m.modules() for name, p in list(mod._parameters.items()) if p is not None]


def _torch_optim(make):
    def go(m):
        make([p for p in m.parameters()]).step()          # on the gradients of the warm-up's backward pass
    return go


def _no_grad_mul(m):
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(0.5)


def _load_state_dict(m):
    m.load_state_dict({k: v * 0.5 for k, v in C.snapshot(m).items()})


def _load_state_dict_assign(m):
    m.load_state_dict({k: nn.Parameter(v.cuda() * 0.5) for k, v in C.snapshot(m).items()}, assign=True)


def _new_parameters(m):
    for mod, name, p in _each_param(m):
        setattr(mod, name, nn.Parameter(p.detach() * 0.5))


def _data_swap(m):
    for p in m.parameters():
        p.data = p.detach() * 0.5


def _data_swap_lstm_biases(m):
    """Only the recurrent layers' biases get a new `.data`: the weights' addresses and every version counter stay, so the
    encoder stack's packed bias image has nothing but the biases' own addresses to notice it by."""
    n = 0
    for name, p in m.named_parameters():
        if ".bias_ih_" in name or ".bias_hh_" in name:
            p.data = p.detach() * 0.5 + 0.25
            n += 1
    assert n == 10


def _pinned_addresses():
    from edgedict_amd import encoder_stack, models
    held = {v[3].data_ptr() for v in models.WEIGHTS._store.values()}
    for ent in encoder_stack._PACKED.values():
        held |= {t.data_ptr() for t in ent.pinned}
    return held


def _data_swap_twice(m, also_held=()):
    """`p.data = a; p.data = b`, with b allocated right after a's predecessor - the tensor the images were built from - lost
    its last user-side reference: at the same size the caching allocator hands that block back, unless someone holds it.
    The cache entries do (``also_held``: tensors something else holds, a bound chunk plan's); a parameter nobody caches an
    image of (biases, LayerNorm) collides - nothing reads a copy of it.  What happened is left in ``_data_swap_twice.last``
    for ``_double_swap_verdict``, which the test calls once its comparison with the witness is through."""
    big = max(m.parameters(), key=lambda p: p.numel())
    t = torch.empty_like(big)
    addr = t.data_ptr()
    del t
    t = torch.empty_like(big)
    obliges = t.data_ptr() == addr                   # does this allocator return a block it was just given back?
    del t
    held = _pinned_addresses() | {t.data_ptr() for t in also_held}
    collided, protected, free = [], 0, 0
    for name, p in m.named_parameters():
        new = p.detach() * 0.5
        addr0, ver0 = p.data_ptr(), p._version
        p.data = p.detach().clone()                  # a
        b = torch.empty_like(p)
        if b.data_ptr() == addr0:
            collided.append(name)
        if addr0 in held:
            protected += 1
            assert b.data_ptr() != addr0, "%s: the block an image was built from was handed out again" % name
        else:
            free += 1
        p.data = b.copy_(new)                        # b
        assert p._version == ver0                    # set_data keeps the counter: only the address can tell
    print("double swap: allocator obliges: %s; %d cached parameters held their block; uncached collisions: %s"
          % (obliges, protected, collided))
    assert protected >= 10
    _data_swap_twice.last = (obliges, collided, free)


def _double_swap_verdict():
    """The collision itself, asserted: in the same run in which the held parameters kept their blocks, the allocator did
    recycle a just-freed block (the control) and did put b on the old address of parameters nobody holds.  An allocator
    that does not recycle (caching off, another configuration) cannot show the hole: the test then skips, with that
    reason, after its comparison with the witness has passed."""
    obliges, collided, free = _data_swap_twice.last
    if not obliges:
        pytest.skip("the allocator did not hand a just-freed block back in the control: no address collision can be made "
                    "here, so the double swap shows nothing about the pin (the comparison with the witness passed)")
    if free:
        assert collided, "the allocator recycles freed blocks, yet none of the %d unheld parameters got its old address back" % free


def _cpu_round_trip(m):
    m.cpu()
    _no_grad_mul(m)
    m.cuda()


def _data_mul_then_public_call(m):
    import edgedict_amd
    for p in m.parameters():
        p.data.mul_(0.5)
    edgedict_amd.weights_changed()


def _fused_available():
    try:
        torch.optim.Adam([nn.Parameter(torch.zeros(1, device="cuda"))], fused=True)
        return True
    except (RuntimeError, TypeError, ValueError):
        return False


ROUTES = {
    "sgd": _torch_optim(lambda ps: torch.optim.SGD(ps, lr=0.05)),
    "adam": _torch_optim(lambda ps: torch.optim.Adam(ps, lr=3e-3)),
    "adam_foreach": _torch_optim(lambda ps: torch.optim.Adam(ps, lr=3e-3, foreach=True)),
    "adam_fused": _torch_optim(lambda ps: torch.optim.Adam(ps, lr=3e-3, fused=True)),
    "no_grad_mul_": _no_grad_mul,
    "load_state_dict": _load_state_dict,
    "load_state_dict_assign": _load_state_dict_assign,
    "new_parameters": _new_parameters,
    "data_swap": _data_swap,
    "data_swap_lstm_biases": _data_swap_lstm_biases,
    "data_swap_twice": _data_swap_twice,
    "cpu_round_trip": _cpu_round_trip,
    "data_mul_then_weights_changed": _data_mul_then_public_call,
}


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_way_of_changing_a_weight_reaches_the_kernels(hip_lib, dtype, route):
    if route == "adam_fused" and not _fused_available():
        pytest.skip("this torch build has no fused Adam for device tensors")
    m = _plain_model(dtype)
    inp = _inputs()
    warm = _use(m, inp)
    ROUTES[route](m)
    _check_against_witness(m, inp, dtype, warm, route)
    gc.collect()
    if route == "data_swap_twice":
        _double_swap_verdict()


@pytest.mark.parametrize("route", ["data_swap_twice", "adam_fused", "data_mul_then_weights_changed"])
def test_bound_chunk_plan_is_rebuilt(hip_lib, route):
    """The streaming decoder's pre-bound plan holds raw pointers to images: the routes no version counter shows must
    rebuild it too (its signature compares addresses, and it holds the tensors those were read from)."""
    from edgedict_amd.stream import BatchedStreamDecoder, chunk_geometry
    if route == "adam_fused" and not _fused_available():
        pytest.skip("this torch build has no fused Adam for device tensors")
    fl = C.flags()
    m = _plain_model("bf16")
    with torch.no_grad():
        m.joint.joint[2].bias[0] -= 1.0                  # (fewer blanks: the tokens have something to say)
    _use(m, _inputs())                                   # gradients for the optimiser route; every training-side image
    win, hop = chunk_geometry(fl, 2)
    wave = (0.1 * torch.randn(4, win + 2 * hop, generator=torch.Generator().manual_seed(7))).cuda()
    chunk = lambda c: wave[:, c * hop:c * hop + win].contiguous()      # noqa: E731
    dec = BatchedStreamDecoder(m, fl, 4, dither=0)
    dec.decode(chunk(0))
    plan0 = dec._plan
    assert plan0 is not None and plan0.ok
    dec.decode(chunk(1))
    assert dec._plan is plan0
    if route == "data_swap_twice":
        _data_swap_twice(m, plan0.pinned)               # the plan holds every parameter's tensor: none may collide
        assert _data_swap_twice.last[1:] == ([], 0), _data_swap_twice.last
    else:
        ROUTES[route](m)
    dec.reset()
    toks = dec.decode(chunk(2)).cpu()
    assert dec._plan is not plan0 and dec._plan.ok
    w = C.transducer(C.snapshot(m), fl, "bf16", train=False)
    wdec = BatchedStreamDecoder(w, fl, 4, dither=0)
    assert torch.equal(toks, wdec.decode(chunk(2)).cpu())
    torch.cuda.synchronize()
    if route == "data_swap_twice":
        _double_swap_verdict()


@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_adam_step_on_a_plain_model(hip_lib, dtype):
    from edgedict_amd.optim import FusedAdam
    m = _plain_model(dtype)
    opt = FusedAdam(m, lr=3e-3)
    grads = lambda: C.flat_grads(opt.flat)                                   # noqa: E731
    inp = _inputs()
    opt.zero_grad()
    warm = _use(m, inp, grads)
    opt.step()
    opt.zero_grad()
    _check_against_witness(m, inp, dtype, warm, "FusedAdam.step", grads)


def test_switching_the_compute_dtype_around_a_change(hip_lib):
    m = _plain_model("bf16")
    inp = _inputs()
    warm16 = _use(m, inp)
    m.compute_dtype = "fp32"
    warm32 = _use(m, inp)
    m.compute_dtype = "bf16"
    _use(m, inp)
    m.compute_dtype = "fp32"
    _no_grad_mul(m)                                                          # the change, seen in fp32 mode first
    _check_against_witness(m, inp, "fp32", warm32, "fp32 after the change")
    m.compute_dtype = "bf16"                                                 # the bf16 images are from before it
    _check_against_witness(m, inp, "bf16", warm16, "bf16 after the change")


@pytest.mark.parametrize("dtype", DTYPES)
def test_train_engine_load(hip_lib, tmp_path, dtype):
    eng = _engine(C.flags(), dtype)
    b = _batches(1)[0]
    eng.train_step(*b)
    xs, xlen = eng.features(b[0], b[1])
    inp = (xs, b[2], xlen, b[3])
    grads = lambda: C.flat_grads(eng.flat)                                   # noqa: E731
    eng.optim.zero_grad()
    warm = _use(eng.model, inp, grads)
    path = str(tmp_path / "half.pt")
    torch.save({"model": {k: v * 0.5 for k, v in C.snapshot(eng.model).items()}}, path)
    eng.load(path, load_optim=False)
    eng.optim.zero_grad()
    _check_against_witness(eng.model, inp, dtype, warm, "TrainEngine.load", grads)
    eng.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_lm_trainer_load(hip_lib, tmp_path, dtype):
    cfg = LM_CFG[True]
    tr = _lm_trainer(cfg, dtype)
    inputs, targets = _lm_batch(40)
    tr.train_step(inputs, targets)
    tr.model.eval()
    toks = torch.randint(2, C.V, (3, 6), generator=torch.Generator().manual_seed(0)).cuda()
    lens = torch.tensor([6, 4, 5])
    warm_score = tr.model.score(toks, lens).cpu()
    tr.model.train()
    path = str(tmp_path / "half_lm.pt")
    torch.save({k: v * 0.5 for k, v in C.snapshot(tr.model).items()}, path)
    tr.load(path)
    tr.optimizer.zero_grad()
    got_loss, _ = tr.model.loss(inputs, targets, None, ignore_index=0, reduction="mean")
    got_loss.backward()
    torch.cuda.synchronize()
    got = C.flat_grads(tr.optimizer.flat)
    w = C.lm(C.snapshot(tr.model), cfg, dtype)
    want_loss, want = C.lm_loss_and_grads(w, inputs, targets)
    assert got_loss.item() == want_loss
    C.assert_same_grads(_lm_names(tr), got, want, "LMTrainer.load:")
    tr.model.eval()
    w.eval()
    score = tr.model.score(toks, lens).cpu()
    assert torch.equal(score, w.score(toks, lens).cpu()) and not torch.equal(score, warm_score)
