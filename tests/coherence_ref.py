"""The witness of tests/test_weight_coherence_gpu.py: a model rebuilt from a ``state_dict`` snapshot.

Not an oracle - it runs the same kernels as the model under test, on the same inputs.  It is built from CPU clones of the
masters into NEW ``Parameter`` objects, so every image it reads (casts, transposes, packed LSTM images) is built from the
snapshot at that moment, under cache keys of its own; nothing here clears ``models.WEIGHTS`` or the encoder stack's packed
images, which would refresh the model under test and hide exactly what is being looked for.  An image on the tested side
that does not follow its master is then the only way for the two to differ."""
import types

import torch

V = 40


def flags(**over):
    """The geometry of tests/test_train_step_gpu.py (encoder 3 x 64, prediction network 2 x 32; 1 s of audio is 34 stacked
    frames >= STACK_MIN_FRAMES; H = 64, B <= 64 selects the launch-persistent forward and the split-K BPTT in bf16), lr 3e-3."""
    d = dict(downsample=3, win_length=320, hop_length=160, n_fft=512, feature_size=80, dither=0.0,
             sample_rate=16000, lr=3e-3, gradclip=None, sub_batch_size=None, bpe_size=V,
             vocab_embed_size=8, enc_hidden_size=64, enc_layers=3, enc_dropout=0.0, enc_proj_size=24,
             dec_hidden_size=32, dec_layers=2, dec_dropout=0.0, dec_proj_size=16, joint_size=32,
             enc_time_reductions=[1], delta=False)
    d.update(over)
    return types.SimpleNamespace(**d)


def snapshot(module):
    """CPU clones of the module's state dict (reading them waits for everything enqueued so far)."""
    return {k: v.detach().cpu().clone() for k, v in module.state_dict().items()}


def transducer(sd, fl, dtype, train=True):
    from edgedict_amd.flags import model_kwargs
    from edgedict_amd.models import Transducer
    m = Transducer(**model_kwargs(fl, vocab_size=V), ctc_weight=getattr(fl, "ctc_weight", 0.0))
    m.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
    m = m.cuda()
    m.compute_dtype = dtype
    return m.train(train)


def lm(sd, cfg, dtype, train=True):
    from edgedict_amd.lm import LMModel
    m = LMModel(*cfg["args"], dropout=0.0, tie_weights=cfg["tied"])
    m.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
    m = m.cuda()
    m.compute_dtype = dtype
    return m.train(train)


def loss_and_grads(model, slices):
    """forward + backward over ``slices`` (a list of (xs, ys, xlen, ylen)), each slice's loss divided by their number as
    TrainEngine.train_step does: (loss as a float, [gradient per parameter, in parameters() order])."""
    total = None
    for xs, ys, xlen, ylen in slices:
        loss = model(xs, ys, xlen, ylen) / len(slices)
        loss.backward()
        total = loss.detach() if total is None else total + loss.detach()
    torch.cuda.synchronize()
    return total.item(), [p.grad.detach().clone() for p in model.parameters()]


def lm_loss_and_grads(model, inputs, targets):
    loss, _ = model.loss(inputs, targets, None, ignore_index=0, reduction="mean")
    loss.backward()
    torch.cuda.synchronize()
    return loss.item(), [p.grad.detach().clone() for p in model.parameters()]


def flat_grads(flat):
    """The flat gradient buffer cut back into per-parameter clones (FlatParams.offsets)."""
    return [flat.grad[off:off + p.numel()].view_as(p).clone() for p, off in zip(flat.params, flat.offsets)]


# the project's bound for two schedules of the same fp32 sums (atomics reorder them): tests/test_train_step_gpu.py
GRAD_RTOL = 2e-5


def grad_bound(grads):
    return GRAD_RTOL * max(g.abs().max().item() for g in grads)


def max_grad_diff(a, b):
    assert len(a) == len(b)
    return max((x.double() - y.double()).abs().max().item() for x, y in zip(a, b))


def assert_same_grads(names, got, want, what=""):
    """Every parameter's gradient within the bound - per parameter, so that a failure names the tensor."""
    assert len(names) == len(got) == len(want)
    bound = grad_bound(want)
    bad = []
    for n, g, w in zip(names, got, want):
        assert g.shape == w.shape, n
        d = (g.double() - w.double()).abs().max().item()
        if not d <= bound:
            bad.append("%s: %.3e" % (n, d))
    assert not bad, "%s gradients off by more than %.3e (= %g x max|g|): %s" % (what, bound, GRAD_RTOL, "; ".join(bad))
