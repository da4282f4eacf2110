"""GPU: a parameter frozen with ``requires_grad_(False)`` after FlatParams attached its flat ``.grad`` view gets no
gradient and is not reported to the data-parallel exchange, as with plain autograd; the trainable parameters' gradients
are those of the same step with nothing frozen.  The backward paths that accumulate weight gradients straight into an
existing fp32 ``.grad`` (LSTM blocks, Linear, the joint with and without the loss, the encoder stack) once chose that
path because ``.grad`` existed, without asking whether the parameter wanted a gradient."""
import pytest
import torch

from oracle import models_ref as M
from oracle import rnnt_loss_ref as R
from oracle.make_golden import CASES

pytestmark = pytest.mark.gpu

FROZEN = ("encoder.lstm.lstms.1.weight_ih_l0", "encoder.lstm.lstms.1.weight_hh_l0", "encoder.lstm.lstms.1.bias_ih_l0",
          "encoder.lstm.lstms.1.bias_hh_l0", "encoder.proj.weight", "encoder.proj.bias",
          "joint.joint.0.weight", "joint.joint.0.bias")


# the encoder stack only runs in bf16; lengths on the host take the packed joint + loss (_JointLossFn), on the device
# the dense joint (_JointFn) and the loss after it
@pytest.mark.parametrize("cd,stack", [("fp32", False), ("fp32", True), ("bf16", False), ("bf16", True)])
def test_frozen_parameters_get_no_gradient(hip_lib, cd, stack):
    from edgedict_amd import config, dp, optim
    from edgedict_amd.models import Transducer
    cfg, B, T0, U, seed = CASES["tiny"]
    sd = M.make_state_dict(cfg, seed)
    xs, ys, xlen, ylen = M.make_batch(cfg, seed + 1, B, T0, U)
    m = Transducer(enc_dropout=0.0, dec_dropout=0.0, output_loss=True, **cfg)
    m.load_state_dict(sd, strict=True)
    m = m.cuda()
    m.compute_dtype = cd
    flat = optim.FlatParams(m)                        # as TrainEngine does: every parameter owns a flat .grad view
    params = dict(m.named_parameters())
    packed = stack
    reported = []
    saved = (config.USE_ENCODER_STACK, config.STACK_MIN_FRAMES, dp.READY_HOOK)
    config.USE_ENCODER_STACK = stack
    config.STACK_MIN_FRAMES = 1 if stack else saved[1]
    dp.READY_HOOK = lambda ps, stream: reported.extend(id(p) for p in ps)

    def step():
        flat.zero_grad()
        del reported[:]
        loss = m(xs.cuda(), ys.cuda(), xlen if packed else xlen.cuda(), ylen if packed else ylen.cuda())
        loss.backward()
        torch.cuda.synchronize()
        return loss.item(), {n: p.grad.clone() for n, p in params.items()}

    try:
        loss_all, g_all = step()
        for n in FROZEN:
            params[n].requires_grad_(False)
        loss_frozen, g_frozen = step()
    finally:
        config.USE_ENCODER_STACK, config.STACK_MIN_FRAMES, dp.READY_HOOK = saved
        for n in FROZEN:
            params[n].requires_grad_(True)
    assert loss_frozen == loss_all
    for n in FROZEN:
        assert params[n].grad is not None and params[n].grad.data_ptr() != 0
        assert (g_frozen[n] == 0).all(), (n, g_frozen[n].abs().max().item())
        assert id(params[n]) not in reported, n
    for n, g in g_all.items():
        if n in FROZEN:
            continue
        # the same arithmetic; only the order of fp32 accumulation (split-K, atomics) may differ
        scale = max(g.abs().max().item(), 1e-8)
        assert (g_frozen[n] - g).abs().max().item() <= 1e-5 * scale, n
    if cd == "fp32":
        # and the oracle's gradients at test_models_gpu's bound
        sd64 = {k: v.double().requires_grad_(True) for k, v in sd.items()}
        logits, act_lens = M.transducer_logits(sd64, xs.double(), ys, xlen, ylen)
        costs, dlogits = R.rnnt_loss_torch_fast(logits.detach(), ys[:, :int(ylen.max())], act_lens, ylen)
        logits.backward(dlogits / B)
        for n, g in g_frozen.items():
            if n in FROZEN:
                continue
            ref = sd64[n].grad
            err = (g.double().cpu() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-6)
            assert err < 2e-3, (n, err)
