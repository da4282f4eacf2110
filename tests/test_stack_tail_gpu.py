"""GPU: the encoder stack's backward pass with EDGEDICT_STACK_TAIL's default (csrc/encoder_stack.hip: the bias column
sums of the two layers that finish last run on the side stream beside those layers' products) against
EDGEDICT_STACK_TAIL=0 (everything where it was before), in one process (``encoder_stack.tail_mode``).

The full stack, forward and backward through ``edgedict_stack_forward`` / ``edgedict_stack_backward``, on the smallest
shapes that reach every branch of the scheduler: 2 and 3 layers, with and without the 2x time reduction, H = 64 and 128
(one and two unit blocks), B = 3, 17, 64 (a partial 16-row tile, two tiles, four), T0 = chunk + 1 and 2 x chunk + 1 frames (a
single-chunk layer behind the reduction, a left-over frame), I0 = 40 (K % 64 != 0 in layer 0's products); gradients
returned and accumulated in place (ACCUM_GRADS), weight gradients after the BPTT (DW_AT_END), one stream (SERIAL), the
split-K and the launch-per-step BPTT, and a layer's weight gradients issued chunk by chunk (EDGEDICT_STACK_DW_SEG=1: the
first segment stores the gradient, the later ones add to it - those updates must stay in order on one stream, so the
bias gradients of such a layer do not move).

The default moves kernels between streams and gives two of them a scratch row of their own: no kernel, no input and the
program order within no sum changes.  So the outputs, the final states and every weight gradient (dW_ih, dW_hh: K slices
written once and summed in a fixed order) must be BIT-IDENTICAL to the =0 run, and two runs of the default to each other.

The LayerNorm parameter gradients (d_in_gamma, d_in_beta, every dgamma / dbeta) and the bias gradients end in fp32
atomicAdds of several workgroups (stack_sum_parts_kernel, stack_input_norm_bwd_kernel, colsum_kernel): the order in which
those arrive is not fixed, in the code before the switch either - two runs of =0 differ from each other in the last bits
(measured on an MI355X at these shapes, largest absolute difference per case: =0 against =0 2.4e-7 ... 4.8e-6, the default
against =0 2.4e-7 ... 5.7e-6, the default twice 2.4e-7 ... 3.8e-6 - the same last-bit scatter in all three, and it shows
in a layer's dgamma as well, whose kernels and stream this switch does not touch; the test prints the figure of every
case).  Bit identity is not a property these sums have, so they are held to the bound the existing stack tests state for
exactly these quantities when the same kernels run in another schedule: tests/test_encoder_stack_gpu.py:78-80,
|a - b| <= 1e-4 x max|a| for the names with "norm", "projs" or "bias".  On top of that the switch may add nothing to the
scatter the order before it has: default against =0 at most 4 x the case's largest =0-against-=0 difference plus 16
fp32 ulps of the gradient's largest value (the floor for a case whose two =0 runs happen to agree: re-ordering the <= 64
atomic contributions of an element moves it by a few ulps of the running sum; a lost or doubled update - a bias
gradient is a sum over B x T rows of order-one terms - is thousands of ulps).  b_ih and b_hh receive the same db through one
kernel launch: identical to each other, bit for bit, in every run."""
import pytest
import torch

pytestmark = pytest.mark.gpu

CHUNK = 4
# name: (B, T0, H, L, time_reductions (after these layers))
SHAPES = {
    "L2_H64_B3_T5": (3, CHUNK + 1, 64, 2, []),
    "L3_H128_B17_T9_red0": (17, 2 * CHUNK + 1, 128, 3, [0]),
    "L2_H128_B64_T9": (64, 2 * CHUNK + 1, 128, 2, []),
    "L3_H64_B64_T5_red1": (64, CHUNK + 1, 64, 3, [1]),
}
I0 = 40
MODES = ["returned", "accum", "dw_at_end", "serial", "launch_per_step", "dw_seg", "dw_seg_accum"]


def _encoder(shape, seed=0):
    from edgedict_amd.models import Encoder
    B, T0, H, L, red = shape
    torch.manual_seed(seed)
    enc = Encoder(input_size=I0, hidden_size=H, num_layers=L, dropout=0.0, proj_size=24, time_reductions=red)
    with torch.no_grad():   # non-trivial LayerNorm affine parameters
        for p in enc.parameters():
            if p.dim() == 1 and p.numel() in (I0, H):
                p.add_(0.3 * torch.randn_like(p))
    enc = enc.cuda()
    g = torch.Generator(device="cpu").manual_seed(seed + 1)
    xs = torch.randn(B, T0, I0, generator=g).cuda()
    return enc, xs


def _run(enc, xs, mode, tail):
    """One forward + backward under EDGEDICT_STACK_TAIL = tail (None: the default); (out, h, c, {name: grad})."""
    from edgedict_amd import config, encoder_stack as es
    old = (config.USE_ENCODER_STACK, es.CHUNK, es.LAG, es.FLAGS, es.SPLIT_K, config.STACK_MIN_FRAMES,
           config.DEFER_WEIGHT_GRADS)
    config.USE_ENCODER_STACK, config.STACK_MIN_FRAMES = True, 1        # tiny geometries on purpose
    es.CHUNK, es.LAG, es.SPLIT_K = CHUNK, 0, 1
    es.FLAGS = {"dw_at_end": es.DW_AT_END, "serial": es.SERIAL}.get(mode, 0)
    config.DEFER_WEIGHT_GRADS = True
    es.tail_mode(-1 if tail is None else tail)
    try:
        enc.compute_dtype = torch.bfloat16
        enc.zero_grad(set_to_none=True)
        ptrs = None
        if mode in ("accum", "dw_seg_accum"):          # the trainer's path: every parameter has a contiguous fp32 .grad, the pass adds into it
            for q in enc.parameters():
                i = torch.arange(q.numel(), device="cuda").view(q.shape)
                q.grad = 0.5 + 0.125 * ((i % 5) - 2).float()
            ptrs = [q.grad.data_ptr() for q in enc.parameters()]
        out, (h, c) = enc(xs)
        g = torch.Generator(device="cpu").manual_seed(5)
        w = torch.randn(out.shape, generator=g).cuda()
        (out.float() * w).sum().backward()
        torch.cuda.synchronize()
        es.check_wsr_error()
        assert es.last_mode(True)[0] == (0 if mode == "launch_per_step" else 2), es.last_mode(True)
        if ptrs is not None:
            assert [q.grad.data_ptr() for q in enc.parameters()] == ptrs, "the gradients were accumulated in place"
        grads = {n: p.grad.detach().clone() for n, p in enc.named_parameters()}
        return out.detach().float(), h.detach(), c.detach(), grads
    finally:
        es.tail_mode(-1)
        (config.USE_ENCODER_STACK, es.CHUNK, es.LAG, es.FLAGS, es.SPLIT_K, config.STACK_MIN_FRAMES,
         config.DEFER_WEIGHT_GRADS) = old


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_default_tail_computes_what_the_order_before_computed(hip_lib, monkeypatch, shape, mode):
    from edgedict_amd import encoder_stack as es
    monkeypatch.setenv("EDGEDICT_STACK_BWD_SK", "0" if mode == "launch_per_step" else "1")
    if mode.startswith("dw_seg"):
        monkeypatch.setenv("EDGEDICT_STACK_DW_SEG", "1")
    assert es.tail_mode() == 1, "the default setting is under test"
    enc, xs = _encoder(SHAPES[shape])
    ref = _run(enc, xs, mode, 0)
    ref2 = _run(enc, xs, mode, 0)
    got = _run(enc, xs, mode, None)
    again = _run(enc, xs, mode, None)
    L = SHAPES[shape][3]
    # the stack's parameters: the input norm's, and per layer both weights, both biases and the LayerNorm's (the output
    # projection `proj.*` behind the stack is another operator's gradient)
    names = sorted(n for n in ref[3] if not n.startswith("proj."))
    assert sum("bias_ih" in n or "bias_hh" in n for n in names) == 2 * L, names
    assert len(names) == 2 + 6 * L, names
    worst = {"=0 twice": 0.0}
    for tag, base, other in (("=0 twice", ref, ref2), ("default vs =0", ref, got), ("default twice", got, again)):
        for i, what in enumerate(("out", "h", "c")):
            assert torch.equal(base[i], other[i]), (tag, what)
        for n in names:
            a, b = base[3][n], other[3][n]
            d = (a - b).abs().max().item()
            assert torch.isfinite(b).all(), (tag, n)
            if "norm" in n or "projs" in n or "bias" in n:      # these end in fp32 atomics (test_encoder_stack_gpu.py:78-80)
                worst[tag] = max(worst.get(tag, 0.0), d)
                assert d <= 1e-4 * max(a.abs().max().item(), 1e-6), (tag, n, d)
                if tag != "=0 twice":
                    assert d <= 4.0 * worst["=0 twice"] + 16 * 2.0 ** -23 * a.abs().max().item(), (tag, n, d, worst)
            else:
                assert torch.equal(a, b), (tag, n, d)
    for run in (ref, got, again):
        for l in range(L):
            assert torch.equal(run[3]["lstm.lstms.%d.bias_ih_l0" % l], run[3]["lstm.lstms.%d.bias_hh_l0" % l]), l
    print("\n%s %s: largest |difference| of an atomically summed gradient %s" % (shape, mode, worst))
