"""Time of LM training at the reference's size (one run, not a gate):

    python tools/lm_train_time.py [--reps 30] [--warmup 5] [--dtype bf16 fp32]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/lm_train_time.py --profile 5

`LMModel(1024, 64, 1024, 2)` at batch 256, T = 64 (cli/train_lm.py:47,62), synthetic tokens (about a fifth of the targets
are the padding 0: ragged sentence ends), per compute dtype:

  * the full `LMTrainer.train_step` in tokens/s, with its phases bracketed by `ops.timed` (forward through the loss,
    backward, optimiser step; the LSTM blocks' own tags come with them);
  * on the step's logits shape, [16384, 1024] in that dtype, forward plus backward of
      - the fused loss (`loss.SoftmaxNLLLoss(ignore_index=0)`: two kernels and the one-workgroup reduction),
      - the composed form (`LMModel.forward`'s row log-softmax autograd function + `torch.nn.NLLLoss`),
      - `torch.nn.functional.cross_entropy` on the same device tensor,
    alternating the three in one loop, device events around each pair, a fresh copy of the logits per call (the fused
    pair consumes them; the copy is outside the events), a synchronize between calls.  Each API gets the target dtype
    it takes natively (int32 here, int64 for torch: an int64 tensor costs the fused path one cast kernel more).
    Timed twice: "queued" - the events and the pair are enqueued behind a ~1.5 ms blocker (three copies of a 1 GiB
    buffer), so the device finds the whole pair waiting and the figure is the device's time for it, launch gaps
    included - and "eager" - on an idle device, where at ~40 us of kernels the figure is the host's enqueue time and
    moves with whatever else the host is doing;
  * a plain device copy of the logits (`dst.copy_(src)`, one read + one write) for the copy rate at this size.

Prints the median (min .. max) of each and the fused pair's bytes/s (2 reads + 1 write of the logits).
--profile N [--kind fused|composed|torch] runs N pairs of one kind in bf16 and nothing else: the run to put under
rocprofv3, whose kernel statistics give the pair's kernel time."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

NTOKEN, NINP, NHID, NLAYERS, BATCH, T = 1024, 64, 1024, 2, 256, 64


def _stats(ms):
    ms = sorted(ms)
    return ms[len(ms) // 2], ms[0], ms[-1]


_BLOCKER = []


def _block():
    """~1.5 ms of device work in three launches: what follows is enqueued while the device is busy."""
    if not _BLOCKER:
        _BLOCKER.append(torch.empty(1 << 28, dtype=torch.float32, device="cuda"))
        _BLOCKER.append(torch.empty(1 << 28, dtype=torch.float32, device="cuda"))
    for _ in range(3):
        _BLOCKER[1].copy_(_BLOCKER[0])


def _event_ms(fn, queued=False):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if queued:
        _block()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def _batch(dev):
    g = torch.Generator(device="cpu").manual_seed(0)
    targets = torch.randint(2, NTOKEN, (BATCH, T), generator=g)
    lens = torch.randint(T // 2, T + 1, (BATCH,), generator=g)
    lens[0] = T
    targets[torch.arange(T)[None, :] >= lens[:, None]] = 0
    inputs = torch.cat([torch.ones(BATCH, 1, dtype=torch.long), targets], 1)[:, :-1]
    return inputs.to(dev), targets.to(dev)


def loss_pairs(dtype, targets, reps, warmup):
    from edgedict_amd.lm import _LogSoftmaxRowsFn
    from edgedict_amd.loss import SoftmaxNLLLoss
    dev = targets.device
    g = torch.Generator(device="cpu").manual_seed(1)
    master = (3.0 * torch.randn(BATCH * T, NTOKEN, generator=g)).to(dev).to(dtype)
    flat = targets.reshape(-1)
    flat32 = flat.int()
    fused_fn = SoftmaxNLLLoss(ignore_index=0)
    nll = torch.nn.NLLLoss(ignore_index=0)

    def pair(kind, queued):
        z = master.clone().requires_grad_(True)

        def run():
            if kind == "fused":
                loss = fused_fn(z, flat32)
            elif kind == "composed":
                loss = nll(_LogSoftmaxRowsFn.apply(z), flat)
            else:
                loss = torch.nn.functional.cross_entropy(z, flat, ignore_index=0)
            loss.backward()
        return _event_ms(run, queued)

    dst = torch.empty_like(master)
    kinds = ("fused", "composed", "torch")
    out = {k: [] for k in kinds + tuple(k + "_eager" for k in kinds) + ("copy",)}
    for i in range(warmup + reps):
        for queued in (True, False):
            for k in kinds:
                ms = pair(k, queued)
                if i >= warmup:
                    out[k if queued else k + "_eager"].append(ms)
        ms = _event_ms(lambda: dst.copy_(master), True)
        if i >= warmup:
            out["copy"].append(ms)
    return out, master.numel() * master.element_size()


def full_step(dtype, inputs, targets, reps, warmup):
    from edgedict_amd import ops
    from edgedict_amd.lm import LMModel, LMTrainer
    torch.manual_seed(0)
    lm = LMModel(NTOKEN, NINP, NHID, NLAYERS).cuda()
    tr = LMTrainer(lm, dtype=dtype)
    for _ in range(warmup):
        tr.train_step(inputs, targets)
    torch.cuda.synchronize()
    whole = [_event_ms(lambda: tr.train_step(inputs, targets)) for _ in range(reps)]
    # the phases, in a run of their own (the brackets are extra events)
    ops.TIMERS = {}
    try:
        for _ in range(max(3, reps // 3)):
            lm.train()
            tr.optimizer.zero_grad()
            with ops.timed("lm_forward_and_loss"):
                loss, _ = lm.loss(inputs, targets)
            with ops.timed("lm_backward"):
                loss.backward()
            with ops.timed("lm_optimizer_step"):
                tr.optimizer.step()
        torch.cuda.synchronize()
        phases = ops.timer_summary()
    finally:
        ops.TIMERS = None
    return whole, phases, float(loss.detach())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dtype", nargs="+", default=["bf16", "fp32"], choices=["bf16", "fp32"])
    ap.add_argument("--profile", type=int, default=0, metavar="N", help="N loss pairs only (for rocprofv3)")
    ap.add_argument("--kind", default="fused", choices=["fused", "composed", "torch"], help="the pair --profile runs")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lm_train_time: needs the GPU (a CPU run measures nothing)")
    dev = torch.device("cuda", 0)
    inputs, targets = _batch(dev)
    if args.profile:
        from edgedict_amd.lm import _LogSoftmaxRowsFn
        from edgedict_amd.loss import SoftmaxNLLLoss
        master = (3.0 * torch.randn(BATCH * T, NTOKEN)).to(dev).to(torch.bfloat16)
        flat = targets.reshape(-1)
        flat32 = flat.int()
        for _ in range(args.profile):
            z = master.clone().requires_grad_(True)
            if args.kind == "fused":
                SoftmaxNLLLoss(ignore_index=0)(z, flat32).backward()
            elif args.kind == "composed":
                torch.nn.NLLLoss(ignore_index=0)(_LogSoftmaxRowsFn.apply(z), flat).backward()
            else:
                torch.nn.functional.cross_entropy(z, flat, ignore_index=0).backward()
        torch.cuda.synchronize()
        return
    valid = int((targets != 0).sum())
    print("LMModel(%d, %d, %d, %d), batch %d x T %d = %d tokens per step (%d not padding)"
          % (NTOKEN, NINP, NHID, NLAYERS, BATCH, T, BATCH * T, valid))
    for name in args.dtype:
        dtype = torch.bfloat16 if name == "bf16" else torch.float32
        whole, phases, last = full_step(name, inputs, targets, args.reps, args.warmup)
        med = _stats(whole)
        print("[%s] train_step: %.3f ms (%.3f .. %.3f) = %.0f tokens/s; last loss %.4f"
              % ((name,) + med + (1e3 * BATCH * T / med[0], last)))
        for tag in sorted(phases):
            print("[%s]   %-28s x%-3d mean %.3f ms" % (name, tag, phases[tag][0], phases[tag][1]))
        pairs, nbytes = loss_pairs(dtype, targets, args.reps, args.warmup)
        for k in ("fused", "composed", "torch"):
            print("[%s] loss forward + backward on [%d, %d], %-8s: queued %.4f ms (%.4f .. %.4f), eager %.4f ms "
                  "(%.4f .. %.4f)" % ((name, BATCH * T, NTOKEN, k) + _stats(pairs[k]) + _stats(pairs[k + "_eager"])))
        f, c, t = _stats(pairs["fused"]), _stats(pairs["copy"]), _stats(pairs["torch"])
        print("[%s] fused / torch = %.3f queued, %.3f eager; fused pair moves 3 x %.1f MB: %.2f TB/s; device copy (2 x %.1f MB) %.4f ms "
              "(%.4f .. %.4f) = %.2f TB/s" % (name, f[0] / t[0],
                                              _stats(pairs["fused_eager"])[0] / _stats(pairs["torch_eager"])[0],
                                              nbytes / 1e6, 3 * nbytes / f[0] / 1e9, nbytes / 1e6,
                                              c[0], c[1], c[2], 2 * nbytes / c[0] / 1e9))
    print("one run of %d alternating calls each, not a gate" % args.reps)


if __name__ == "__main__":
    main()
