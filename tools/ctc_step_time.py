"""Cost of the CTC auxiliary head in the training step: the bench-shaped step (bench.py's
preset, batch and synthetic input; bf16) at ctc_weight = 0.3 against ctc_weight = 0 on ONE engine of one build:

    python tools/ctc_step_time.py [--reps 20] [--warmup 5]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/ctc_step_time.py --profile 5

The engine is built with the head (its two tensors sit in the flat buffer in both modes); `model.ctc_weight` is a plain
attribute, so the two modes alternate step by step in one process: at 0 forward() launches what a model without the head
launches.  Device events around train_step, a synchronize between steps.  Prints the median (min .. max) of each mode
and the difference of the medians.  --profile N runs N steps at 0.3 and nothing else: the run to put under rocprofv3,
whose kernel statistics then hold the ctc_* kernels' times."""
import argparse
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def _stats(ms):
    ms = sorted(ms)
    return ms[len(ms) // 2], ms[0], ms[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--weight", type=float, default=0.3)
    ap.add_argument("--preset", default="E6D2")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=15.0)
    ap.add_argument("--labels", type=int, default=64)
    ap.add_argument("--profile", type=int, default=0, metavar="N", help="N steps at --weight only (for rocprofv3)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ctc_step_time: needs the GPU (a CPU run measures nothing)")
    from bench import synth_batch
    from edgedict_amd import side
    from edgedict_amd.flags import make_flags
    from edgedict_amd.trainer import TrainEngine
    device = torch.device("cuda", 0)
    side.stream(device)
    flags = make_flags(args.preset, gradclip=None, dither=1e-5)
    flags.sub_batch_size = args.batch
    flags.ctc_weight = args.weight
    torch.manual_seed(0)
    random.seed(0)
    engine = TrainEngine(flags, device=device, compute_dtype="bf16")
    batch = synth_batch(flags, args.batch, args.seconds, args.labels, 1000, device)
    nxt = (batch[0], batch[1])

    def step(w):
        engine.model.ctc_weight = w
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        loss = engine.train_step(*batch, next_batch=nxt)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), loss

    try:
        if args.profile:
            for _ in range(args.profile):
                step(args.weight)
            return
        for _ in range(args.warmup):
            step(args.weight)
            step(0.0)
        on, off = [], []
        for _ in range(args.reps):
            ms, loss = step(args.weight)
            on.append(ms)
            parts = engine.model.loss_parts
            ms, _ = step(0.0)
            off.append(ms)
        print("loss %.4f = rnnt %.4f + %g x ctc %.4f" % (loss.item(), parts[0].item(), args.weight, parts[1].item()))
        m_on, m_off = _stats(on), _stats(off)
        print("step, ctc_weight = %g: %.3f ms (%.3f .. %.3f)" % ((args.weight,) + m_on))
        print("step, ctc_weight = 0: %.3f ms (%.3f .. %.3f)" % m_off)
        print("difference of the medians: %+.3f ms (%+.2f %%), %d alternating steps each"
              % (m_on[0] - m_off[0], 100.0 * (m_on[0] - m_off[0]) / m_off[0], args.reps))
    finally:
        engine.close()


if __name__ == "__main__":
    main()
