"""Cost of an MWER step beside the plain training step: the bench-shaped batch (bench.py's preset,
batch and synthetic input; bf16) through TrainEngine.mwer_step at beam width W against TrainEngine.train_step on ONE
engine of one build, alternating step by step in one process:

    python tools/mwer_time.py [--reps 3] [--warmup 1] [-W 4]

Device events around each step, a synchronize between steps; prints the median (min .. max) of each and their ratio,
the lattice rows the MWER step materialised, the time of the risk kernel alone on the step's own [B, N] list (its two
launches, median of 200 calls), and the time of the encoder-row gather (``index_select`` of the [B, T, P] encoder output
to the R lattice rows) alone - the copy a shared-encoder joint kernel would avoid.  No threshold: this tool reports."""
import argparse
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def _stats(ms):
    ms = sorted(ms)
    return ms[len(ms) // 2], ms[0], ms[-1]


def _timed(fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return _stats(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("-W", type=int, default=4)
    ap.add_argument("--nll-weight", type=float, default=0.0)
    ap.add_argument("--search", default="sync_beam")
    ap.add_argument("--preset", default="E6D2")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=15.0)
    ap.add_argument("--labels", type=int, default=64)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mwer_time: needs the GPU (a CPU run measures nothing)")
    from bench import synth_batch
    from edgedict_amd import loss, ops, side
    from edgedict_amd.flags import make_flags
    from edgedict_amd.trainer import TrainEngine
    device = torch.device("cuda", 0)
    side.stream(device)
    flags = make_flags(args.preset, gradclip=None, dither=1e-5)
    flags.sub_batch_size = args.batch
    torch.manual_seed(0)
    random.seed(0)
    engine = TrainEngine(flags, device=device, compute_dtype="bf16")
    wave, wave_len, ys, ylen = synth_batch(flags, args.batch, args.seconds, args.labels, 1000, device)
    ys_host = ys.cpu()                       # the packer reads the references on the host

    def step(mwer):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        if mwer:
            out = engine.mwer_step(wave, wave_len, ys_host, ylen, W=args.W, nll_weight=args.nll_weight,
                                   search=args.search)
        else:
            out = engine.train_step(wave, wave_len, ys, ylen)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), out

    try:
        for _ in range(args.warmup):
            step(True)
            step(False)
        on, off = [], []
        for _ in range(args.reps):
            ms, mloss = step(True)
            on.append(ms)
            rows, last = ops.LAST["joint_rows"], engine.model.last_mwer
            ms, tloss = step(False)
            off.append(ms)
        m_on, m_off = _stats(on), _stats(off)
        n_hyp = last["n_hyp"].cpu()
        lens = [t.size for own in last["lists"] for t in own]
        print("mwer_step, W = %d (%s): %.3f ms (%.3f .. %.3f), loss %.4f" % ((args.W, args.search) + m_on + (mloss.item(),)))
        print("train_step: %.3f ms (%.3f .. %.3f), loss %.4f" % (m_off + (tloss.item(),)))
        print("ratio of the medians: %.2f, %d alternating steps each" % (m_on[0] / m_off[0], args.reps))
        print("last MWER step: %d hypotheses over %d utterances (N = %d), %d .. %d tokens each, %d lattice rows, mean risk %.3f"
              % (int(n_hyp.sum()), n_hyp.numel(), last["costs"].shape[1], min(lens), max(lens), rows,
                 last["risk"].mean().item()))
        costs, errs, nh = last["costs"].contiguous(), last["errors"], last["n_hyp"]
        k = _timed(lambda: loss.MWERLoss()(costs, errs, nh), 200)
        print("risk kernel alone (MWERLoss forward on [%d, %d]): %.4f ms (%.4f .. %.4f)" % (tuple(costs.shape) + k))
        # the gather alone: the encoder output's shape and dtype, the utterance of every lattice row
        T = engine.model.encoder.output_frames(engine.features.output_frames(wave.shape[1]))
        P = engine.model.joint.joint[0].weight.shape[1] - engine.model.decoder.proj.weight.shape[0]
        enc = torch.zeros(args.batch, T, P, dtype=torch.bfloat16, device=device)
        utt = torch.repeat_interleave(torch.arange(args.batch, dtype=torch.int32), n_hyp.long()).to(device)
        gth = _timed(lambda: enc.index_select(0, utt), 20)
        print("encoder-row gather alone ([%d, %d, %d] -> %d rows): %.3f ms (%.3f .. %.3f), %.1f %% of the MWER step"
              % (args.batch, T, P, utt.numel(), gth[0], gth[1], gth[2], 100.0 * gth[0] / m_on[0]))
    finally:
        engine.close()


if __name__ == "__main__":
    main()
