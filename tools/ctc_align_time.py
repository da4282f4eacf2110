"""Time of the CTC forced aligner on the bench batch (one run, not a gate):

    python tools/ctc_align_time.py [--runs 3] [--warmup 2]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/ctc_align_time.py --profile 5

The bench's model and batch (bench.py's preset E6D2, 64 utterances of 15 s, 32 .. 64 labels each; seeded random
weights) with a CTC head, in bf16, eval mode.  Three model-level calls, each INCLUDING the encoder, alternate in one
process: `Transducer.ctc_align` (encoder, head, row pass, Viterbi walk, back-trace), `Transducer.align` (encoder,
prediction network, packed joint, RNN-T Viterbi) and `Transducer.ctc_greedy_decode` (encoder, head, arg max, collapse,
one read to the host).  Beside them, on the head logits of that batch alone: `loss.ctc_align` against the forward of
`loss.CTCLoss` (the same row pass, two walks and the label chain instead of one walk and the back-trace).  Device
events around every call, a synchronize between calls; prints the median (min .. max) of --runs alternating runs.
--profile N runs N `loss.ctc_align` calls and nothing else: the run to put under rocprofv3, whose kernel statistics
split the call into ctc_lse_gather / ctc_alpha_beta / ctc_viterbi_backtrace."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def _stats(ms):
    ms = sorted(ms)
    return ms[len(ms) // 2], ms[0], ms[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--preset", default="E6D2")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=15.0)
    ap.add_argument("--labels", type=int, default=64)
    ap.add_argument("--profile", type=int, default=0, metavar="N", help="N loss.ctc_align calls only (for rocprofv3)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ctc_align_time: needs the GPU (a CPU run measures nothing)")
    from bench import synth_batch
    from edgedict_amd.features import StackedLogFbank
    from edgedict_amd.flags import make_flags, model_kwargs
    from edgedict_amd.loss import CTCLoss, ctc_align
    from edgedict_amd.models import Transducer
    dev = torch.device("cuda", 0)
    flags = make_flags(args.preset, gradclip=None, dither=1e-5)
    wave, wave_len, ys, ylen = synth_batch(flags, args.batch, args.seconds, args.labels, 1000, dev)
    fb = StackedLogFbank(n_frame=flags.downsample, pad_to_divisible=True, out_dtype=torch.float32,
                         sample_rate=getattr(flags, "sample_rate", 16000), win_length=flags.win_length,
                         hop_length=flags.hop_length, n_fft=flags.n_fft, n_filt=flags.feature_size, dither=0.0).to(dev)
    torch.manual_seed(0)
    m = Transducer(**model_kwargs(flags, vocab_size=flags.bpe_size), ctc_weight=0.3).to(dev).eval()
    m.compute_dtype = "bf16"
    with torch.no_grad():
        xs, xlen = fb(wave, wave_len)
        h_enc, _ = m.encoder(xs[:, :int(xlen.max())].contiguous())
        act = m.scale_length(h_enc, xlen).to(device=dev, dtype=torch.int32).contiguous()
        logits = m._ctc_logits(h_enc).contiguous()
    lab = ylen.to(device=dev, dtype=torch.int32).contiguous()
    labels = ys[:, :int(ylen.max())].to(torch.int32).contiguous()
    loss_fn = CTCLoss(blank=m.blank, reduction="none", check_lengths=False)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        with torch.no_grad():
            out = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), out

    calls = [
        ("Transducer.ctc_align       ", lambda: m.ctc_align(xs, ys, xlen, ylen)),
        ("Transducer.align           ", lambda: m.align(xs, ys, xlen, ylen)),
        ("Transducer.ctc_greedy_decode", lambda: m.ctc_greedy_decode(xs, xlen)),
        ("loss.ctc_align (logits)    ", lambda: ctc_align(logits, labels, act, lab, m.blank, check_lengths=False)),
        ("loss.CTCLoss fwd (logits)  ", lambda: loss_fn(logits, labels, act, lab)),
    ]
    if args.profile:
        for _ in range(args.profile):
            timed(calls[3][1])
        return
    for _ in range(args.warmup):
        for _, fn in calls:
            timed(fn)
    ms = [[] for _ in calls]
    outs = [None] * len(calls)
    for _ in range(args.runs):
        for i, (_, fn) in enumerate(calls):
            t, outs[i] = timed(fn)
            ms[i].append(t)
    frames, ends, scores = outs[0]
    rf = outs[1][0]
    live = frames >= 0
    print("%s, batch %d x %.0f s, bf16: head logits %s, labels %d .. %d, CTC paths on %d / %d rows, label spans %.2f "
          "frames on average" % (args.preset, args.batch, args.seconds, list(logits.shape), int(ylen.min()),
                                 int(ylen.max()), int(torch.isfinite(scores).sum()), args.batch,
                                 (ends - frames + 1)[live].double().mean().item() if live.any() else float("nan")))
    print("mean |ctc frame - rnnt frame| on this random model: %.1f frames (no claim: there is no corpus)"
          % (frames - rf)[live & (rf >= 0)].abs().double().mean().item())
    for (name, _), t in zip(calls, ms):
        print("%s: %.3f ms per batch (%.3f .. %.3f)" % ((name,) + _stats(t)))
    print("median of %d alternating runs in one process, not a gate" % args.runs)


if __name__ == "__main__":
    main()
