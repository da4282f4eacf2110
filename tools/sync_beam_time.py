"""Time of the frame-synchronous beam search beside the best-first search and the greedy search, on the bench's batch
(one run, not a gate):

    python tools/sync_beam_time.py [--reps 5] [--warmup 2] [--W 10]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/sync_beam_time.py --profile 3

The batch is bench.py's: E6D2, 64 utterances of 15 s, ragged lengths (`bench.synth_batch`, seed 1000), through the
bench's feature front-end, bf16; the model is the one bench.py times its beam search on - torch.manual_seed(0) weights
with the joint's blank bias raised by 12, so that the best-first search pops its minimum of W hypotheses per frame, as a
trained model does.  The three searches run on the same features; each call includes the encoder, as the public entry
points do.  Prints the median (min .. max) of the wall time around each call with a synchronize on both sides,
utterances/s, and for the frame-synchronous search the time per frame.  --profile N runs N frame-synchronous searches and
nothing else: the run to put under rocprofv3."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def _stats(ms):
    ms = sorted(ms)
    return ms[len(ms) // 2], ms[0], ms[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=15.0)
    ap.add_argument("--W", type=int, default=10)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--profile", type=int, default=0, metavar="N", help="N frame-synchronous searches only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sync_beam_time: needs the GPU (a CPU run measures nothing)")
    import bench
    from edgedict_amd import decode
    from edgedict_amd.features import StackedLogFbank
    from edgedict_amd.flags import make_flags, model_kwargs
    from edgedict_amd.models import Transducer
    dev = torch.device("cuda", 0)
    flags = make_flags("E6D2", gradclip=None, dither=1e-5)
    wave, wave_len, _, _ = bench.synth_batch(flags, args.batch, args.seconds, 64, 1000, dev)
    fb = StackedLogFbank(n_frame=flags.downsample, pad_to_divisible=True, out_dtype=torch.float32,
                         sample_rate=getattr(flags, "sample_rate", 16000), win_length=flags.win_length,
                         hop_length=flags.hop_length, n_fft=flags.n_fft, n_filt=flags.feature_size, dither=0.0).to(dev)
    torch.manual_seed(0)
    m = Transducer(**model_kwargs(flags, vocab_size=flags.bpe_size)).to(dev).eval()
    m.compute_dtype = args.dtype
    with torch.no_grad():
        m.joint.joint[2].bias[0] += 12.0
        xs, xlen = fb(wave, wave_len)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), out

    sync = lambda: m.sync_beam_search(xs, xlen, W=args.W)
    best_first = lambda: m.beam_search(xs, xlen, W=args.W)
    greedy = lambda: m.greedy_decode(xs, xlen)
    with torch.no_grad():
        if args.profile:
            for _ in range(args.profile):
                timed(sync)
            return
        for _ in range(args.warmup):
            timed(sync), timed(best_first), timed(greedy)
        ts, tb, tg = [], [], []
        for _ in range(args.reps):
            ms, (s_seqs, s_scores) = timed(sync)
            ts.append(ms)
            ms, (b_seqs, b_scores) = timed(best_first)
            tb.append(ms)
            ms, _ = timed(greedy)
            tg.append(ms)
        enc, _ = m.encoder(xs)
        frames = int(m.scale_length(enc, xlen.cpu()).max())
    B = args.batch
    same = sum(int(len(a) == len(b) and (a == b).all()) for a, b in zip(s_seqs, b_seqs))
    print("E6D2 %s, %d utterances of %.0f s, %d encoder frames at most, W = %d, V = %d"
          % (args.dtype, B, args.seconds, frames, args.W, flags.bpe_size))
    for name, t in (("sync_beam_search", ts), ("beam_search     ", tb), ("greedy_decode   ", tg)):
        med, lo, hi = _stats(t)
        print("%s: %8.2f ms per batch (%.2f .. %.2f)  %7.0f utterances/s" % (name, med, lo, hi, 1e3 * B / med))
    print("sync_beam_search: %.1f us per frame (whole call, encoder and read-out included)"
          % (1e3 * _stats(ts)[0] / max(1, frames)))
    print("best-first expansions of the last call: %d;  utterances with the same best tokens in both searches: %d of %d "
          "(different algorithms: equality is not expected)" % (decode.beam_search_batch.last_expansions, same, B))
    print("one run of %d alternating calls each, not a gate" % args.reps)


if __name__ == "__main__":
    main()
