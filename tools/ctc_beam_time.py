"""Time of the CTC prefix beam search on the bench shape's head logits (one run, not a gate):

    python tools/ctc_beam_time.py [--reps 20] [--warmup 5] [--W 10] [--cand N]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/ctc_beam_time.py --profile 5

The bench step (E6D2, bf16, 64 utterances of 15 s) hands the CTC head 64 x 201 frames; the logits here are synthetic at
that shape, [64, 201, 2048] bf16 drawn as the tests draw theirs (3 x normal, the blank raised by 2; full lengths): the
search reads nothing but the logits, and its time depends on their values only through how often a candidate merges.
Device events around `loss.ctc_prefix_beam` (row pass + walk + read-out, no host sync inside) and around
`loss.ctc_greedy` on the same logits, a synchronize between calls.  Prints the median (min .. max) of both, the whole
call's time divided by the frames (row pass and read-out included: the walk's own share comes from the rocprofv3 run
below), and beside them the RNN-T beam search's recorded 142 ms per batch at W = 10 (section 4.32).
--profile N runs N searches and nothing else: the run to put under rocprofv3, whose kernel statistics split the call
into ctc_beam_rows / ctc_beam_walk / ctc_beam_readout."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

RNNT_BEAM_MS = 142.0   # beam_search_batch, W = 10, the same batch


def _stats(ms):
    ms = sorted(ms)
    return ms[len(ms) // 2], ms[0], ms[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=201)
    ap.add_argument("--vocab", type=int, default=2048)
    ap.add_argument("--W", type=int, default=10)
    ap.add_argument("--cand", type=int, default=None)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--profile", type=int, default=0, metavar="N", help="N searches only (for rocprofv3)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ctc_beam_time: needs the GPU (a CPU run measures nothing)")
    from edgedict_amd.loss import ctc_greedy, ctc_prefix_beam
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(0)
    z = 3.0 * torch.randn(args.batch, args.frames, args.vocab, generator=g)
    z[:, :, 0] += 2.0
    z = z.to(dev).to(torch.bfloat16 if args.dtype == "bf16" else torch.float32).contiguous()
    act = torch.full((args.batch,), args.frames, dtype=torch.int32, device=dev)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), out

    beam = lambda: ctc_prefix_beam(z, act, W=args.W, cand=args.cand)
    greedy = lambda: ctc_greedy(z, act)
    if args.profile:
        for _ in range(args.profile):
            timed(beam)
        return
    for _ in range(args.warmup):
        timed(beam)
        timed(greedy)
    tb, tg = [], []
    for _ in range(args.reps):
        ms, out = timed(beam)
        tb.append(ms)
        ms, gout = timed(greedy)
        tg.append(ms)
    cand = min(args.vocab - 1, 32) if args.cand is None else args.cand
    mb, mg = _stats(tb), _stats(tg)
    ntok, nhyp = out[3], out[4]
    print("logits [%d, %d, %d] %s, W = %d, cand = %d: n_hyp %d .. %d, top-1 tokens %d .. %d (greedy %d .. %d)"
          % (args.batch, args.frames, args.vocab, args.dtype, args.W, cand, int(nhyp.min()), int(nhyp.max()),
             int(ntok[:, 0].min()), int(ntok[:, 0].max()), int(gout[1].min()), int(gout[1].max())))
    print("ctc_prefix_beam: %.3f ms per batch (%.3f .. %.3f), whole call / frames = %.2f us (rows + walk + read-out)"
          % (mb + (1e3 * mb[0] / args.frames,)))
    print("ctc_greedy     : %.3f ms per batch (%.3f .. %.3f)" % mg)
    print("RNN-T beam search, W = 10, recorded (section 4.32): %.0f ms per batch" % RNNT_BEAM_MS)
    print("one run of %d alternating calls each, not a gate" % args.reps)


if __name__ == "__main__":
    main()
