"""Cost of internal-LM estimation (ILME, ``ilm_weight=``) in the frame-synchronous beam search, offline and streaming
(a measurement, not a gate):

    python tools/sync_ilme_time.py [--runs 3] [--warmup 2] [--W 10] [--streams 256] [--steps 100] [--part both]

Offline part: tools/sync_fusion_time.py's workload - the bench's E6D2 batch (64 utterances of 15 s, ragged lengths,
`bench.synth_batch` seed 1000) through the bench's feature front-end, bf16, torch.manual_seed(0) weights with the joint's
blank bias raised by 12 - searched with `Transducer.sync_beam_search` in four configurations, alternating inside a run:
plain; `lm=LMModel(V, 64, 1024, 2)` (random weights, lm_weight 0.3); that LM with `ilm_weight=0.2`; `ilm_weight=0.2`
alone.  Each call includes the encoder, as the public entry point does.  Prints median (min .. max) ms per batch,
utterances/s, the cost over plain, and ILME's cost over the same search without it.

Streaming part: tools/sync_stream_time.py's chunk step - `BatchedStreamSyncFusionBeamDecoder.decode(chunk)` for 256
streams, one encoder frame per chunk - for the same four configurations, `--steps` consecutive steps per run between two
synchronisations, every run from a reset (not timed).

The plain and the LM-only searches launch exactly what they launched before ILME existed, so they are the yardsticks of
the same process.  What the figures do not say: the weights are random, so nothing here is an accuracy or WER claim, and
ILME changes which hypotheses survive, so the searches compared do not hold the same beams."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def _stats(ms):
    ms = sorted(ms)
    return ms[len(ms) // 2], ms[0], ms[-1]


def _report(rows, unit, per_s=None):
    med = {name: _stats(t)[0] for name, t in rows}
    for name, t in rows:
        m, lo, hi = _stats(t)
        tail = "" if per_s is None else "  %7.0f utterances/s" % (1e3 * per_s / m)
        print("%-10s: %9.3f ms per %s (%.3f .. %.3f)%s  %+6.1f %% over plain"
              % (name, m, unit, lo, hi, tail, 100.0 * (m / med["plain"] - 1.0)))
    print("ILME's cost: %+.3f ms (%+.1f %%) on the plain search, %+.3f ms (%+.1f %%) on the LM-fused one"
          % (med["ilm"] - med["plain"], 100.0 * (med["ilm"] / med["plain"] - 1.0), med["lm + ilm"] - med["lm"],
             100.0 * (med["lm + ilm"] / med["lm"] - 1.0)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=15.0)
    ap.add_argument("--W", type=int, default=10)
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--ilm-weight", type=float, default=0.2)
    ap.add_argument("--part", default="both", choices=["offline", "stream", "both"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sync_ilme_time: needs the GPU (a CPU run measures nothing)")
    import bench
    from edgedict_amd.features import StackedLogFbank
    from edgedict_amd.flags import make_flags, model_kwargs
    from edgedict_amd.lm import LMModel
    from edgedict_amd.models import Transducer
    from edgedict_amd.stream import BatchedStreamSyncFusionBeamDecoder, chunk_geometry
    dev = torch.device("cuda", 0)
    flags = make_flags("E6D2", gradclip=None, dither=1e-5)
    V = flags.bpe_size
    torch.manual_seed(0)
    m = Transducer(**model_kwargs(flags, vocab_size=V)).to(dev).eval()
    m.compute_dtype = "bf16"
    with torch.no_grad():
        m.joint.joint[2].bias[0] += 12.0
    torch.manual_seed(1)
    lm = LMModel(V, 64, 1024, 2, dropout=0.0).to(dev).eval()
    lm.compute_dtype = "bf16"
    for p in lm.parameters():
        p.requires_grad_(False)
    fuse = dict(lm=lm, lm_weight=0.3, length_bonus=0.0)
    ilm = dict(ilm_weight=args.ilm_weight)
    configs = [("plain", {}), ("lm", fuse), ("lm + ilm", dict(fuse, **ilm)), ("ilm", ilm)]
    W = args.W

    if args.part in ("offline", "both"):
        wave, wave_len, _, _ = bench.synth_batch(flags, args.batch, args.seconds, 64, 1000, dev)
        fb = StackedLogFbank(n_frame=flags.downsample, pad_to_divisible=True, out_dtype=torch.float32,
                             sample_rate=getattr(flags, "sample_rate", 16000), win_length=flags.win_length,
                             hop_length=flags.hop_length, n_fft=flags.n_fft, n_filt=flags.feature_size,
                             dither=0.0).to(dev)
        with torch.no_grad():
            xs, xlen = fb(wave, wave_len)
            times = [[] for _ in configs]
            for rep in range(args.warmup + args.runs):
                for k, (_, kw) in enumerate(configs):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    m.sync_beam_search(xs, xlen, W=W, **kw)
                    torch.cuda.synchronize()
                    if rep >= args.warmup:
                        times[k].append(1e3 * (time.perf_counter() - t0))
            enc, _ = m.encoder(xs)
            frames = int(m.scale_length(enc, xlen.cpu()).max())
        print("offline: E6D2 bf16, %d utterances of %.0f s, %d encoder frames at most, W = %d, V = %d, LM 64/1024/2, "
              "ilm_weight %.2f, %d alternating runs" % (args.batch, args.seconds, frames, W, V, args.ilm_weight, args.runs))
        _report([(n, t) for (n, _), t in zip(configs, times)], "batch", per_s=args.batch)

    if args.part in ("stream", "both"):
        S = args.streams
        win, hop = chunk_geometry(flags, 2)
        chunk = 0.1 * torch.randn(S, win, device="cuda")
        rows = []
        for name, kw in configs:
            dec = BatchedStreamSyncFusionBeamDecoder(m, flags, S, W=W, **kw)
            for _ in range(max(args.warmup, 5)):
                dec.decode(chunk)
            ms = []
            for _ in range(args.runs):
                dec.reset()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    dec.decode(chunk)
                torch.cuda.synchronize()
                ms.append(1e3 * (time.perf_counter() - t0) / args.steps)
            rows.append((name, ms))
            del dec
        print("streaming: %d streams, W = %d, chunk = %d samples (one encoder frame), %d runs of %d consecutive steps"
              % (S, W, win, args.runs, args.steps))
        _report(rows, "chunk step")
    print("one process, not a gate")


if __name__ == "__main__":
    main()
