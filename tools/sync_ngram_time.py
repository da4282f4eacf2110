"""Cost of the back-off n-gram in the frame-synchronous beam search, offline and streaming, beside the plain search and
the LSTM-fused one (a measurement, not a gate):

    python tools/sync_ngram_time.py [--runs 3] [--warmup 2] [--W 10] [--streams 256] [--steps 100] [--part both]

Offline part: tools/sync_fusion_time.py's workload - the bench's E6D2 batch (64 utterances of 15 s, ragged lengths,
`bench.synth_batch` seed 1000) through the bench's feature front-end, bf16, torch.manual_seed(0) weights with the joint's
blank bias raised by 12 - searched with `Transducer.sync_beam_search` in four configurations, alternating inside a run:
plain; a trigram (`NGramLM.train` on the synthetic corpus generator tools/ctc_ngram_time.py carries; lm_weight 0.3); the
trigram with `ilm_weight = 0.2`; `lm=LMModel(V, 64, 1024, 2)` (random weights, lm_weight 0.3).  Each call includes the
encoder, as the public entry point does.  Prints median (min .. max) ms per batch, utterances/s, the cost over plain and
the n-gram search's time over the plain and over the LSTM-fused search's.

Streaming part: tools/sync_stream_time.py's chunk step - `BatchedStreamSyncFusionBeamDecoder.decode(chunk)` for 256 streams,
one encoder frame per chunk - plain and with the trigram, `--steps` consecutive steps per run between two
synchronisations, every run from a reset (not timed).

What the figures do not say: the weights are random and the corpus synthetic, so nothing here is an accuracy or WER
claim.  The beams of a random model hold few distinct contexts; the LDS fill's cost is that of the unigram level (V
columns per row and frame) plus short arc rows."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def corpus(V, sentences, seed=7):
    """tools/ctc_ngram_time.py's generator (the same as tests/ngram_ref.py's ``corpus``; a tool cannot import the tests)."""
    rng = np.random.default_rng(seed)
    succ = rng.integers(3, V, size=(V, 3))
    out = []
    for _ in range(sentences):
        n = int(rng.integers(3, 12))
        k = int(rng.integers(3, V))
        sent = [k]
        while len(sent) < n:
            k = int(succ[k, rng.integers(0, 3)]) if rng.random() < 0.8 else int(rng.integers(3, V))
            sent.append(k)
        out.append(sent)
    return out


def _stats(ms):
    ms = sorted(ms)
    return ms[len(ms) // 2], ms[0], ms[-1]


def _report(rows, unit, per_s=None):
    base = _stats(rows[0][1])[0]
    for name, t in rows:
        med, lo, hi = _stats(t)
        tail = "" if per_s is None else "  %7.0f utterances/s" % (1e3 * per_s / med)
        print("%-14s: %9.3f ms per %s (%.3f .. %.3f)%s  %+6.1f %% over plain"
              % (name, med, unit, lo, hi, tail, 100.0 * (med / base - 1.0)))
    return {name: _stats(t)[0] for name, t in rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=15.0)
    ap.add_argument("--W", type=int, default=10)
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--order", type=int, default=3)
    ap.add_argument("--sentences", type=int, default=2000)
    ap.add_argument("--part", default="both", choices=["offline", "stream", "both"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sync_ngram_time: needs the GPU (a CPU run measures nothing)")
    import bench
    from edgedict_amd.features import StackedLogFbank
    from edgedict_amd.flags import make_flags, model_kwargs
    from edgedict_amd.lm import LMModel
    from edgedict_amd.models import Transducer
    from edgedict_amd.ngram import NGramLM
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
    ng = NGramLM.train(corpus(V, args.sentences), args.order, V)
    ng.tables(dev)
    ngram = dict(lm=ng, lm_weight=0.3, length_bonus=0.0)
    configs = [("plain", {}), ("n-gram", ngram), ("n-gram + ilm", dict(ilm_weight=0.2, **ngram)),
               ("lstm", dict(lm=lm, lm_weight=0.3, length_bonus=0.0))]
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
        print("offline: E6D2 bf16, %d utterances of %.0f s, %d encoder frames at most, W = %d, V = %d, %d-gram of %d "
              "sentences (%d states, %d arcs), LM 64/1024/2, %d alternating runs"
              % (args.batch, args.seconds, frames, W, V, args.order, args.sentences, ng.n_states, ng.n_arcs, args.runs))
        med = _report([(n, t) for (n, _), t in zip(configs, times)], "batch", per_s=args.batch)
        print("n-gram / plain = %.3f, n-gram / lstm = %.3f, (n-gram + ilm) / plain = %.3f"
              % (med["n-gram"] / med["plain"], med["n-gram"] / med["lstm"], med["n-gram + ilm"] / med["plain"]))

    if args.part in ("stream", "both"):
        S = args.streams
        win, hop = chunk_geometry(flags, 2)
        chunk = 0.1 * torch.randn(S, win, device="cuda")
        rows = []
        for name, kw in configs[:2]:
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
        med = _report(rows, "chunk step")
        print("n-gram / plain = %.3f" % (med["n-gram"] / med["plain"]))
    print("one process, not a gate")


if __name__ == "__main__":
    main()
