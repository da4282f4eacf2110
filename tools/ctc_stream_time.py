"""ms per chunk step of the streaming CTC prefix beam search beside the greedy streaming decoder and the streaming
frame-synchronous beam search (a measurement, not a gate):

    python tools/ctc_stream_time.py [--streams 256] [--steps 100] [--runs 3] [--warmup 10] [--W 10]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/ctc_stream_time.py --profile 50

The model is the bench's E6D2 with a CTC head in bf16 (torch.manual_seed(0) weights, V = 2048, the joint's blank bias
raised by 12 as tools/sync_stream_time.py does); the chunk geometry is that tool's (`chunk_geometry(flags, 2)`: 75 ms of
audio, one encoder frame per chunk).  All decoders run in this one process on the same chunk.  A chunk step is one
`decode(chunk)`: features, encoder, head logits, search and the read of every stream's best hypothesis.  Every run resets
the decoder (not timed) and takes `--steps` consecutive steps between two synchronisations.  The CTC decoder runs plain,
with the synthetic trigram of tools/ctc_ngram_time.py (random weights, no text: what the look-ups cost, nothing about
recognition), and with the trigram and a 100-phrase bias list.

Second part: where an advance of the plain search spends its time.  `advance` on the chunk's logits is timed against
`advance` with `n_frames = 0` for every stream - no row of the row pass, a walk that only loads and stores the beam, the
compaction, the advance's one device-to-host read and its synchronisation - and `nbest()` / `best()` / `idle_frames()`
alone.  The kernels' own times (row pass, walk, compaction) are the profiler's: --profile N runs N plain advances and
nothing else."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ctc_ngram_time import corpus  # noqa: E402


def _stats(ms):
    ms = sorted(ms)
    return ms[len(ms) // 2], ms[0], ms[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--W", type=int, default=10)
    ap.add_argument("--sentences", type=int, default=2000)
    ap.add_argument("--profile", type=int, default=0, metavar="N", help="N plain advances only (for rocprofv3)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ctc_stream_time: needs the GPU (a CPU run measures nothing)")
    from edgedict_amd.bias import ContextGraph
    from edgedict_amd.decode import StreamingCTCBeamSearch
    from edgedict_amd.flags import make_flags, model_kwargs
    from edgedict_amd.models import Transducer
    from edgedict_amd.ngram import NGramLM
    from edgedict_amd.stream import (BatchedStreamCTCBeamDecoder, BatchedStreamDecoder, BatchedStreamSyncBeamDecoder,
                                     chunk_geometry)
    flags = make_flags("E6D2")
    V = 2048
    torch.manual_seed(0)
    m = Transducer(ctc_weight=0.3, **model_kwargs(flags, vocab_size=V)).cuda().eval()
    m.compute_dtype = "bf16"
    with torch.no_grad():
        m.joint.joint[2].bias[0] += 12.0
    S, W = args.streams, args.W
    win, hop = chunk_geometry(flags, 2)
    chunk = 0.1 * torch.randn(S, win, device="cuda")
    # a run never compacts below what W hypotheses keep alive: room for every frame between two resets
    NC = max(32 * W + 1024, W * (args.steps + args.warmup + max(args.profile, 0) + 2) + 1)

    if args.profile:
        dec = BatchedStreamCTCBeamDecoder(m, flags, S, W=W, node_capacity=NC)
        with torch.no_grad():
            logits = m._ctc_logits(dec.encode(chunk)).contiguous()
        for _ in range(args.profile):
            dec.search.advance(logits)
        torch.cuda.synchronize()
        return

    sents = corpus(V, args.sentences)
    lm = NGramLM.train(sents, 3, V, blank=m.blank)
    rng = np.random.default_rng(1)
    graph = ContextGraph([s[:int(rng.integers(2, 5))] for s in sents[:100]], 1.5, V, blank=m.blank)
    fused = dict(lm=lm, lm_weight=0.5, length_bonus=0.3)
    decs = [("CTC beam, plain                ", BatchedStreamCTCBeamDecoder(m, flags, S, W=W, node_capacity=NC)),
            ("CTC beam + trigram             ", BatchedStreamCTCBeamDecoder(m, flags, S, W=W, node_capacity=NC, **fused)),
            ("CTC beam + trigram + 100 phrases", BatchedStreamCTCBeamDecoder(m, flags, S, W=W, node_capacity=NC, bias=graph, **fused)),
            ("BatchedStreamDecoder (greedy)  ", BatchedStreamDecoder(m, flags, S)),
            ("BatchedStreamSyncBeamDecoder   ", BatchedStreamSyncBeamDecoder(m, flags, S, W=W))]
    print("E6D2 bf16 with a CTC head, %d streams, W = %d, V = %d, chunk = %d samples (hop %d), %d runs of %d consecutive "
          "steps; trigram: %d states, %d arcs; bias list: %d states"
          % (S, W, V, win, hop, args.runs, args.steps, lm.n_states, lm.n_arcs, graph.n_states))
    for name, dec in decs:
        for _ in range(args.warmup):
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
        med, lo, hi = _stats(ms)
        print("%s: %8.4f ms per chunk step (%.4f .. %.4f)" % (name, med, lo, hi))

    # the parts of an advance: the plain search alone on one chunk's head logits
    dec = decs[0][1]
    with torch.no_grad():
        logits = m._ctc_logits(dec.encode(chunk)).contiguous()
    Tc = logits.shape[1]
    sb = StreamingCTCBeamSearch(S, V, W=W, blank=m.blank, node_capacity=NC)
    none = np.zeros(S, dtype=np.int32)
    calls = (lambda: sb.advance(logits), lambda: sb.advance(logits, none), sb.nbest, sb.best, sb.idle_frames)
    acc = [[] for _ in calls]
    for _ in range(args.runs):
        sb.reset()
        for _ in range(args.warmup):
            sb.advance(logits)
        tot = [0.0] * len(calls)
        for _ in range(args.steps):
            for k, fn in enumerate(calls):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                tot[k] += 1e3 * (time.perf_counter() - t0)
        for k in range(len(calls)):
            acc[k].append(tot[k] / args.steps)
    names = ("advance, %d frame(s)        " % Tc, "advance, no frame          ", "nbest()                    ",
             "best()                     ", "idle_frames()              ")
    for name, t in zip(names, acc):
        med, lo, hi = _stats(t)
        print("%s: %8.4f ms per call (%.4f .. %.4f)" % (name, med, lo, hi))
    print("an advance that takes no frame = %.0f %% of an advance over %d frame(s); live nodes per stream at the end: %d at "
          "most; committed tokens: %d at most"
          % (100.0 * _stats(acc[1])[0] / _stats(acc[0])[0], Tc, int(sb.live_nodes().max()),
             max(len(c) for c in sb.committed())))
    print("one process, %d runs, not a gate" % args.runs)


if __name__ == "__main__":
    main()
