"""ms per chunk step of the streaming frame-synchronous beam search beside the streaming best-first search and the greedy
streaming decoder (a measurement, not a gate):

    python tools/sync_stream_time.py [--streams 256] [--steps 100] [--runs 3] [--warmup 10] [--W 10]

The model is the bench's E6D2 in bf16 (torch.manual_seed(0) weights, V = 2048, the joint's blank bias raised by 12 as
tools/sync_beam_time.py does, so that the best-first search pops its minimum of W hypotheses per frame); the chunk
geometry is tools/stream_step_time.py's (`chunk_geometry(flags, 2)`: 75 ms of audio, one encoder frame per chunk).  All
three decoders run in this one process on the same chunk.  A chunk step is one `decode(chunk)`: features, encoder,
search and - for the two beam decoders - the read of every stream's best hypothesis.  Every run resets the decoders (not
timed) and takes `--steps` consecutive steps between two synchronisations.

Second part: where an advance of the frame-synchronous search spends its time.  `advance_rows` on one frame is timed
against `advance_rows` on NO frame (`n_frames = 0` for every stream), which launches nothing but the compaction and then
does the advance's one device-to-host read and its stream synchronisation on the same trees: the share of an advance that
is compaction plus host read.  `nbest()` and `best()` (the read-out kernel, its reads, a second synchronisation and the
assembly of the results in Python) are timed alone."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402


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
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sync_stream_time: needs the GPU (a CPU run measures nothing)")
    from edgedict_amd.flags import make_flags, model_kwargs
    from edgedict_amd.models import Transducer
    from edgedict_amd.stream import (BatchedStreamBeamDecoder, BatchedStreamDecoder, BatchedStreamSyncBeamDecoder,
                                     chunk_geometry)
    flags = make_flags("E6D2")
    torch.manual_seed(0)
    m = Transducer(**model_kwargs(flags, vocab_size=2048)).cuda().eval()
    m.compute_dtype = "bf16"
    with torch.no_grad():
        m.joint.joint[2].bias[0] += 12.0
    S, W = args.streams, args.W
    win, hop = chunk_geometry(flags, 2)
    chunk = 0.1 * torch.randn(S, win, device="cuda")
    decs = [("BatchedStreamSyncBeamDecoder", BatchedStreamSyncBeamDecoder(m, flags, S, W=W)),
            ("BatchedStreamBeamDecoder    ", BatchedStreamBeamDecoder(m, flags, S, W=W)),
            ("BatchedStreamDecoder        ", BatchedStreamDecoder(m, flags, S))]
    print("E6D2 bf16, %d streams, W = %d, V = 2048, chunk = %d samples (hop %d), %d runs of %d consecutive steps"
          % (S, W, win, hop, args.runs, args.steps))
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

    # the parts of an advance: the search alone on one frame's joint rows
    dec = decs[0][1]
    sb = dec.search
    with torch.no_grad():
        xs, _ = dec.transform(chunk)
        enc, _ = m.encoder(xs)
        enc = enc.contiguous()
        E1 = sb.joint_rows(enc)
    T, P = enc.shape[1], enc.shape[2]
    none = np.zeros(S, dtype=np.int32)
    full, empty, read, top = [], [], [], []
    for _ in range(args.runs):
        sb.reset()
        for _ in range(args.warmup):
            sb.advance_rows(E1, P)
        acc = [0.0, 0.0, 0.0, 0.0]
        for _ in range(args.steps):
            for k, fn in enumerate((lambda: sb.advance_rows(E1, P), lambda: sb.advance_rows(E1, P, none), sb.nbest,
                                   sb.best)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                acc[k] += 1e3 * (time.perf_counter() - t0)
        full.append(acc[0] / args.steps)
        empty.append(acc[1] / args.steps)
        read.append(acc[2] / args.steps)
        top.append(acc[3] / args.steps)
    for name, t in (("advance, %d frame(s)        " % T, full), ("advance, no frame          ", empty),
                    ("nbest()                    ", read), ("best()                     ", top)):
        med, lo, hi = _stats(t)
        print("%s: %8.4f ms per call (%.4f .. %.4f)" % (name, med, lo, hi))
    print("compaction + host read = %.0f %% of an advance over %d frame(s); live nodes per stream at the end: %d at most"
          % (100.0 * _stats(empty)[0] / _stats(full)[0], T, int(sb.live_nodes().max())))
    print("one process, %d runs, not a gate" % args.runs)


if __name__ == "__main__":
    main()
