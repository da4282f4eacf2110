"""Time of the batched edit distance on synthetic N-best lists (one run, not a gate):

    python tools/edit_distance_time.py [--runs 3] [--warmup 2] [--batch 64] [--beam 10]

No model: 64 utterances x 10 hypotheses of 152 .. 201 tokens - the length range of the random bench model's lists
(tools/ctc_rescore_time.py) - over a vocabulary of 1000, every hypothesis a corrupted copy of its utterance's first one,
against (a) references of transcript length, 32 .. 64 tokens, and (b) references of the hypotheses' own length, 152 ..
201 tokens (a corrupted copy again, so that hits, substitutions, insertions and deletions all occur).  Device tensors
are prepared beforehand; `metrics.edit_distance` is timed with device events around every call and a synchronize between
calls, the two cases alternating in one process; beside it the host oracle of the tests (numpy, one row at a time) on the
same lists, wall clock, once.  Prints the median (min .. max) of --runs runs, both routes' times and whether the two
agree on every integer (and a checksum of them)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def _stats(ms):
    ms = sorted(ms)
    return ms[len(ms) // 2], ms[0], ms[-1]


def _corrupt(rng, base, length, vocab):
    """A sequence of `length` tokens derived from `base`: tokens dropped or inserted to reach the length, then one in
    ten replaced."""
    t = list(base)
    while len(t) > length:
        del t[int(rng.integers(0, len(t)))]
    while len(t) < length:
        t.insert(int(rng.integers(0, len(t) + 1)), int(rng.integers(1, vocab)))
    t = np.array(t, dtype=np.int32)
    swap = rng.random(t.size) < 0.1
    t[swap] = rng.integers(1, vocab, size=int(swap.sum()))
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--beam", type=int, default=10)
    ap.add_argument("--vocab", type=int, default=1000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("edit_distance_time: needs the GPU (a CPU run measures nothing)")
    import edit_distance_ref as ER
    from edgedict_amd.metrics import edit_distance
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    B, N, V = args.batch, args.beam, args.vocab
    Uh = 201
    hyps = np.zeros((B, N, Uh), dtype=np.int32)
    hl = rng.integers(152, 202, size=(B, N)).astype(np.int32)
    for b in range(B):
        first = rng.integers(1, V, size=int(hl[b, 0])).astype(np.int32)
        for n in range(N):
            hyps[b, n, :hl[b, n]] = first if n == 0 else _corrupt(rng, first, int(hl[b, n]), V)
    cases = []
    for name, lo, hi in (("references of 32 .. 64 tokens  ", 32, 64), ("references of 152 .. 201 tokens", 152, 201)):
        rl = rng.integers(lo, hi + 1, size=B).astype(np.int32)
        refs = np.zeros((B, hi), dtype=np.int32)
        for b in range(B):
            refs[b, :rl[b]] = _corrupt(rng, hyps[b, 0, :hl[b, 0]], int(rl[b]), V)
        cases.append((name, refs, rl))
    d_hyps, d_hl = torch.from_numpy(hyps).to(dev), torch.from_numpy(hl).to(dev)
    d_cases = [(torch.from_numpy(refs).to(dev), torch.from_numpy(rl).to(dev)) for _, refs, rl in cases]

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), out

    calls = [lambda r=r, l=l: edit_distance(d_hyps, d_hl, r, l) for r, l in d_cases]
    for _ in range(args.warmup):
        for fn in calls:
            timed(fn)
    ms = [[] for _ in calls]
    outs = [None] * len(calls)
    for _ in range(args.runs):
        for i, fn in enumerate(calls):
            t, outs[i] = timed(fn)
            ms[i].append(t)
    print("edit distance, %d utterances x %d hypotheses of %d .. %d tokens, vocabulary %d"
          % (B, N, int(hl.min()), int(hl.max()), V))
    for (name, refs, rl), t, out in zip(cases, ms, outs):
        got = out.cpu().numpy()
        t0 = time.perf_counter()
        want = ER.counts_nbest(hyps, hl, None, refs, rl)
        host = (time.perf_counter() - t0) * 1e3
        tot = got.reshape(-1, 4).astype(np.int64).sum(axis=0)
        print("%s: metrics.edit_distance %.3f ms per batch (%.3f .. %.3f); host oracle (numpy rows) %.0f ms; equal on "
              "every integer: %s; checksum (dist, sub, del, ins) = %s, token error rate %.4f"
              % ((name,) + _stats(t) + (host, bool(np.array_equal(got, want)), tot.tolist(),
                                        tot[0] / float(N * rl.astype(np.int64).sum()))))
    print("median of %d alternating runs in one process, not a gate" % args.runs)


if __name__ == "__main__":
    main()
