"""Time of the CTC prefix beam search with an n-gram LM on the bench shape's head logits (one
run, no pass mark):

    python tools/ctc_ngram_time.py [--reps 3] [--warmup 2] [--W 10] [--order 3] [--sentences 2000]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/ctc_ngram_time.py --profile 5

Logits as tools/ctc_beam_time.py draws them: [64, 201, 2048] bf16, full lengths.  The LM is a trigram trained
(``NGramLM.train``) on a synthetic corpus over the same ids - random weights, no text: the numbers say what the look-ups
cost, nothing about recognition.  Measured on the same logits, alternating in one process, median of ``--reps``:

    ctc_prefix_beam plain / with the trigram / with the trigram and a 100-phrase bias list,
    NGramLM.score_nbest on the fused search's lists, NGramLM.logprobs on 640 states.

--profile N runs N fused searches and nothing else (for rocprofv3: ctc_beam_walk's LM instantiation beside the row pass)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def corpus(V, sentences, seed=7):
    """Sentences of 3 .. 11 ids from 3 .. V-1; with probability 0.8 the next token is one of 3 fixed successors of the
    current one, else uniform.  The same generator as tests/ngram_ref.py's ``corpus`` (a tool cannot import the tests):
    keep the two alike, or say in DESIGN.md section 4.54 that the measured model is no longer the tests' kind."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=201)
    ap.add_argument("--vocab", type=int, default=2048)
    ap.add_argument("--W", type=int, default=10)
    ap.add_argument("--cand", type=int, default=None)
    ap.add_argument("--order", type=int, default=3)
    ap.add_argument("--sentences", type=int, default=2000)
    ap.add_argument("--lm-weight", type=float, default=0.5)
    ap.add_argument("--length-bonus", type=float, default=0.3)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--profile", type=int, default=0, metavar="N", help="N fused searches only (for rocprofv3)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ctc_ngram_time: needs the GPU (a CPU run measures nothing)")
    from edgedict_amd.bias import ContextGraph
    from edgedict_amd.loss import ctc_prefix_beam
    from edgedict_amd.ngram import NGramLM
    dev = torch.device("cuda", 0)
    V = args.vocab
    g = torch.Generator(device="cpu").manual_seed(0)
    z = 3.0 * torch.randn(args.batch, args.frames, V, generator=g)
    z[:, :, 0] += 2.0
    z = z.to(dev).to(torch.bfloat16 if args.dtype == "bf16" else torch.float32).contiguous()
    act = torch.full((args.batch,), args.frames, dtype=torch.int32, device=dev)
    sents = corpus(V, args.sentences)
    lm = NGramLM.train(sents, args.order, V)
    rng = np.random.default_rng(1)
    phrases = [s[:int(rng.integers(2, 5))] for s in sents[:100]]
    graph = ContextGraph(phrases, 1.5, V)
    lm.tables(dev)
    graph.tables(dev)
    fused_kw = dict(lm=lm, lm_weight=args.lm_weight, length_bonus=args.length_bonus)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), out

    plain = lambda: ctc_prefix_beam(z, act, W=args.W, cand=args.cand)
    fused = lambda: ctc_prefix_beam(z, act, W=args.W, cand=args.cand, **fused_kw)
    both = lambda: ctc_prefix_beam(z, act, W=args.W, cand=args.cand, bias=graph, **fused_kw)
    if args.profile:
        for _ in range(args.profile):
            timed(fused)
        return
    out = fused()
    hyps, hyp_lens, n_hyp = out[0].contiguous(), out[3].contiguous(), out[4].contiguous()
    states = torch.arange(640, dtype=torch.int32, device=dev) % lm.n_states
    runs = [("ctc_prefix_beam plain", plain), ("ctc_prefix_beam + %d-gram" % args.order, fused),
            ("ctc_prefix_beam + %d-gram + %d phrases" % (args.order, len(phrases)), both),
            ("score_nbest [%d, %d, %d]" % tuple(hyps.shape), lambda: lm.score_nbest(hyps, hyp_lens, n_hyp)),
            ("logprobs, 640 states x %d" % V, lambda: lm.logprobs(states))]
    for _ in range(args.warmup):
        for _, fn in runs:
            timed(fn)
    ms = [[] for _ in runs]
    for _ in range(args.reps):
        for i, (_, fn) in enumerate(runs):
            ms[i].append(timed(fn)[0])
    top_plain, top_fused = plain()[0][:, 0], out[0][:, 0]
    moved = int((top_plain != top_fused).any(dim=1).sum())
    print("logits [%d, %d, %d] %s, W = %d, cand = %s; %d-gram of %d sentences: %d states, %d arcs; bias list: %d phrases, "
          "%d states; lm_weight %.2f, length_bonus %.2f: top-1 differs from the plain search's on %d of %d utterances"
          % (args.batch, args.frames, V, args.dtype, args.W, args.cand or min(V - 1, 32), args.order, len(sents), lm.n_states,
             lm.n_arcs, len(phrases), graph.n_states, args.lm_weight, args.length_bonus, moved, args.batch))
    base = sorted(ms[0])[len(ms[0]) // 2]
    for (name, _), m in zip(runs, ms):
        m = sorted(m)
        med = m[len(m) // 2]
        print("%-44s %8.3f ms (%.3f .. %.3f)%s" % (name, med, m[0], m[-1],
                                                   "  x%.2f of plain" % (med / base) if "beam" in name else ""))
    print("median of %d alternating runs in one process; random weights, no corpus: no accuracy claim" % args.reps)


if __name__ == "__main__":
    main()
