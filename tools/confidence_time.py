"""Time of the confidence pass over N-best lists on the bench batch (one run, not a gate):

    python tools/confidence_time.py [--runs 3] [--warmup 2] [--beam 10]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/confidence_time.py --profile 5

The bench's model and batch (bench.py's preset E6D2, 64 utterances of 15 s; seeded random weights), in bf16, eval mode,
beam width W = 10.  Three model-level calls, each INCLUDING the encoder, alternate in one process:
`Transducer.sync_beam_search_nbest` alone, followed by `Transducer.confidence` of the 1-best of every list, and followed
by `Transducer.confidence` of the whole lists (the pass runs the encoder a second time there: a caller who keeps the
encoder output calls `decode.hypothesis_confidence` and saves it; that call is timed too, on its own).  Beside them the
device time of the two new kernels alone, on the shapes of the whole-list pass (device tensors prepared beforehand):
`decode.confidence_hidden_rows` and `loss.row_confidence` on one chunk of rows.  A model with random weights emits a
token on almost every frame, so its hypotheses are several times longer than a trained model's: the row counts are
printed.  Device events around every call, a synchronize between calls; prints the median (min .. max) of --runs
alternating runs.  --profile N runs N whole-list passes on a kept encoder output and nothing else: the run to put
under rocprofv3, whose kernel statistics split the pass into its launches."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
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
    ap.add_argument("--beam", type=int, default=10)
    ap.add_argument("--profile", type=int, default=0, metavar="N", help="N whole-list passes only (for rocprofv3)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("confidence_time: needs the GPU (a CPU run measures nothing)")
    from bench import synth_batch
    from edgedict_amd import decode
    from edgedict_amd.decode import NBestResult
    from edgedict_amd.features import StackedLogFbank
    from edgedict_amd.flags import make_flags, model_kwargs
    from edgedict_amd.loss import row_confidence
    from edgedict_amd.models import Transducer
    dev = torch.device("cuda", 0)
    flags = make_flags(args.preset, gradclip=None, dither=1e-5)
    wave, wave_len, _, _ = synth_batch(flags, args.batch, args.seconds, args.labels, 1000, dev)
    fb = StackedLogFbank(n_frame=flags.downsample, pad_to_divisible=True, out_dtype=torch.float32,
                         sample_rate=getattr(flags, "sample_rate", 16000), win_length=flags.win_length,
                         hop_length=flags.hop_length, n_fft=flags.n_fft, n_filt=flags.feature_size, dither=0.0).to(dev)
    torch.manual_seed(0)
    m = Transducer(**model_kwargs(flags, vocab_size=flags.bpe_size)).to(dev).eval()
    m.compute_dtype = "bf16"
    W = args.beam
    with torch.no_grad():
        xs, xlen = fb(wave, wave_len)
        xs = xs[:, :int(xlen.max())].contiguous()
        enc, _ = m.encoder(xs)
        enc = enc.contiguous()
        lens = m.scale_length(enc, xlen.cpu()).numpy().astype(np.int32)
        lists = m.sync_beam_search_nbest(xs, xlen, W)

    def best(res):
        return [NBestResult(r.tokens[:1], r.frames[:1], r.token_logp[:1], r.logp[:1]) for r in res]

    rows_all = sum(len(t) for r in lists for t in r.tokens)
    rows_one = sum(len(r.tokens[0]) for r in lists)
    V, J = m.joint.joint[2].weight.shape[0], m.joint.joint[0].weight.shape[0]
    chunk = min(rows_all, max(1, decode.CONF_LOGITS_BYTES // (4 * V)))
    g = torch.Generator(device="cpu").manual_seed(1)
    E1 = decode.joint_rows(m, enc)
    D1 = torch.randn(4096, J, generator=g).to(device=dev, dtype=E1.dtype)
    er = torch.randint(0, E1.shape[0], (chunk,), generator=g, dtype=torch.int32).to(dev)
    dr = torch.randint(0, D1.shape[0], (chunk,), generator=g, dtype=torch.int32).to(dev)
    hid = torch.empty(chunk, J, dtype=E1.dtype, device=dev)
    logits = torch.randn(chunk, V, generator=g).to(dev)
    tok = torch.randint(1, V, (chunk,), generator=g, dtype=torch.int32).to(dev)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        with torch.no_grad():
            out = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), out

    def search_then(pick):
        res = m.sync_beam_search_nbest(xs, xlen, W)
        return m.confidence(xs, xlen, pick(res))

    calls = [
        ("sync_beam_search_nbest                          ", lambda: m.sync_beam_search_nbest(xs, xlen, W)),
        ("sync_beam_search_nbest + confidence (1-best)    ", lambda: search_then(best)),
        ("sync_beam_search_nbest + confidence (whole list)", lambda: search_then(lambda r: r)),
        ("decode.hypothesis_confidence (kept encoder out.)", lambda: decode.hypothesis_confidence(m, enc, lens, lists)),
        ("conf_hidden_rows, one chunk                     ", lambda: decode.confidence_hidden_rows(E1, D1, er, dr, None, hid)),
        ("conf_row_stats, one chunk                       ", lambda: row_confidence(logits, tok)),
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
    conf = outs[3]
    tokc = np.concatenate([c.token[i] for c in conf for i in range(len(c))] or [np.zeros(0)])
    worst = max([float(np.abs(c.raw[i][:, 0] - r.token_logp[i]).max()) for c, r in zip(conf, lists)
                 for i in range(len(r)) if len(r.tokens[i])] or [0.0])
    print("%s, batch %d x %.0f s, bf16, W = %d: encoder output %s, V = %d, J = %d; lists of %d .. %d hypotheses; token rows: "
          "%d in the 1-best, %d in the whole lists; one chunk = %d rows (fp32 logits %.1f MiB)"
          % (args.preset, args.batch, args.seconds, W, list(enc.shape), V, J, min(len(r) for r in lists),
             max(len(r) for r in lists), rows_one, rows_all, chunk, chunk * V * 4 / 2.0 ** 20))
    print("Tsallis (alpha 1/3) token confidence of this random model: mean %.3f, min %.3f, max %.3f; largest |raw logp - "
          "token_logp| %.3g (bf16; no claim: there is no corpus, no calibration is measured)"
          % (float(tokc.mean()) if tokc.size else float("nan"), float(tokc.min()) if tokc.size else float("nan"),
             float(tokc.max()) if tokc.size else float("nan"), worst))
    for (name, _), t in zip(calls, ms):
        print("%s: %.3f ms per batch (%.3f .. %.3f)" % ((name,) + _stats(t)))
    print("median of %d alternating runs in one process, not a gate" % args.runs)


if __name__ == "__main__":
    main()
