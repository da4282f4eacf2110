"""Cost and gain of skipping CTC-blank frames ahead of the RNN-T beam searches (a measurement,
not a gate):

    python tools/frame_skip_time.py [--runs 3] [--warmup 2] [--W 10]

Workload: tools/sync_fusion_time.py's offline part - the bench's E6D2 batch (64 utterances of 15 s, ragged lengths,
`bench.synth_batch` seed 1000) through the bench's feature front-end, bf16, torch.manual_seed(0) weights with the joint's
blank bias raised by 12 - on a model built with a CTC head (`ctc_weight=0.3`).  The weights are random, so the head's
blank posterior says nothing about speech: the thresholds are QUANTILES of a first pass's `lp_blank` over the live
frames, chosen to keep about 100 % (threshold 1), 50 % and 25 % of them.

Timed, alternating inside a run, median of `--runs`: `Transducer.sync_beam_search` and `Transducer.beam_search`, plain
and with `skip_blank=` at the three thresholds.  Each call includes the encoder, as the public entry point does; the
encoder alone is timed too, and so is the front alone (`decode.skip_blank_frames` on a given encoder output: the head
product, three kernels, one read to the host).

What the figures do not say: which share of the frames a TRAINED model's head would let go, and what dropping them does
to the word error rate.  Neither is measured here - there is no corpus."""
import argparse
import math
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
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=15.0)
    ap.add_argument("--W", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("frame_skip_time: needs the GPU (a CPU run measures nothing)")
    import bench
    from edgedict_amd import decode
    from edgedict_amd.features import StackedLogFbank
    from edgedict_amd.flags import make_flags, model_kwargs
    from edgedict_amd.loss import ctc_blank_skip
    from edgedict_amd.models import Transducer
    dev = torch.device("cuda", 0)
    flags = make_flags("E6D2", gradclip=None, dither=1e-5)
    V = flags.bpe_size
    torch.manual_seed(0)
    m = Transducer(**model_kwargs(flags, vocab_size=V), ctc_weight=0.3).to(dev).eval()
    m.compute_dtype = "bf16"
    with torch.no_grad():
        m.joint.joint[2].bias[0] += 12.0
    W = args.W
    wave, wave_len, _, _ = bench.synth_batch(flags, args.batch, args.seconds, 64, 1000, dev)
    fb = StackedLogFbank(n_frame=flags.downsample, pad_to_divisible=True, out_dtype=torch.float32,
                         sample_rate=getattr(flags, "sample_rate", 16000), win_length=flags.win_length,
                         hop_length=flags.hop_length, n_fft=flags.n_fft, n_filt=flags.feature_size,
                         dither=0.0).to(dev)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    with torch.no_grad():
        xs, xlen = fb(wave, wave_len)
        enc, _ = m.encoder(xs)
        enc = enc.contiguous()
        lens = m.scale_length(enc, xlen.cpu()).numpy().astype(np.int32)
        # first pass: the thresholds are quantiles of lp_blank over the live frames
        act = torch.from_numpy(lens).to(dev)
        _, _, lp = ctc_blank_skip(m._ctc_logits(enc).contiguous(), act, 1.0, m.blank)
        lp = lp.cpu().numpy()
        live = np.arange(lp.shape[1])[None, :] < lens[:, None]
        points = [("100 %", 1.0)] + [("%d %%" % round(100 * q), min(1.0, math.exp(float(np.quantile(lp[live], q)))))
                                     for q in (0.5, 0.25)]
        shares = []
        for _, thr in points:
            sk = decode.skip_blank_frames(m, enc, lens, thr)
            shares.append((int(sk.lens.sum()), int(sk.enc_out.shape[1])))
        configs = [("sync", "plain", lambda: m.sync_beam_search(xs, xlen, W=W)),
                   ("best-first", "plain", lambda: m.beam_search(xs, xlen, W=W))]
        for name, thr in points:
            configs.append(("sync", name, lambda thr=thr: m.sync_beam_search(xs, xlen, W=W, skip_blank=thr)))
            configs.append(("best-first", name, lambda thr=thr: m.beam_search(xs, xlen, W=W, skip_blank=thr)))
        configs.append(("encoder", "alone", lambda: m.encoder(xs)))
        for name, thr in points:
            configs.append(("front", name, lambda thr=thr: decode.skip_blank_frames(m, enc, lens, thr)))
        times = [[] for _ in configs]
        for rep in range(args.warmup + args.runs):
            for k, (_, _, fn) in enumerate(configs):
                ms = timed(fn)
                if rep >= args.warmup:
                    times[k].append(ms)
    total = int(lens.sum())
    print("E6D2 bf16 with a CTC head, %d utterances of %.0f s, %d live encoder frames (%d at most), W = %d, V = %d, "
          "%d alternating runs, median (min .. max) ms per batch"
          % (args.batch, args.seconds, total, int(lens.max()), W, V, args.runs))
    for (name, thr), (kept, Tc) in zip(points, shares):
        print("threshold for %-5s: %.6g   kept %d of %d frames = %.1f %%, longest utterance %d frames"
              % (name, thr, kept, total, 100.0 * kept / total, Tc))
    base = {}
    for (what, name, _), t in zip(configs, times):
        med, lo, hi = _stats(t)
        if name == "plain":
            base[what] = med
        tail = "  %+6.1f %% over plain" % (100.0 * (med / base[what] - 1.0)) if what in base and name != "plain" else ""
        print("%-10s %-6s: %9.3f ms (%.3f .. %.3f)%s" % (what, name, med, lo, hi, tail))
    print("every sync / best-first call includes the encoder; one process, not a gate; random weights: the kept share of "
          "a trained model and any WER effect are NOT measured")


if __name__ == "__main__":
    main()
