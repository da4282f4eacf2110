"""Time of CTC rescoring of N-best lists on the bench batch (one run, not a gate):

    python tools/ctc_rescore_time.py [--runs 3] [--warmup 2] [--beam 10]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/ctc_rescore_time.py --profile 5

The bench's model and batch (bench.py's preset E6D2, 64 utterances of 15 s; seeded random weights) with a CTC head, in
bf16, eval mode, beam width W = 10.  Two model-level calls, each INCLUDING the encoder, alternate in one process:
`Transducer.sync_beam_search_nbest` plain and with `ctc_rescore=0.3` (the head's product, one upload of the lists' tokens,
the row pass, one walk per hypothesis, one read to the host, the host's combine and sort).  Beside them, on the head
logits of that batch and that search's hypotheses alone (device tensors prepared beforehand): `loss.ctc_score_nbest`
against the only route there was before it, W forward calls of `loss.CTCLoss(reduction='none')`, one per rank.  A model
with random weights emits a token on almost every frame, so its hypotheses are several times longer than a trained
model's and mostly have no CTC path; the same pair is therefore timed a second time on lists of transcript length: the
batch's own label sequences (32 .. 64 tokens), rank n with one token replaced.  Both routes' workspace bytes are
printed.  Device events around every call, a synchronize between calls; prints the median
(min .. max) of --runs alternating runs.  --profile N runs N `loss.ctc_score_nbest` calls and nothing else: the run to
put under rocprofv3, whose kernel statistics split the call into ctc_score_rows / ctc_score_walk."""
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
    ap.add_argument("--weight", type=float, default=0.3)
    ap.add_argument("--profile", type=int, default=0, metavar="N", help="N loss.ctc_score_nbest calls only (for rocprofv3)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ctc_rescore_time: needs the GPU (a CPU run measures nothing)")
    from bench import synth_batch
    from edgedict_amd import _lib
    from edgedict_amd.features import StackedLogFbank
    from edgedict_amd.flags import make_flags, model_kwargs
    from edgedict_amd.loss import CTCLoss, ctc_score_nbest
    from edgedict_amd.models import Transducer
    dev = torch.device("cuda", 0)
    flags = make_flags(args.preset, gradclip=None, dither=1e-5)
    wave, wave_len, ys, ylen = synth_batch(flags, args.batch, args.seconds, args.labels, 1000, dev)
    fb = StackedLogFbank(n_frame=flags.downsample, pad_to_divisible=True, out_dtype=torch.float32,
                         sample_rate=getattr(flags, "sample_rate", 16000), win_length=flags.win_length,
                         hop_length=flags.hop_length, n_fft=flags.n_fft, n_filt=flags.feature_size, dither=0.0).to(dev)
    torch.manual_seed(0)
    m = Transducer(**model_kwargs(flags, vocab_size=flags.bpe_size), ctc_weight=0.3).to(dev).eval()
    m.compute_dtype = "bf16"
    W = args.beam
    with torch.no_grad():
        xs, xlen = fb(wave, wave_len)
        xs = xs[:, :int(xlen.max())].contiguous()
        h_enc, _ = m.encoder(xs)
        lens = m.scale_length(h_enc, xlen.cpu()).numpy().astype(np.int32)
        act = torch.from_numpy(lens).to(dev)
        logits = m._ctc_logits(h_enc).contiguous()
        lists = m.sync_beam_search_nbest(xs, xlen, W)
    B, T, V = logits.shape

    def pack(token_lists):
        """device hyps [B, N, U], hyp_lens [B, N], n_hyp [B] of per-utterance lists of token arrays, and the per-rank
        route's inputs: labels [B, U] and lengths [B] of every rank, contiguous, made beforehand"""
        N = max(len(r) for r in token_lists)
        U = max(len(t) for r in token_lists for t in r)
        hyps = np.zeros((B, N, U), dtype=np.int32)
        hl = np.zeros((B, N), dtype=np.int32)
        nh = np.array([len(r) for r in token_lists], dtype=np.int32)
        for b, r in enumerate(token_lists):
            for n, t in enumerate(r):
                hyps[b, n, :len(t)] = t
                hl[b, n] = len(t)
        d = [torch.from_numpy(a).to(dev) for a in (hyps, hl, nh)]
        ranks = [(d[0][:, n].contiguous(), d[1][:, n].contiguous()) for n in range(N)]
        return d, ranks, (hyps, hl, nh)

    (d_hyps, d_hl, d_nh), ranks, (hyps, hl, nh) = pack([r.tokens for r in lists])
    N, U = hyps.shape[1], hyps.shape[2]
    # lists of transcript length: the batch's labels, rank n with the token at position 7 n replaced
    ys_h, ylen_h = ys.cpu().numpy(), ylen.cpu().numpy()
    short = []
    for b in range(B):
        base = ys_h[b, :int(ylen_h[b])].astype(np.int64)
        alts = []
        for n in range(W):
            t = base.copy()
            if n and t.size:
                k = (7 * n) % t.size
                t[k] = 1 + (t[k] + n) % (V - 1)
            alts.append(t)
        short.append(alts)
    (s_hyps, s_hl, s_nh), s_ranks, (sh, shl, snh) = pack(short)
    loss_fn = CTCLoss(blank=m.blank, reduction="none", check_lengths=False)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        with torch.no_grad():
            out = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), out

    calls = [
        ("sync_beam_search_nbest                  ", lambda: m.sync_beam_search_nbest(xs, xlen, W)),
        ("sync_beam_search_nbest(ctc_rescore=%.1f) " % args.weight,
         lambda: m.sync_beam_search_nbest(xs, xlen, W, ctc_rescore=args.weight)),
        ("loss.ctc_score_nbest (logits, lists)    ", lambda: ctc_score_nbest(logits, act, d_hyps, d_hl, d_nh, m.blank)),
        ("%2d x loss.CTCLoss fwd, one per rank     " % N,
         lambda: torch.stack([loss_fn(logits, y, act, yl) for y, yl in ranks], dim=1)),
        ("loss.ctc_score_nbest (transcript length)", lambda: ctc_score_nbest(logits, act, s_hyps, s_hl, s_nh, m.blank)),
        ("%2d x loss.CTCLoss fwd (transcript length)" % W,
         lambda: torch.stack([loss_fn(logits, y, act, yl) for y, yl in s_ranks], dim=1)),
    ]
    if args.profile:
        for _ in range(args.profile):
            timed(calls[2][1])
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
    scores, costs = outs[2].cpu().numpy(), outs[3].double().cpu().numpy()
    live = np.arange(N)[None, :] < nh[:, None]
    same = (scores[live].astype(np.float32) == (-costs[live]).astype(np.float32)).all()
    s_scores, s_costs = outs[4].cpu().numpy(), outs[5].double().cpu().numpy()
    s_same = (s_scores.astype(np.float32) == (-s_costs).astype(np.float32)).all()
    moved = sum(int(not np.array_equal(a.tokens[0], b.tokens[0])) for a, b in zip(outs[0], outs[1]))
    print("%s, batch %d x %.0f s, bf16, W = %d: head logits %s, lists of %d .. %d hypotheses, %d .. %d tokens, a CTC path "
          "on %d / %d" % (args.preset, args.batch, args.seconds, W, list(logits.shape), int(nh.min()), int(nh.max()),
                          int(hl[live].min()), int(hl[live].max()), int(np.isfinite(scores[live]).sum()), int(live.sum())))
    print("scores equal to -CTCLoss after the float cast on every live slot: %s; rescoring changed the first hypothesis of "
          "%d / %d utterances of this random model (no claim: there is no corpus, no WER effect is measured)"
          % (same, moved, B))
    print("transcript-length lists: %d hypotheses each, %d .. %d tokens, a CTC path on %d / %d, equal to -CTCLoss after the "
          "float cast: %s" % (W, int(shl.min()), int(shl.max()), int(np.isfinite(s_scores).sum()), s_scores.size, s_same))
    for (name, _), t in zip(calls, ms):
        print("%s: %.3f ms per batch (%.3f .. %.3f)" % ((name,) + _stats(t)))
    lib = _lib.load()
    ws_new = lib.edgedict_ctc_score_workspace_bytes(B, T, N, U)
    ws_old = lib.edgedict_ctc_workspace_bytes(B, T, U)
    print("workspace: ctc_score_nbest %d bytes (+ %d of tokens and lengths); CTCLoss route %d bytes per call, %d for the "
          "%d ranks when all are kept" % (ws_new, hyps.nbytes + hl.nbytes + nh.nbytes, ws_old, N * ws_old, N))
    Us = sh.shape[2]
    ws_old = lib.edgedict_ctc_workspace_bytes(B, T, Us)
    print("workspace, transcript length: ctc_score_nbest %d bytes (+ %d of tokens and lengths); CTCLoss route %d bytes "
          "per call, %d for the %d ranks when all are kept"
          % (lib.edgedict_ctc_score_workspace_bytes(B, T, W, Us), sh.nbytes + shl.nbytes + snh.nbytes, ws_old, W * ws_old,
             W))
    print("median of %d alternating runs in one process, not a gate" % args.runs)


if __name__ == "__main__":
    main()
