"""Time of the loss-gradient kernel (ops.timed tag "rnnt_grad") with and without emission windows on the bench lattice
[64, 201, 65, 2048] - bf16, packed, fused column sums - through _JointLossFn, the training path:

    python tools/arloss_grad_time.py [--reps 20] [--slack 5]

Windows: a random alignment per utterance (sorted random frames), `slack` frames either side.  The two calls alternate
in one process; prints one JSON line with both times, the live-cell fraction (ops.LAST["joint_band_rows"] over
ops.LAST["joint_rows"]) and the bytes each kernel has to move by its shapes (logits rows read + gradient rows written;
the restricted kernel reads the live rows only and still writes every row)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from edgedict_amd import config, ops  # noqa: E402
from edgedict_amd.loss import alignment_windows  # noqa: E402
from edgedict_amd.models import _JointLossFn  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--slack", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("arloss_grad_time: needs the GPU (a CPU run measures nothing)")
    B, T, U1, V, P, P2, J = 64, 201, 65, 2048, 640, 256, 640     # E6D2's joint on the bench batch
    cd = torch.bfloat16
    g = torch.Generator(device="cpu").manual_seed(0)
    act = torch.randint(150, T + 1, (B,), generator=g, dtype=torch.int32)
    ylen = torch.randint(32, U1, (B,), generator=g, dtype=torch.int32)
    act[0], ylen[0] = T, U1 - 1
    labels = torch.randint(4, V, (B, U1 - 1), generator=g, dtype=torch.int32).cuda()
    frames = torch.full((B, U1 - 1), -1, dtype=torch.int32)
    for b in range(B):
        n = int(ylen[b])
        frames[b, :n] = torch.sort(torch.randint(0, int(act[b]), (n,), generator=g, dtype=torch.int32)).values
    windows = alignment_windows(frames.cuda(), act.cuda(), ylen.cuda(), args.slack, args.slack)
    enc = (0.5 * torch.randn(B, T, P, generator=g)).cuda().to(cd).requires_grad_(True)
    dec = (0.5 * torch.randn(B, U1, P2, generator=g)).cuda().to(cd).requires_grad_(True)
    w1 = torch.nn.Parameter((torch.randn(J, P + P2, generator=g) / 30).cuda())
    b1 = torch.nn.Parameter(torch.zeros(J).cuda())
    w2 = torch.nn.Parameter((torch.randn(V, J, generator=g) / 25).cuda())
    b2 = torch.nn.Parameter(torch.zeros(V).cuda())

    def step(win):
        tail = () if win is None else win
        loss = _JointLossFn.apply(enc, dec, w1, b1, w2, b2, labels, act, ylen, 0, cd, 0.0, *tail)
        loss.backward()
        return loss

    out = {"lattice": [B, T, U1, V], "dtype": "bf16", "slack": args.slack, "fused_colsum": bool(config.FUSED_DB2),
           "fused_lse": bool(config.FUSED_LSE), "reps": args.reps}
    times = {"windows": [], "plain": []}
    for it in range(args.warmup + args.reps):
        for name, win in (("windows", windows), ("plain", None)):
            ops.TIMERS = {}
            loss = step(win)
            torch.cuda.synchronize()
            if it >= args.warmup:
                times[name].append(ops.timer_summary()["rnnt_grad"][1])
            if it == 0:
                out["loss_" + name] = float(loss)
                if win is not None:
                    out["joint_rows"] = int(ops.LAST["joint_rows"])
                    out["joint_band_rows"] = int(ops.LAST["joint_band_rows"])
    ops.TIMERS = None
    for name, ms in times.items():
        ms.sort()
        out["rnnt_grad_ms_" + name] = {"median": ms[len(ms) // 2], "min": ms[0], "max": ms[-1]}
    rows, live = out["joint_rows"], out["joint_band_rows"]
    out["live_fraction"] = live / rows
    out["bytes_plain"] = 2 * rows * V * 2                        # read every row, write every row (bf16)
    out["bytes_windows"] = (live + rows) * V * 2                 # read the live rows, write every row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
