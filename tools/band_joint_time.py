"""Time of the joint + loss chain under emission windows, on the box rows against on the band rows (DESIGN.md section
4.40): _JointLossFn forward plus backward on the bench lattice [64, 201, 65, 2048] - bf16, bench-sized joint, weight
gradients included - with and without a loss.BandPlan:

    python tools/band_joint_time.py [--reps 20] [--slack 5]

Windows: a random alignment per utterance (sorted random frames), `slack` frames either side - the set-up of
tools/arloss_grad_time.py, so its live-cell fraction carries over.  Device events around forward + backward - on the
band route around the plan as well (table, scan, host read, fill), with nothing enqueued to hide the read behind - and
the two routes alternate in one process.  Prints the median (min .. max) of each route, the per-kernel ops.timed medians,
joint_rows / joint_packed_rows, the peak of torch.cuda.max_memory_allocated of each route and the host time of the plan
(start of rnnt_band_plan to the return of its event wait, with an idle device: the wait is the device work itself)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from edgedict_amd import config, ops  # noqa: E402
from edgedict_amd.loss import alignment_windows, rnnt_band_plan  # noqa: E402
from edgedict_amd.models import _JointLossFn  # noqa: E402


def _stats(ms):
    ms = sorted(ms)
    return ms[len(ms) // 2], ms[0], ms[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--slack", type=int, default=5)
    ap.add_argument("--shape", type=int, nargs=7, default=[64, 201, 65, 2048, 640, 256, 640],
                    metavar=("B", "T", "U1", "V", "P", "P2", "J"), help="default: E6D2's joint on the bench batch")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("band_joint_time: needs the GPU (a CPU run measures nothing)")
    B, T, U1, V, P, P2, J = args.shape
    cd = torch.bfloat16
    g = torch.Generator(device="cpu").manual_seed(0)
    act = torch.randint(max(1, 3 * T // 4), T + 1, (B,), generator=g, dtype=torch.int32)
    ylen = torch.randint(U1 // 2, U1, (B,), generator=g, dtype=torch.int32)
    act[0], ylen[0] = T, U1 - 1
    labels = torch.randint(4, V, (B, U1 - 1), generator=g, dtype=torch.int32).cuda()
    frames = torch.full((B, U1 - 1), -1, dtype=torch.int32)
    for b in range(B):
        n = int(ylen[b])
        frames[b, :n] = torch.sort(torch.randint(0, int(act[b]), (n,), generator=g, dtype=torch.int32)).values
    act_d, ylen_d = act.cuda(), ylen.cuda()
    lo, hi = alignment_windows(frames.cuda(), act_d, ylen_d, args.slack, args.slack)
    enc = (0.5 * torch.randn(B, T, P, generator=g)).cuda().to(cd).requires_grad_(True)
    dec = (0.5 * torch.randn(B, U1, P2, generator=g)).cuda().to(cd).requires_grad_(True)
    w1 = torch.nn.Parameter((torch.randn(J, P + P2, generator=g) / 30).cuda())
    b1 = torch.nn.Parameter(torch.zeros(J).cuda())
    w2 = torch.nn.Parameter((torch.randn(V, J, generator=g) / 25).cuda())
    b2 = torch.nn.Parameter(torch.zeros(V).cuda())

    def step(plan):
        loss = _JointLossFn.apply(enc, dec, w1, b1, w2, b2, labels, act, ylen, 0, cd, 0.0, lo, hi, plan)
        loss.backward()
        return loss

    routes = ("band", "box")
    total = {r: [] for r in routes}
    kernels = {r: {} for r in routes}
    peak = {r: 0 for r in routes}
    plan_ms = []
    info = {}
    for it in range(args.warmup + args.reps):
        for route in routes:
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            ops.TIMERS = {}
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            plan = None
            if route == "band":
                # inside the timed region, as the box route's own rnnt_band launch is: table, scan, the host read, fill
                t0 = time.perf_counter()
                plan = rnnt_band_plan(lo, hi, act_d, ylen_d, T, finish=False)
                plan.wait()
                t1 = time.perf_counter()
                plan.finish()
                if it >= args.warmup:
                    plan_ms.append(1e3 * (t1 - t0))
            loss = step(plan)
            end.record()
            torch.cuda.synchronize()
            if it >= args.warmup:
                total[route].append(start.elapsed_time(end))
                for tag, (_, ms) in ops.timer_summary().items():
                    kernels[route].setdefault(tag, []).append(ms)
                peak[route] = max(peak[route], torch.cuda.max_memory_allocated())
            if it == 0:
                info[route] = (float(loss.detach()), int(ops.LAST["joint_rows"]), int(ops.LAST["joint_packed_rows"]),
                               int(ops.LAST["joint_band_rows"]))
            del loss
    ops.TIMERS = None
    print("band_joint_time: lattice [%d, %d, %d, %d], bf16, P %d + %d, J %d, slack %d, %d warm-up + %d reps, fused_lse %s, "
          "fused_colsum %s" % (B, T, U1, V, P, P2, J, args.slack, args.warmup, args.reps, bool(config.FUSED_LSE),
                               bool(config.FUSED_DB2)))
    for route in routes:
        loss, rows, packed, live = info[route]
        print("%-4s joint_rows %d, joint_packed_rows %d, joint_band_rows %d (%.4f of the box), loss %.6f"
              % (route, rows, packed, live, live / rows, loss))
    print("forward + backward of _JointLossFn, ms: median (min .. max)")
    for route in routes:
        print("  %-4s %8.3f  (%.3f .. %.3f)   peak memory %.1f MB" % ((route,) + _stats(total[route]) + (peak[route] / 2 ** 20,)))
    print("  band max %s box min" % ("<" if max(total["band"]) < min(total["box"]) else ">="))
    print("per kernel (ops.timed), ms median: band / box")
    for tag in sorted(set(kernels["band"]) | set(kernels["box"])):
        cell = lambda r: "%8.3f" % _stats(kernels[r][tag])[0] if tag in kernels[r] else "       -"
        print("  %-20s %s  %s" % (tag, cell("band"), cell("box")))
    print("plan, host ms from the start of rnnt_band_plan to the return of its event wait (idle device): "
          "median %.3f (%.3f .. %.3f)" % _stats(plan_ms))


if __name__ == "__main__":
    main()
