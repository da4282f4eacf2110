"""The tail of the encoder stack's backward pass (what runs after the last BPTT launch) at the E6D2 bench geometry.

Two views, because `rocprofv3 --kernel-trace` stretches the step and re-orders the background products
(profiles/README.md):

  python tools/tail_report.py marks [N]       UN-profiled, N stamped training steps (default 8): per step, GPU ms from
                                              stack_bwd:enter to stack_bwd:exit, the span of the BPTT launches (in-kernel
                                              stamps), their difference (= prologue + tail) and the launch period
  python tools/tail_report.py trace DB        a rocprofv3 results DB of `bench.py --steps 3 --warmup 1`: per training
                                              step the tail (end of the last BPTT launch -> end of the last kernel of the
                                              pass), and for the last step every kernel that ends after the last launch,
                                              with queue, start, end, duration, and the two chains' lengths

The switch under test is EDGEDICT_STACK_TAIL (csrc/encoder_stack.hip): run once with =0 and once with the default."""
import ctypes
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# kernels that only the stack's backward pass enqueues behind its last launch
TAIL_ONLY = ("unpermute_rows", "stack_sum_parts_kernel", "stack_input_norm_bwd_kernel")


def marks(n_steps):
    import numpy as np
    import torch
    import bench
    from edgedict_amd import _lib, ops
    from edgedict_amd.flags import make_flags
    from edgedict_amd.trainer import TrainEngine
    lib = _lib.load()
    flags = make_flags("E6D2", gradclip=None, dither=1e-5)
    flags.sub_batch_size = 64
    torch.manual_seed(0)
    dev = torch.device("cuda", 0)
    eng = TrainEngine(flags, device=dev, compute_dtype="bf16")
    batch = bench.synth_batch(flags, 64, 15.0, 64, 1000, dev)
    nxt = (batch[0], batch[1])
    for _ in range(5):
        eng.train_step(*batch, next_batch=nxt)
    torch.cuda.synchronize()
    lib.edgedict_stack_time_launches(1)
    print("EDGEDICT_STACK_TAIL=%s" % os.environ.get("EDGEDICT_STACK_TAIL", "(default)"))
    print("step  stack_bwd ms  BPTT span ms  launches  period us  prologue+tail ms  step ms")
    res = []
    for i in range(n_steps):
        ops.MARKS = []
        eng.train_step(*batch, next_batch=nxt)
        torch.cuda.synchronize()
        m, ops.MARKS = ops.MARKS, None
        ev = {tag: e for tag, _, e in m}
        bwd = ev["stack_bwd:enter"].elapsed_time(ev["stack_bwd:exit"])
        step = ev["step:enter"].elapsed_time(ev["step:exit"])
        buf = (ctypes.c_ulonglong * 8192)()
        n = ctypes.c_int(0)
        assert lib.edgedict_stack_launch_stamps(1, buf, 4096, ctypes.byref(n)) == 0
        raw = np.array(buf[:2 * n.value], dtype=np.uint64).reshape(-1, 2)
        ok = (raw[:, 1] > raw[:, 0]) & (raw[:, 0] != np.uint64(0xffffffffffffffff))
        st = raw[ok].astype(np.float64) * 0.01
        span = (st[-1, 1] - st[0, 0]) * 1e-3
        res.append((bwd, span, bwd - span, step))
        print("%4d  %12.3f  %12.3f  %8d  %9.1f  %16.3f  %7.2f" % (i, bwd, span, len(st), 1e3 * span / len(st), bwd - span, step))
    lib.edgedict_stack_time_launches(0)
    r = np.array(res)
    print("mean  %12.3f  %12.3f  %8s  %9s  %16.3f  %7.2f" % (r[:, 0].mean(), r[:, 1].mean(), "", "", r[:, 2].mean(), r[:, 3].mean()))
    print("median%11.3f  %12.3f  %8s  %9s  %16.3f  %7.2f" % tuple([np.median(r[:, 0]), np.median(r[:, 1]), "", ""]
                                                                  + [np.median(r[:, 2]), np.median(r[:, 3])]))
    print("min..max of prologue+tail: %.3f .. %.3f ms" % (r[:, 2].min(), r[:, 2].max()))


def short(n):
    n = n.replace("(anonymous namespace)::", "").replace("void ", "")
    return re.sub(r"\(.*", "", n)[:64]


def trace(path):
    import sqlite3
    db = sqlite3.connect(path)
    rows = list(db.execute("select name,start,end,queue_id,grid_x from kernels order by start"))
    idx = [i for i, r in enumerate(rows) if "stack_bwd_sk" in r[0]]
    groups = []
    for i in idx:                                    # a step's launches are < 2 ms apart
        if groups and rows[i][1] - rows[groups[-1][-1]][2] < 2e6:
            groups[-1].append(i)
        else:
            groups.append([i])
    print("EDGEDICT_STACK_TAIL=%s (rocprofv3 --kernel-trace: the step is stretched and the background products re-ordered)"
          % os.environ.get("EDGEDICT_STACK_TAIL", "(default)"))
    for gi, g in enumerate(groups):
        t1 = rows[g[-1]][2]
        span = (t1 - rows[g[0]][1]) / 1e6
        # the pass's own kernels behind the last launch: up to the last tail-only kernel that starts within 4 ms
        last = None
        for j in range(g[-1] + 1, len(rows)):
            if rows[j][1] - t1 > 4e6:
                break
            if any(k in rows[j][0] for k in TAIL_ONLY):
                last = j
        if last is None:
            continue
        t_end = max(rows[j][2] for j in range(g[-1] + 1, last + 1) if any(k in rows[j][0] for k in TAIL_ONLY))
        print("step %d: %d BPTT launches, span %.3f ms, period %.1f us, tail (last launch end -> last kernel of the pass) %.1f us"
              % (gi, len(g), span, 1e3 * span / len(g), (t_end - t1) / 1e3))
        if gi != len(groups) - 1:
            continue
        print("--- last step: kernels that end after the last BPTT launch ends (us relative to that end)")
        print("    start      end      dur  queue  kernel")
        byq = {}
        for j, r in enumerate(rows):
            if r[2] <= t1 or r[1] > t_end or j in g:
                continue
            if r[1] < t1 - 3e6:
                continue
            print("%9.1f %8.1f %8.1f  q%-4s %s grid %d" % ((r[1] - t1) / 1e3, (r[2] - t1) / 1e3, (r[2] - r[1]) / 1e3, r[3], short(r[0]), r[4]))
            q = byq.setdefault(r[3], [r[1], r[2], 0.0])
            q[1] = max(q[1], r[2])
            q[2] += (r[2] - max(r[1], t1)) / 1e3
        for q, (a, b, busy) in sorted(byq.items()):
            print("queue %s: last kernel ends %.1f us after the last launch, busy %.1f us of them" % (q, (b - t1) / 1e3, busy))


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "trace":
        trace(sys.argv[2])
    elif len(sys.argv) >= 2 and sys.argv[1] == "marks":
        marks(int(sys.argv[2]) if len(sys.argv) > 2 else 8)
    else:
        raise SystemExit(__doc__)
