"""GPU, world_size 2 (two processes sharing cuda:0, gloo transport): the REAL training engine —
auxiliary streams, deferred and in-place accumulated weight gradients, the packed lattice, the
bucket hooks — under data parallelism.  Two ranks that each take half of a batch must end up with
the parameters of one process that takes the whole batch (equal shard sizes: the mean of the shard
means is the global mean), and with identical parameters on both ranks."""
import os
import sys
import types

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _flags():
    return types.SimpleNamespace(
        downsample=3, win_length=320, hop_length=160, n_fft=512, feature_size=80, dither=0.0,
        sample_rate=16000, lr=1e-3, gradclip=None, sub_batch_size=None, bpe_size=40,
        vocab_embed_size=8, enc_hidden_size=64, enc_layers=3, enc_dropout=0.0, enc_proj_size=24,
        dec_hidden_size=32, dec_layers=2, dec_dropout=0.0, dec_proj_size=16, joint_size=32,
        enc_time_reductions=[1], delta=False)


def _batch():
    g = torch.Generator(device="cpu").manual_seed(7)
    wave = 0.1 * torch.randn(4, 16000, generator=g)
    wlen = torch.tensor([16000, 15000, 12000, 14000], dtype=torch.int32)
    ys = torch.randint(4, 40, (4, 6), generator=g, dtype=torch.int32)
    ylen = torch.tensor([6, 5, 6, 3], dtype=torch.int32)
    return wave, wlen, ys, ylen


def _steps(eng, wave, wlen, ys, ylen, n=2):
    losses = []
    for _ in range(n):
        losses.append(eng.train_step(wave.cuda(), wlen, ys.cuda(), ylen))
    torch.cuda.synchronize()
    return [float(x) for x in losses], eng.flat.data.detach().cpu().clone()


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    os.environ["EDGEDICT_DP_MIN_BUCKET"] = "1024"        # tiny model: still one bucket per encoder layer
    from edgedict_amd.dp import shard_batch
    from edgedict_amd.trainer import TrainEngine
    torch.manual_seed(100 + rank)          # different initial weights: the engine must broadcast rank 0's
    eng = TrainEngine(_flags(), vocab_size=40, device="cuda", compute_dtype="bf16")
    shard = shard_batch(list(_batch()), rank, world)
    losses, params = _steps(eng, *shard)
    red = eng.reducer
    early = (list(red.last_early_buckets), len(red.bounds),
             [red.param_bucket[id(m.layer(0)[1])] for m in eng.model.encoder.lstm.lstms],
             red.param_bucket[id(eng.model.encoder.norm.weight)],
             red.param_bucket[id(eng.model.joint.joint[2].weight)], red.ready_calls,
             list(red.last_early_by), {n: red.param_bucket[id(p)] for n, p in eng.model.named_parameters()},
             list(red.expected))
    q.put((rank, losses, params.numpy(), early))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_equal_one_process_on_the_whole_batch(hip_lib):
    world, port = 2, 29700 + (os.getpid() % 2000)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = {}
    for _ in range(world):
        r, losses, params, early = q.get(timeout=240)
        got[r] = (losses, torch.from_numpy(params), early)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert torch.equal(got[0][1], got[1][1])                 # replicas stay identical
    # the exchange is overlapped: one bucket per encoder layer (distinct bucket ids) plus the joint's left
    # from INSIDE the backward pass (edgedict_stack_desc_t.grads_final / the joint's deferred block),
    # only the small remainder was flushed by finish()
    early, n_buckets, layer_buckets, norm_bucket, joint_bucket, ready_calls, by, names, expected = got[0][2]
    assert len(set(layer_buckets)) == 3, layer_buckets
    # the joint's block + one call per encoder layer + (round 6) the blocks whose weight gradients are deferred to the
    # auxiliary stream as well: the two projections and the two layers of the prediction network
    assert ready_calls == 8, ready_calls
    assert joint_bucket in early and all(b in early for b in layer_buckets), (early, layer_buckets)
    # top layer first: the order the BPTT finishes the layers in
    pos = [early.index(b) for b in layer_buckets]
    assert pos[2] < pos[1] < pos[0], (early, layer_buckets)
    # the encoder layers' and the joint's buckets were completed by ready() (in-place accumulation reported
    # from inside the backward pass), not by autograd hooks or finish()
    for b in layer_buckets + [joint_bucket]:
        assert by[early.index(b)] == "ready", (b, early, by)
    # the input LayerNorm's gradients are final only at the very end of the stack's backward: its bucket
    # leaves after every layer's (from finish(), or from its hook once the native call has returned)
    if norm_bucket in early:
        assert early.index(norm_bucket) > max(pos), (early, norm_bucket)
    from edgedict_amd.trainer import TrainEngine
    torch.manual_seed(100)                                    # rank 0's initial weights
    eng = TrainEngine(_flags(), vocab_size=40, device="cuda", compute_dtype="bf16")
    losses, ref = _steps(eng, *_batch())
    # mean of the shard losses = loss of the whole batch (equal shards), step by step
    for k in range(2):
        both = 0.5 * (got[0][0][k] + got[1][0][k])
        assert abs(both - losses[k]) <= 2e-2 * abs(losses[k]), (k, both, losses[k])
    diff = (got[0][1] - ref).abs().max().item()
    assert diff <= 5e-4, diff                                # two Adam steps of lr 1e-3, bf16 activations


def _run_py(code, env_extra, timeout=600):
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(env_extra)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    import json
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


_ONE_RANK = """
import json, os, sys, torch
sys.path.insert(0, %r)
import bench
from edgedict_amd import encoder_stack, side
from edgedict_amd.flags import make_flags
from edgedict_amd.trainer import TrainEngine
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
side.stream(dev)
if os.environ.get("EDGEDICT_DP_FORCE") == "1":
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    dist.init_process_group("nccl", rank=0, world_size=1)
flags = make_flags("E6D2", gradclip=None, dither=0.0)
flags.preset_name = "E6D2"
flags.sub_batch_size = 64
torch.manual_seed(0)
eng = TrainEngine(flags, device=dev, compute_dtype="bf16")
eng.spec_augment = None                      # (random masks would differ between the two processes)
data = bench.synth_batch(flags, 64, 15.0, 64, 1000, dev)
losses = [float(eng.train_step(*data)) for _ in range(2)]
torch.cuda.synchronize()
encoder_stack.check_wsr_error()              # no bounded in-kernel wait gave up (the Adam steps were applied)
red = eng.reducer
p = eng.flat.data.double()
print(json.dumps({"losses": losses, "sum": float(p.sum()), "sumsq": float((p * p).sum()),
                  "probe": [float(x) for x in eng.flat.data[::1000003][:40]],
                  "fwd_mode": encoder_stack.last_mode(False), "bwd_mode": encoder_stack.last_mode(True),
                  "early": red.last_issued_early, "buckets": len(red.bounds), "by": list(red.last_early_by)}))
sys.stdout.flush()
if os.environ.get("EDGEDICT_DP_FORCE") == "1":
    # leave in order: a process that exits with the communicator alive lets torch's watchdog thread race the
    # interpreter's teardown, and an exception on that thread aborts the process after all the work was done
    eng.close()
    dist.destroy_process_group()
"""


@pytest.mark.timeout(900)
def test_one_rank_rccl_with_the_default_kernels_equals_no_exchange(hip_lib):
    """the DEFAULT kernels (launch-persistent forward, split-K BPTT: all workgroups of a layer must be
    co-resident and wait for each other inside a launch) next to a real RCCL communicator - one rank, the only one a
    one-GPU box can host, EDGEDICT_DP_FORCE=1 so that every bucket goes through the real issue path (hooks, ready()
    from inside the backward pass on the auxiliary stream, finish()).  Full E6D2 size (B = 64 x 15 s: 256 resident
    workgroups per recurrence launch), two training steps: no give-up word, both default kernels ran, the buckets
    left during the backward pass, and the parameters equal those of the same two steps without any exchange
    (a one-rank all-reduce is the identity, 1/N = 1)."""
    from edgedict_amd import encoder_stack
    code = _ONE_RANK % ROOT
    port = 29800 + (os.getpid() % 1500)
    ex = _run_py(code, {"EDGEDICT_DP_FORCE": "1", "MASTER_PORT": str(port), "HSA_ENABLE_IPC_MODE_LEGACY": "0"})
    ref = _run_py(code, {"EDGEDICT_DP_FORCE": "0"})
    assert tuple(ex["fwd_mode"]) == (1, encoder_stack.CHUNK) and tuple(ex["bwd_mode"]) == (2, encoder_stack.CHUNK), ex
    assert ex["buckets"] >= 8 and ex["early"] >= 7 and ex["by"].count("ready") >= 7, ex
    assert ref["early"] == 0
    for a, b in zip(ex["losses"], ref["losses"]):
        assert abs(a - b) <= 1e-5 * abs(b), (ex["losses"], ref["losses"])
    # fp32 atomics in a few small products order differently from run to run: equal to ~1e-6 of the values
    assert abs(ex["sum"] - ref["sum"]) <= 1e-6 * abs(ref["sumsq"]) ** 0.5 + 1e-3, (ex["sum"], ref["sum"])
    assert abs(ex["sumsq"] - ref["sumsq"]) <= 1e-6 * ref["sumsq"], (ex["sumsq"], ref["sumsq"])
    for a, b in zip(ex["probe"], ref["probe"]):
        assert abs(a - b) <= 1e-4 * max(abs(b), 1e-3), (a, b)


@pytest.mark.timeout(900)
def test_collective_footprint_stand_in_does_not_starve_the_recurrence_launches(hip_lib):
    """32 workgroups x 512 threads x >= 128 registers streaming each layer's 34 MB gradient slice on the
    auxiliary stream at every grads_final point (what RCCL's ring kernels would occupy while the BPTT of the layers
    below runs): the training step still completes on the default kernels and no bounded wait gives up
    (tools/rccl_footprint.py raises otherwise; the table for 0 / 16 / 32 / 64 workgroups is in DESIGN 7)."""
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "rccl_footprint.py"), "0", "32"],
                       capture_output=True, text=True, timeout=840, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    import json
    rows = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert [x["workgroups"] for x in rows] == [0, 32]
    from edgedict_amd import encoder_stack
    for x in rows:
        assert tuple(x["fwd_mode"]) == (1, encoder_stack.CHUNK) and tuple(x["bwd_mode"]) == (2, encoder_stack.CHUNK), x
    assert rows[1]["footprint_launches_per_step"] >= 7, rows
    assert rows[1]["ms_per_step"] < 3.0 * rows[0]["ms_per_step"], rows

