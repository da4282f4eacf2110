"""Cost of LM shallow fusion in the beam searches on the E6D2 shape (run on the GPU box):
    python tools/lm_beam_bench.py B W dtype LM_H          e.g. 64 10 bf16 1024
Model as tools/stream_beam_bench.py: random E6D2 weights (vocabulary 1024, the BPE size cli/train_lm.py's LM uses)
with the blank logit biased up, so that every frame costs the minimum of W pops per utterance and the lockstep
iterations are T x W.  The LM is LMModel(1024, 64, LM_H, 2) (cli/train_lm.py:47 has LM_H = 1024) with random weights;
weight 0.3, no length bonus (the fused children only lose score, so the pops do not change).  Reported: the offline
search (beam_search_rows over T frames of B utterances) and the streaming search (StreamingBeamSearch.advance over
chunks of 2 frames for B streams) with and without the LM, as us per lockstep iteration (call time / (frames x pops per
frame)).  The added launches' breakdown comes from a kernel trace of this run:
    rocprofv3 --kernel-trace --stats -- python tools/lm_beam_bench.py ..."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from edgedict_amd import decode  # noqa: E402
from edgedict_amd.flags import make_flags, model_kwargs  # noqa: E402
from edgedict_amd.lm import LMModel  # noqa: E402
from edgedict_amd.models import Transducer  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
W = int(sys.argv[2]) if len(sys.argv) > 2 else 10
dtype = sys.argv[3] if len(sys.argv) > 3 else "bf16"
LM_H = int(sys.argv[4]) if len(sys.argv) > 4 else 1024
T = int(os.environ.get("FRAMES", "40"))
V = 1024

flags = make_flags("E6D2")
torch.manual_seed(0)
m = Transducer(**model_kwargs(flags, vocab_size=V)).cuda().eval()
m.compute_dtype = dtype
cd = torch.bfloat16 if dtype == "bf16" else torch.float32
with torch.no_grad():
    m.joint.joint[2].bias[0] += 12.0
lm = LMModel(V, 64, LM_H, 2, dropout=0.0).cuda().eval()
for p in lm.parameters():
    p.requires_grad_(False)
P = m.joint.joint[0].weight.shape[1] - m.decoder.proj.weight.shape[0]
fuse = dict(lm=lm, lm_weight=0.3, length_bonus=0.0)


def sync():
    torch.cuda.synchronize()


def offline(E1, **kw):
    decode.beam_search_rows(m, E1, B, T, P, None, W=W, **kw)          # warm-up (workspace, weight copies)
    sync()
    t0 = time.time()
    decode.beam_search_rows(m, E1, B, T, P, None, W=W, **kw)
    sync()
    return time.time() - t0, decode.beam_search_batch.last_expansions


def streaming(rows, **kw):
    sb = decode.StreamingBeamSearch(m, B, W=W, **kw)
    sb.advance_rows(rows[0], P)
    sb.reset()
    sync()
    t0 = time.time()
    for r in rows:
        sb.advance_rows(r, P)
    sync()
    return time.time() - t0, int(sb.expansions().sum())


with torch.no_grad():
    enc = torch.randn(B, T, P, device="cuda").to(cd)
    E1 = decode.joint_rows(m, enc)
    rows = [decode.joint_rows(m, enc[:, t:t + 2].contiguous()) for t in range(0, T, 2)]
    res = {}
    for name, kw in (("plain", {}), ("lm", fuse)):
        t_off, e_off = offline(E1, **kw)
        t_str, e_str = streaming(rows, **kw)
        # lockstep iterations = frames x pops per frame (every utterance pops the same number when blank dominates)
        it_off = e_off / B
        it_str = e_str / B
        res[name] = (t_off, e_off, t_off / it_off * 1e6, t_str, e_str, t_str / it_str * 1e6)

print('{"B": %d, "W": %d, "dtype": "%s", "lm_H": %d, "frames": %d, '
      '"offline_ms": [%.2f, %.2f], "offline_expansions": [%d, %d], "offline_us_per_iter": [%.1f, %.1f], '
      '"stream_ms": [%.2f, %.2f], "stream_expansions": [%d, %d], "stream_us_per_iter": [%.1f, %.1f], '
      '"lm_over_plain_offline": %.3f, "lm_over_plain_stream": %.3f}'
      % (B, W, dtype, LM_H, T, res["plain"][0] * 1e3, res["lm"][0] * 1e3, res["plain"][1], res["lm"][1],
         res["plain"][2], res["lm"][2], res["plain"][3] * 1e3, res["lm"][3] * 1e3, res["plain"][4], res["lm"][4],
         res["plain"][5], res["lm"][5], res["lm"][2] / res["plain"][2], res["lm"][5] / res["plain"][5]))
