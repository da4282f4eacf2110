"""Streaming beam search cost per chunk step on the E6D2 shape (run on the GPU box):
    python tools/stream_beam_bench.py S W dtype          e.g. 256 10 bf16
Model as tools/decode_bench.py: random weights with the blank logit biased up, so that every frame costs about the
minimum of W expansions (the regime of a trained model).  A chunk step is 2 encoder frames per stream.  Reported per
chunk step: the encoder on the chunk's stacked features with the carried (h, c); ``StreamingBeamSearch.advance`` on the
chunk's encoder output (search frames + tree compaction, one native call; the compaction kernel's share
comes from a kernel trace of this run: rocprofv3 --kernel-trace --stats -- python tools/stream_beam_bench.py ...,
kernel beam_compact); and the offline ``beam_search_rows`` over the same frames of all chunks, divided by the number of chunks, from the same process."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from edgedict_amd import decode  # noqa: E402
from edgedict_amd.flags import make_flags, model_kwargs  # noqa: E402
from edgedict_amd.models import Transducer  # noqa: E402

S = int(sys.argv[1]) if len(sys.argv) > 1 else 64
W = int(sys.argv[2]) if len(sys.argv) > 2 else 10
dtype = sys.argv[3] if len(sys.argv) > 3 else "bf16"
N = int(os.environ.get("CHUNKS", "50"))
FR = 2

flags = make_flags("E6D2")
torch.manual_seed(0)
m = Transducer(**model_kwargs(flags, vocab_size=2048)).cuda().eval()
m.compute_dtype = dtype
cd = torch.bfloat16 if dtype == "bf16" else torch.float32
with torch.no_grad():
    m.joint.joint[2].bias[0] += 12.0
I = flags.feature_size * flags.downsample
L, H = len(m.encoder.lstm.lstms), m.encoder.lstm.hidden_size


def sync():
    torch.cuda.synchronize()


with torch.no_grad():
    feats = [torch.randn(S, FR * 2, I, device="cuda") for _ in range(N)]
    # encoder per chunk step, carried state
    h = torch.zeros(L, S, H, device="cuda")
    c = torch.zeros(L, S, H, device="cuda")
    enc_out = []
    m.encoder(feats[0], (h, c))
    sync()
    t0 = time.time()
    for x in feats:
        e, (h, c) = m.encoder(x, (h, c))
        enc_out.append(e.contiguous())
    sync()
    t_enc = (time.time() - t0) / N
    P = enc_out[0].shape[2]
    enc_out = [e[:, :FR].contiguous() if e.shape[1] >= FR else e for e in enc_out]
    sb = decode.StreamingBeamSearch(m, S, W=W)
    rows = [sb.joint_rows(e) for e in enc_out]
    sb.advance_rows(rows[0], P)          # warm-up
    sb.reset()
    sync()
    t0 = time.time()
    for r in rows:
        sb.advance_rows(r, P)
    sync()
    t_adv = (time.time() - t0) / N
    t0 = time.time()
    for e in enc_out:
        sb.joint_rows(e)
    sync()
    t_e1 = (time.time() - t0) / N
    nexp = int(sb.expansions().sum())
    T = sum(r.shape[0] // S for r in rows)
    cat = torch.cat([r.reshape(S, -1, r.shape[1]) for r in rows], 1).reshape(S * T, -1).contiguous()
    decode.beam_search_rows(m, cat, S, T, P, None, W=W)
    sync()
    t0 = time.time()
    decode.beam_search_rows(m, cat, S, T, P, None, W=W)
    sync()
    t_off = (time.time() - t0) / N
    oexp = decode.beam_search_batch.last_expansions

print('{"S": %d, "W": %d, "dtype": "%s", "frames_per_chunk": %d, "chunks": %d, "encoder_us": %.1f, '
      '"joint_rows_us": %.1f, "advance_us": %.1f, "offline_us_per_chunk": %.1f, "advance_over_offline": %.3f, '
      '"expansions": %d, "offline_expansions": %d}'
      % (S, W, dtype, FR, N, t_enc * 1e6, t_e1 * 1e6, t_adv * 1e6, t_off * 1e6, t_adv / t_off, nexp, oexp))
