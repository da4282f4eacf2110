"""CPU: the float64 replay of the streaming encoder step (tests/stream_enc_ref.py) chained over the chunks of a stream, at
the chunk shapes tests/test_stream_geometry_gpu.py runs on the device: T0 in {1, 3, 13} stacked frames of I0 in {80, 160,
320} features, 3 chunks with carried (h, c), the body of oracle.make_golden_stream.SMALL (H = 64, 3 layers, the time
reduction behind layer 1) with seeded weights, the LSTM matrices rounded to bf16 as the kernels read them.  The inputs are
real chunks: the oracle's stacked log-mel features (oracle.features_ref) of seeded noise, consecutive in time.

(a) the bf16-rounded replay stays inside the GPU test's bound, BF16_TOL = 2e-2 of the buffer's max, of the exact float64
replay - output, last output frame (the zero-padded pair at odd T0), h and c, after every chunk, each chain carrying its
own state; (b) each of four mistakes in how a chunk is fed or its state carried (stream_enc_ref.CHUNK_MUTATIONS) moves
one of them beyond that bound at every shape where it is a mistake at all.  So at these shapes the bound is not used up
by the reference and is not slack either.

Measured (printed with -s), error / max(|ref|, 1e-3):
  (a) worst over the nine shapes and three chunks: out 1.43e-2 and h 1.49e-2 (both T0 3, I0 320), last frame 9.8e-3,
      c 9.3e-3 (bound 2e-2; each chain runs free, so chunk 2 holds three chunks of rounding)
  (b) smallest movement over the shapes where the mistake applies: no_pad 0.19 (T0 13, I0 320), state_after_pad 0.48,
      state_reset 0.45, wrong_stride 1.40 - 9 to 70 times the bound."""
import pytest
import torch

import stream_enc_ref as R
from oracle import features_ref as Fr
from oracle import models_ref as M
from oracle.make_golden_stream import SMALL

BF16 = torch.bfloat16
BF16_TOL = 2e-2              # tests/test_stream_encoder_gpu.py
SHAPES = [(T0, I0) for T0 in (1, 3, 13) for I0 in (80, 160, 320)]
N_CHUNKS, B, HOP = 3, 3, 160

_PROBLEMS = {}


def _problem(T0, I0):
    """(sd as the kernels read it, [chunk 0, 1, 2] of [B, T0, I0] float64), built once."""
    if (T0, I0) not in _PROBLEMS:
        ds = I0 // 80
        sd = R.kernel_weights(M.make_state_dict(dict(SMALL, input_size=I0), 40 + T0))
        g = torch.Generator(device="cpu").manual_seed(1000 * T0 + I0)
        wave = 0.1 * torch.randn(B, HOP * ds * T0 * N_CHUNKS + 512, generator=g)
        xs = Fr.stacked_features(wave, ds, False, win_length=320, hop_length=HOP, n_fft=512, n_filt=80)
        assert xs.shape[1] >= T0 * N_CHUNKS and xs.shape[2] == I0
        _PROBLEMS[T0, I0] = (sd, [xs[:, c * T0:(c + 1) * T0].double().contiguous() for c in range(N_CHUNKS)])
    return _PROBLEMS[T0, I0]


def _rel(a, b):
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-3)


def _views(r):
    return (("out", r.out), ("last frame", r.out[:, -1]), ("h", r.h), ("c", r.c))


@pytest.mark.parametrize("T0,I0", SHAPES)
def test_rounded_chain_stays_inside_the_gpu_bound_of_the_exact_chain(T0, I0):
    sd, chunks = _problem(T0, I0)
    exact, rounded = R.chain64(sd, chunks), R.chain64(sd, chunks, store=BF16)
    worst = {}
    for c, (e, r) in enumerate(zip(exact, rounded)):
        assert r.T_out == e.T_out == (T0 + 1) // 2 and tuple(r.out.shape) == (B, (T0 + 1) // 2, 64)
        for (key, a), (_, b) in zip(_views(r), _views(e)):
            worst[key] = max(worst.get(key, 0.0), _rel(a, b))
    # the carried state matters: chunk 1 from zeros is another result
    assert _rel(R.chunk_step64(sd, chunks[1], None).out, exact[1].out) > BF16_TOL
    print("\nstream chunks T0 %d I0 %d rounded vs exact: %s" % (T0, I0, ", ".join("%s %.2e" % kv for kv in worst.items())))
    for key, v in worst.items():
        assert v <= BF16_TOL, (T0, I0, key, v)


@pytest.mark.parametrize("mutation", R.CHUNK_MUTATIONS)
def test_every_chunk_mistake_overshoots_the_gpu_bound(mutation):
    """Rounded chain with the mistake against the rounded chain without it, as the GPU test compares a device result with
    the rounded replay: the worst of out, last frame, h and c over the three chunks must exceed BF16_TOL at EVERY shape
    where the mistake changes anything - an odd T0 for the two pad mistakes, T0 > 1 for the stride."""
    hit = []
    for T0, I0 in SHAPES:
        if not R.chunk_mutation_applies(mutation, T0, N_CHUNKS):
            continue
        sd, chunks = _problem(T0, I0)
        ref = R.chain64(sd, chunks, store=BF16)
        mut = R.chain64(sd, chunks, store=BF16, mutate=mutation)
        moved = max(_rel(a, b) for m, r in zip(mut, ref) for (_, a), (_, b) in zip(_views(m), _views(r)))
        print("\nstream chunks T0 %d I0 %d with %s: moved by %.2f of the scale" % (T0, I0, mutation, moved))
        assert moved > BF16_TOL, (T0, I0, mutation, moved)
        hit.append((T0, I0))
    need = {"no_pad": 9, "state_after_pad": 9, "state_reset": 9, "wrong_stride": 6}[mutation]
    assert len(hit) == need, (mutation, hit)
