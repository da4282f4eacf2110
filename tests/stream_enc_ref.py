"""float64 replay of edgedict_stream_encoder_step (csrc/decode_fused.hip): the streaming decoder's encoder call on a chunk
of a few frames.  A plain restatement, composed as oracle.models_ref.encoder_forward composes it and without the output
projection: LayerNorm of the input; per layer T LSTM steps (gate order i, f, g, o in the 4H rows, both biases; i, f, o =
sigmoid, g = tanh; c' = f c + i g, h' = o tanh(c')), the layer's input added for layers > 0, LayerNorm, then
TimeReduction where the layer has one (the zero frame is appended AFTER the norm, so a lone last frame is halved).

``encoder_steps64(..., store=torch.bfloat16)`` rounds exactly where the native call stores bf16: the bf16 copy of an fp32
input, the normalised input X, the bf16 copy of the carried h (the operand of step 0), every y row (the operand of the
next step and the LayerNorm input), every LayerNorm / TimeReduction output (ONE rounding: the fused kernel keeps the
mean of the two normalised frames in fp32).  h and c stay unrounded, as in the kernels; weights are taken as given - the
caller rounds them.  With it a difference beyond a few bf16 ulps is no rounding.

``layer_steps64`` is one layer's T steps on operands as given, no LayerNorm: what the step kernels should have made of
the buffers they actually read.  It separates the two kernels from every rounding decision upstream.

``mutate`` names ONE deliberate arithmetic error (MUTATIONS); tests/test_stream_enc_ref_host.py uses them to show that the
GPU test's bounds would notice each.

CASES and ``problem`` are the shapes and seeded operands tests/test_stream_encoder_gpu.py runs on the device; they live
here so that the host test can check every one of them without a GPU.
"""
import collections

import torch

from oracle import models_ref as M

F64 = torch.float64

Replay = collections.namedtuple("Replay", "out h c T_out stored")

MUTATIONS = ("drop_x_tail", "drop_h_tail", "no_b_hh", "swap_fg", "h0_zero", "no_residual", "lone_not_halved")


def _rt(x, store):
    """x rounded to ``store`` (round-to-nearest-even, torch's cast), back in float64."""
    return x if store is None else x.to(store).to(F64)


def _d(t):
    return t.detach().to(F64)


def layer_steps64(X, w_ih, w_hh, b_ih, b_hh, h_b, c, store=None, Y_stored=None, mutate=None):
    """X [B,T,K], w_ih [4H,K], w_hh [4H,H], b_* [4H], h_b [B,H] (the operand of step 0, as given), c [B,H].
    The operand of step t > 0 is the previous h - rounded to ``store`` if given - or, with ``Y_stored`` [B,T,H], the row
    t - 1 of that buffer (a kernel's own y rows: every step is then judged on what it read).
    Returns (Y [B,T,H] unrounded h rows, h [B,H], c [B,H])."""
    X, w_ih, w_hh, b_ih, b_hh, h, c = (_d(t) for t in (X, w_ih, w_hh, b_ih, b_hh, h_b, c))
    B, T, K = X.shape
    H = w_hh.shape[1]
    assert tuple(w_ih.shape) == (4 * H, K) and tuple(w_hh.shape) == (4 * H, H) and tuple(h.shape) == tuple(c.shape) == (B, H)
    Kx = K - 8 if mutate == "drop_x_tail" else K
    Kh = H - 8 if mutate == "drop_h_tail" else H
    if mutate == "h0_zero":
        h = torch.zeros_like(h)
    ys = []
    h_exact = h
    for t in range(T):
        pre = X[:, t, :Kx] @ w_ih[:, :Kx].t() + b_ih + h[:, :Kh] @ w_hh[:, :Kh].t()
        if mutate != "no_b_hh":
            pre = pre + b_hh
        i, f, g, o = pre.split(H, dim=1)
        if mutate == "swap_fg":
            f, g = g, f
        i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
        c = f * c + i * g
        h_exact = o * torch.tanh(c)
        ys.append(h_exact)
        h = _rt(h_exact, store) if Y_stored is None else _d(Y_stored[:, t])
    return torch.stack(ys, 1), h_exact, c


def _reduce(x, lone_not_halved):
    """models_ref.time_reduction; the mutation leaves the lone last frame of an odd T as it is."""
    T = x.shape[1]
    y = M.time_reduction(x)
    if lone_not_halved and T % 2:
        y = torch.cat([y[:, :-1], x[:, -1:]], 1)
    return y


def encoder_steps64(sd, xs, hiddens=None, time_reductions=(), store=None, mutate=None):
    """sd: the encoder's parameters under the oracle's key names (encoder.norm.*, encoder.lstm.lstms.N.*,
    encoder.lstm.projs.N.0.*; a projection is not used); xs [B,T,I0]; hiddens (h, c) [L,B,H] or None (zeros).
    Returns Replay(out [B,T',H], h, c [L,B,H], T', stored) - ``stored``: name -> every buffer the native call keeps in
    bf16, as rounded here (float64 values)."""
    assert mutate is None or mutate in MUTATIONS, mutate
    p = {k: _d(v) for k, v in sd.items()}
    L = M.n_enc_layers(sd)
    stored = {}
    x = stored["input copy"] = _rt(_d(xs), store)
    x = stored["X"] = _rt(M.layer_norm(x, p["encoder.norm.weight"], p["encoder.norm.bias"]), store)
    B = x.shape[0]
    hs, cs = [], []
    for l in range(L):
        q = "encoder.lstm.lstms.%d." % l
        H = p[q + "weight_hh_l0"].shape[1]
        if hiddens is None:
            h0 = c0 = torch.zeros(B, H, dtype=F64)
        else:
            h0, c0 = _d(hiddens[0][l]), _d(hiddens[1][l])
        hb = stored["h copy %d" % l] = _rt(h0, store)
        y, h, c = layer_steps64(x, p[q + "weight_ih_l0"], p[q + "weight_hh_l0"], p[q + "bias_ih_l0"], p[q + "bias_hh_l0"],
                                hb, c0, store=store, mutate=mutate)
        y = stored["Y %d" % l] = _rt(y, store)
        x = y if l == 0 or mutate == "no_residual" else x + y
        x = M.layer_norm(x, p["encoder.lstm.projs.%d.0.weight" % l], p["encoder.lstm.projs.%d.0.bias" % l])
        if l in time_reductions:
            x = _reduce(x, mutate == "lone_not_halved")
        x = stored["act %d" % l] = _rt(x, store)
        hs.append(h)
        cs.append(c)
    return Replay(x, torch.stack(hs), torch.stack(cs), x.shape[1], stored)


# ---------------------------------------------------------------------------------------------------------------------
# the GPU test's cases: (B, T, I0, H, L, reduction layers, carried state, input dtype), each with the edge it is there for
Case = collections.namedtuple("Case", "B T I0 H L red state xdtype")
F32, BF16 = torch.float32, torch.bfloat16

CASES = collections.OrderedDict([
    # one 8-group of K: lanes kq >= 1 fully zeroed; in the tile kernel 7 of 8 chunks come from the zero block
    ("k8_step", Case(5, 1, 8, 32, 1, (), True, BF16)),
    ("k8_tile", Case(17, 1, 8, 32, 1, (), True, BF16)),
    # H = 32: the h segment is half a 64-k stage, two unit blocks
    ("h32", Case(65, 2, 40, 32, 2, (0,), True, F32)),
    # K = 40: the second 32-step is a quarter full
    ("k40", Case(16, 1, 40, 64, 1, (), False, BF16)),
    # K = 240, the first layer's real K, at the batch edges of both kernels
    ("k240_b1", Case(1, 1, 240, 64, 1, (), True, F32)),
    ("k240_b16", Case(16, 1, 240, 64, 1, (), True, F32)),
    ("k240_b17", Case(17, 1, 240, 64, 1, (), True, F32)),
    ("k240_b64", Case(64, 1, 240, 64, 1, (), True, F32)),
    ("k240_b65", Case(65, 1, 240, 64, 1, (), True, F32)),
    ("k240_b130", Case(130, 1, 240, 64, 1, (), True, F32)),
    # H = 96 (one and a half stages) and H = 160
    ("h96", Case(37, 3, 240, 96, 3, (1,), True, F32)),
    ("h160", Case(17, 2, 240, 160, 2, (0,), False, F32)),
    # second load batch of rows_product (K > 512), x side and h side
    ("k520", Case(3, 1, 520, 64, 1, (), True, BF16)),
    ("h544", Case(3, 2, 24, 544, 1, (), True, BF16)),
    # odd T under reductions, a lone last frame, a reduction on the last layer
    ("odd_t", Case(5, 5, 240, 64, 3, (0, 2), True, F32)),
    # depth
    ("deep", Case(70, 3, 240, 128, 4, (0, 2), True, F32)),
])

_PROBLEMS = {}


def make_problem(cs, seed):
    """Seeded operands of a Case: (sd, x, hiddens or None).  x has a per-row offset and spread (the mean and the variance
    of the input LayerNorm both matter) and is rounded to the case's input dtype; the LayerNorm affine parameters are away
    from (1, 0); the carried state is 0.5 * randn; the matrices are U(-1, 1) / sqrt(fan_in) with the LAST 8 COLUMNS
    multiplied by 4 - a dropped K tail cannot hide - and then rounded to bf16, the values the kernels read; the biases
    are 0.5 * randn whatever H is, so that a dropped bias cannot hide at H = 544 either."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    randn = lambda *s: torch.randn(*s, generator=g)                  # noqa: E731
    x = (randn(cs.B, cs.T, cs.I0) * (0.5 + torch.rand(cs.B, cs.T, 1, generator=g)) + randn(cs.B, cs.T, 1)).to(cs.xdtype)
    sd = {"encoder.norm.weight": 1.0 + 0.5 * randn(cs.I0), "encoder.norm.bias": 0.5 * randn(cs.I0)}
    for l in range(cs.L):
        K = cs.I0 if l == 0 else cs.H
        q = "encoder.lstm.lstms.%d." % l
        for key, fan in (("weight_ih_l0", K), ("weight_hh_l0", cs.H)):
            w = (torch.rand(4 * cs.H, fan, generator=g) * 2 - 1) / fan ** 0.5
            w[:, -8:] *= 4
            sd[q + key] = w.to(BF16).float()
        sd[q + "bias_ih_l0"] = 0.5 * randn(4 * cs.H)
        sd[q + "bias_hh_l0"] = 0.5 * randn(4 * cs.H)
        sd["encoder.lstm.projs.%d.0.weight" % l] = 1.0 + 0.5 * randn(cs.H)
        sd["encoder.lstm.projs.%d.0.bias" % l] = 0.5 * randn(cs.H)
    hid = (0.5 * randn(cs.L, cs.B, cs.H), 0.5 * randn(cs.L, cs.B, cs.H)) if cs.state else None
    return sd, x, hid


def problem(name):
    """make_problem of CASES[name], built once."""
    if name not in _PROBLEMS:
        _PROBLEMS[name] = make_problem(CASES[name], 1 + list(CASES).index(name))
    return _PROBLEMS[name]


_REPLAYS = {}


def replay(name, store=None):
    """encoder_steps64 of problem(name), computed once per (case, store); callers leave it unchanged."""
    key = (name, store)
    if key not in _REPLAYS:
        sd, x, hid = problem(name)
        _REPLAYS[key] = encoder_steps64(sd, x, hid, CASES[name].red, store=store)
    return _REPLAYS[key]


# ---------------------------------------------------------------------------------------------------------------------
# chunks of a stream: the replay chained over consecutive chunks with carried (h, c), as stream.BatchedStreamDecoder
# drives the encoder (tests/test_stream_geometry_gpu.py), and four mistakes in HOW a chunk is fed and its state carried
CHUNK_MUTATIONS = ("no_pad", "state_after_pad", "state_reset", "wrong_stride")


def kernel_weights(sd):
    """The encoder's parameters as the bf16 kernels read them: the LSTM matrices rounded to bf16, the rest as given."""
    return {k: (v.to(BF16).to(v.dtype) if k.endswith(("weight_ih_l0", "weight_hh_l0")) else v)
            for k, v in sd.items() if k.startswith("encoder.") and not k.startswith("encoder.proj.")}


def chunk_step64(sd, xs, hiddens, time_reductions=(1,), store=None, mutate=None):
    """encoder_steps64 on ONE chunk xs [B,T0,I0] with the carried ``hiddens``, or with one mistake:

    no_pad           an odd frame count under a time reduction is not zero-padded: the lone last frame leaves the
                     reduction as it is instead of as its mean with a zero frame (the encoder_steps64 mutation
                     'lone_not_halved'); the reference pads inside every chunk (rnnt/models.py TimeReduction)
    state_after_pad  the chunk is padded to an even frame count at its INPUT, so that the layers up to the first time
                     reduction run one step more than the chunk has frames: their carried (h, c) is the state after the
                     pad frame, not after the last real one.  The chunk's own output is left right - only the next
                     chunk sees it
    state_reset      the carried state is dropped: the chunk starts from zeros
    wrong_stride     stacked frame t is read at t * (I0 - 8) of the row instead of t * I0
    Returns a Replay."""
    assert mutate is None or mutate in CHUNK_MUTATIONS, mutate
    B, T0, I0 = xs.shape
    if mutate == "state_reset":
        hiddens = None
    if mutate == "wrong_stride":
        flat = xs.reshape(B, T0 * I0)
        xs = torch.stack([flat[:, t * (I0 - 8):t * (I0 - 8) + I0] for t in range(T0)], 1)
    good = encoder_steps64(sd, xs, hiddens, time_reductions, store=store, mutate="lone_not_halved" if mutate == "no_pad" else None)
    if mutate == "state_after_pad" and T0 % 2 and len(time_reductions):
        padded = encoder_steps64(sd, torch.cat([xs, torch.zeros_like(xs[:, :1])], 1), hiddens, time_reductions, store=store)
        upto = min(time_reductions) + 1
        good = good._replace(h=torch.cat([padded.h[:upto], good.h[upto:]]), c=torch.cat([padded.c[:upto], good.c[upto:]]))
    return good


def chunk_mutation_applies(mutation, T0, n_chunks):
    """Is the mistake one at all for chunks of T0 frames (one time reduction)?"""
    return {"no_pad": T0 % 2 == 1, "state_after_pad": T0 % 2 == 1 and n_chunks > 1, "state_reset": n_chunks > 1,
            "wrong_stride": T0 > 1}[mutation]


def chain64(sd, chunks, time_reductions=(1,), store=None, mutate=None):
    """chunk_step64 over ``chunks`` (a list of [B,T0,I0]), each fed the (h, c) the previous one returned, from zeros.
    Returns the list of Replays."""
    out, hid = [], None
    for xs in chunks:
        r = chunk_step64(sd, xs, hid, time_reductions, store=store, mutate=mutate)
        out.append(r)
        hid = (r.h, r.c)
    return out
