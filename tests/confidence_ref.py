"""ORACLE (test infrastructure only) of the confidence pass (csrc/confidence.hip; loss.row_confidence,
decode.confidence_measure, decode.hypothesis_confidence): the five row statistics and the four measures restated in
numpy, the teacher-forced replay of N-best lists on tests/search_ref.py's network, the inputs of the row-kernel test,
and the bounds the GPU test applies.  tests/test_confidence_host.py pins all of it without a GPU.

Row statistics of logits z [V] and a token k, in the kernel's form (``row_stats``; ``dtype=np.float32`` evaluates the
same expressions in fp32 numpy - the restatement whose error against fp64 scales the GPU bounds on H and log sum p^a):
    m = max z;  s = sum e^(z - m);  a = sum e^(z - m) (z - m);  q = sum e^(alpha (z - m))      (-inf logits add 0)
    logp = (z[k] - m) - log s;  logp_max = -log s;  logp_blank = (z[blank] - m) - log s;  H = log s - a / s;
    log sum p^alpha = log q - alpha log s;  top = first arg max
``measures_direct`` forms the measures from the softmax itself, not from the statistics: an independent second route.

The replay (``replay_logits``): for a hypothesis (tokens, frames) of utterance b the prediction network reads BOS +
tokens from a zero state (search_ref.pred_step), row u is its output after y_<u, and the joint is evaluated on
E1[b, frames[u]] (search_ref.joint_logits).  ``cd=None``: float64 throughout, weights as given.  ``cd=torch.float32``: the
same replay in float32 arithmetic - an fp32 kernel holds fp32 everywhere, registers included.  ``cd=torch.bfloat16``:
float64 arithmetic on weights rounded to bf16, rounded to bf16 where the kernels store bf16 (search_ref's storage points
with ``round_g``: embedding row, gate pre-activations, h as an operand, layer outputs, dec_out; E1, the first product with
its bias, hid), the logits rounded to fp32.  The rounded replays take their statistics from the fp32 restatement.

ERR (``err``; measured by tests/test_confidence_host.py, on this CPU, torch 2.x; largest |rounded - exact| per statistic
over the token rows of the oracle's lists - ``oracle_lists``: sync_beam_ref.search, W = 4, blank_bias 1.0 -
columns logp / logp_max / logp_blank / H / log sum p^alpha at alpha = 1/3):
    CFG    fp32  3.3e-07  3.3e-07  3.8e-07  3.0e-07  3.1e-07      bf16  3.8e-03  3.8e-03  7.4e-03  1.2e-03  2.7e-04
    CFG32  fp32  3.7e-07  3.7e-07  3.5e-07  2.5e-07  1.5e-07      bf16  3.1e-03  3.1e-03  4.6e-03  7.4e-04  1.3e-04
    CFGV   fp32  1.1e-06  1.1e-06  4.7e-07  6.2e-07  5.0e-07      bf16  3.4e-03  3.4e-03  3.6e-03  5.1e-04  1.1e-04
(44, 55 and 57 token rows; the fp64 replay reproduces the oracle's own token_logp within 3.5e-7, 3.7e-7 and 4.2e-7.)
The GPU bound of the end-to-end test is 3 x ERR, the project's margin for such replays (tests/search_ref.py bounds):
the device shares the replay's storage points and differs by summation order and its exp / tanh / log, each far
below one rounding of the storage format but able to move a value across a rounding boundary."""
import collections
import functools

import numpy as np
import torch

import search_ref as R
import sync_beam_ref as S
from oracle import models_ref as M

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
ALPHA = 1.0 / 3.0
MIN_MARGIN = 2e-3
COLUMNS = ("logp", "logp_max", "logp_blank", "entropy", "log_sum_p_alpha")
# the docstring's figures as a table; tests/test_confidence_host.py measures them again and fails when one has moved by
# more than a small factor.  The GPU test multiplies err() itself - the live measurement - by 3.
ERR_TABLE = {
    ("CFG", "fp32"): (3.3e-07, 3.3e-07, 3.8e-07, 3.0e-07, 3.1e-07),
    ("CFG", "bf16"): (3.8e-03, 3.8e-03, 7.4e-03, 1.2e-03, 2.7e-04),
    ("CFG32", "fp32"): (3.7e-07, 3.7e-07, 3.5e-07, 2.5e-07, 1.5e-07),
    ("CFG32", "bf16"): (3.1e-03, 3.1e-03, 4.6e-03, 7.4e-04, 1.3e-04),
    ("CFGV", "fp32"): (1.1e-06, 1.1e-06, 4.7e-07, 6.2e-07, 5.0e-07),
    ("CFGV", "bf16"): (3.4e-03, 3.4e-03, 3.6e-03, 5.1e-04, 1.1e-04),
}


# --------------------------------------------------------------------------------------------------- row statistics
def row_stats(z, tokens, alpha=ALPHA, blank=M.NUL, dtype=np.float64):
    """z [R, V] (numpy, any float dtype) -> (stats [R, 5] float64, top [R] int64, gap [R]): every expression evaluated
    in ``dtype``.  ``gap``: largest minus second-largest logit (inf for V = 1 finite rows, NaN for a dead row).  A row
    holding a NaN or nothing above -inf gives NaN statistics and top -1; a token outside [0, V) NaN in logp only."""
    z = np.asarray(z).astype(dtype)
    Rn, V = z.shape
    al = dtype(alpha)
    stats = np.full((Rn, 5), np.nan, dtype=np.float64)
    top = np.full(Rn, -1, dtype=np.int64)
    gap = np.full(Rn, np.nan, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        for r in range(Rn):
            x = z[r]
            if np.isnan(x).any() or not (x > -np.inf).any():
                continue
            top[r] = int(np.argmax(x))
            m = x[top[r]]
            rest = np.delete(x, top[r])
            gap[r] = float(m) - float(rest.max())
            live = x[x > -np.inf]
            t = (live - m).astype(dtype)
            e = np.exp(t).astype(dtype)
            s = e.sum(dtype=dtype)
            a = (e * t).astype(dtype).sum(dtype=dtype)
            q = np.exp((al * t).astype(dtype)).astype(dtype).sum(dtype=dtype)
            ls = np.log(s).astype(dtype)
            k = int(tokens[r])
            if 0 <= k < V:
                stats[r, 0] = dtype(dtype(x[k] - m) - ls)
            stats[r, 1] = dtype(-ls)
            stats[r, 2] = dtype(dtype(x[blank] - m) - ls)
            stats[r, 3] = dtype(ls - dtype(a / s))
            stats[r, 4] = dtype(np.log(q).astype(dtype) - dtype(al * ls))
    return stats, top, gap


def measure(stats, V, method, alpha=ALPHA):
    """decode.confidence_measure restated."""
    stats = np.asarray(stats, dtype=np.float64)
    c = {"prob": lambda: np.exp(stats[..., 0]), "max_prob": lambda: np.exp(stats[..., 1]),
         "entropy": lambda: 1.0 - stats[..., 3] / np.log(V),
         "tsallis": lambda: 1.0 - (1.0 - np.exp(stats[..., 4])) / (1.0 - float(V) ** (1.0 - alpha))}[method]()
    return np.minimum(np.maximum(c, 0.0), 1.0)


def measures_direct(z, tokens, alpha=ALPHA):
    """The four measures from the softmax p itself (float64): dict method -> [R].  Rows must be live."""
    z = np.asarray(z, dtype=np.float64)
    V = z.shape[1]
    p = np.exp(z - z.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        H = -np.where(p > 0, p * np.log(p), 0.0).sum(axis=1)
    tsallis = (1.0 - np.where(p > 0, p ** alpha, 0.0).sum(axis=1))
    out = {"prob": p[np.arange(len(z)), np.asarray(tokens)], "max_prob": p.max(axis=1),
           "entropy": 1.0 - H / np.log(V), "tsallis": 1.0 - tsallis / (1.0 - float(V) ** (1.0 - alpha))}
    return {k: np.clip(v, 0.0, 1.0) for k, v in out.items()}


# ------------------------------------------------------------------------------------ inputs of the row-kernel test
KERNEL_V = (2, 63, 64, 65, 256, 2112)
KERNEL_R = (1, 3, 4, 5, 9)


@functools.lru_cache(maxsize=None)
def kernel_rows(V, Rn, bf16=False):
    """(z float32 [Rn, V], tokens int32 [Rn]) of one case; with ``bf16`` the values are bf16-representable.  Row r mod 4:
    0 a peaked row (normal x 3, one symbol raised by 6), 1 a flat row (normal x 0.3, one symbol raised by 1) with every
    third logit -inf, 2 a row spanning -80 .. +80 with a winner 2 above the next, 3 a peaked row whose token is the
    arg max.  Every row has a clear winner: the top-two gap stays far above MIN_MARGIN, bf16 rounding included."""
    g = torch.Generator().manual_seed(1000 * V + 10 * Rn + int(bf16))
    z = torch.randn(Rn, V, generator=g)
    tokens = torch.randint(0, V, (Rn,), generator=g, dtype=torch.int32)
    for r in range(Rn):
        kind, win = r % 4, int(torch.randint(0, V, (1,), generator=g))
        if kind in (0, 3):
            z[r] *= 3.0
            z[r, win] = z[r].max() + 6.0
        elif kind == 1:
            z[r] *= 0.3
            z[r, win] = z[r].max() + 1.0
            dead = torch.arange(V) % 3 == 2
            dead[win] = False
            if V > 2:
                z[r, dead] = -float("inf")
        else:
            z[r] = torch.linspace(-80.0, 78.0, V)[torch.randperm(V, generator=g)]
            z[r, win] = 80.0
        if kind == 3:
            tokens[r] = win
    if bf16:
        z = z.to(BF16).to(F32)
    return z.numpy(), tokens.numpy()


def kernel_bounds(z, tokens, alpha=ALPHA):
    """(exact stats, top, gap, bound [5]) of a case: the log-prob columns at the project's 1e-5 for this arithmetic form
    (rtol = atol, tests/test_ilme_gpu.py), H and log sum p^alpha at 4 x the fp32 restatement's error on these inputs
    (the 4 pays for the kernel's other summation order), never below 1e-5."""
    exact, top, gap = row_stats(z, tokens, alpha)
    f32, _, _ = row_stats(z, tokens, alpha, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        d = np.abs(f32 - exact)
    d = np.where(np.isnan(d), 0.0, d).max(axis=0)
    return exact, top, gap, np.array([1e-5, 1e-5, 1e-5, max(1e-5, 4 * d[3]), max(1e-5, 4 * d[4])])


# ------------------------------------------------------------------------------------------------------ the replay
def _arith_net(sd, P, cd):
    """search_ref.Net in the replay's arithmetic dtype: float32 for cd = fp32, else float64 (bf16: rounded weights)."""
    if cd == F32:
        net = R.net_from_sd(sd, P)
        cast = lambda v: [w.to(F32) for w in v] if isinstance(v, list) else (v.to(F32) if torch.is_tensor(v) else v)  # noqa
        return R.Net(*[cast(v) for v in net])
    return R.net_from_sd(sd, P, cd)


def replay_logits(sd, enc, lists, cd=None):
    """enc [B, T, P] (the encoder output the pass is given, any dtype) and ``lists[b]`` = [(tokens, frames), ...] ->
    list over b of lists of logits [len, V] (numpy float64), as the module docstring states."""
    P = enc.shape[2]
    net = _arith_net(sd, P, cd)
    ar = F32 if cd == F32 else F64
    store = BF16 if cd == BF16 else None
    w1e = sd["joint.joint.0.weight"][:, :P]
    w1e = (w1e if store is None else w1e.to(store)).to(ar)
    L, H = len(net.w_hh), net.w_hh[0].shape[1]
    out = []
    for b, hyps in enumerate(lists):
        E1 = R._rt(R._rt(enc[b].to(ar), store) @ w1e.t(), store)
        rows = []
        for tokens, frames in hyps:
            h = c = torch.zeros(L, 1, H, dtype=ar)
            decs = []
            for tok in [M.BOS] + [int(k) for k in tokens][:-1]:
                dec, h, c = R.pred_step(net, np.array([tok]), h, c, store, store is not None)
                decs.append(dec[0])
            if not decs or not len(tokens):
                rows.append(np.zeros((0, net.W2.shape[0])))
                continue
            z = R.joint_logits(net, E1[torch.as_tensor(np.asarray(frames), dtype=torch.long)], torch.stack(decs), store)
            if store is not None:
                z = z.to(F32)
            rows.append(z.to(F64).numpy())
        out.append(rows)
    return out


def replay_stats(sd, enc, lists, cd=None, alpha=ALPHA):
    """(stats, top, gap) per utterance and hypothesis of ``replay_logits``: float64 restatement for cd None, the fp32
    one for a rounded replay."""
    dtype = np.float64 if cd is None else np.float32
    return [[row_stats(z, t, alpha, dtype=dtype) if len(t) else (np.zeros((0, 5)), np.zeros(0, np.int64), np.zeros(0))
             for z, (t, _) in zip(rows, hyps)] for rows, hyps in zip(replay_logits(sd, enc, lists, cd), lists)]


# ------------------------------------------------------------------------------------------- the oracle's lists
def _inputs(name, blank_bias):
    from test_sync_beam_gpu import _inputs as inputs
    return inputs(name, blank_bias=blank_bias)


@functools.lru_cache(maxsize=None)
def oracle_lists(name, blank_bias=1.0, W=4):
    """(sd, xs, xlen, h_enc [B, T, P] fp32, lens, ranked lists of sync_beam_ref.search): computed once, read only."""
    sd, xs, xlen = _inputs(name, blank_bias)
    h_enc, lens = S.encode(sd, xs, xlen)
    res, _ = S.search(sd, xs, xlen, W)
    return sd, xs, xlen, h_enc, lens, res


def pairs(res):
    """The oracle's ranked lists as ``replay_logits`` takes them."""
    return [[(h["tokens"], h["frames"]) for h in r] for r in res]


@functools.lru_cache(maxsize=None)
def exact_stats(name, blank_bias=1.0, W=4):
    sd, _, _, h_enc, _, res = oracle_lists(name, blank_bias, W)
    return replay_stats(sd, h_enc, pairs(res))


def _flat(per_utt, k):
    a = [h[k] for u in per_utt for h in u if len(h[k])]
    return np.concatenate(a) if a else np.zeros((0, 5) if k == 0 else 0)


@functools.lru_cache(maxsize=None)
def err(name, dtype):
    """ERR [5] of a config and ``dtype`` ("fp32" / "bf16"): module docstring."""
    sd, _, _, h_enc, _, res = oracle_lists(name)
    cd = F32 if dtype == "fp32" else BF16
    rounded = replay_stats(sd, h_enc.to(cd), pairs(res), cd)
    # the exact side sees what the rounded side was given: the encoder output as stored in cd
    exact = replay_stats(rounded_sd(sd, cd), h_enc.to(cd), pairs(res))
    return np.abs(_flat(rounded, 0) - _flat(exact, 0)).max(axis=0)


def rounded_sd(sd, cd):
    """The state dict as decode._SearchNet hands it to the kernels: matrices in ``cd``, biases and the embedding fp32."""
    if cd == F32:
        return sd
    keep = ("bias", "embed.weight", "norm")
    return {k: (v if any(s in k for s in keep) or v.dim() < 2 else v.to(cd).to(F32)) for k, v in sd.items()}


Wrapped = collections.namedtuple("Wrapped", "results lists")


def wrapped(name):
    """The oracle's lists as decode.NBestResult objects (the engine's own class): no search decision is involved."""
    from edgedict_amd.decode import NBestResult
    _, _, _, _, _, res = oracle_lists(name)
    out = [NBestResult([np.asarray(h["tokens"], dtype=np.int64) for h in r],
                       [np.asarray(h["frames"], dtype=np.int32) for h in r],
                       [np.asarray(h["token_logp"], dtype=np.float64) for h in r], [h["logp"] for h in r]) for r in res]
    return Wrapped(out, pairs(res))
