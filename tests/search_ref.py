"""float64 replay of one search call of csrc/decode_fused.hip / csrc/decode.hip (``edgedict_greedy_decode``: the greedy
search, and with ``unk >= 0`` the stream decoder's frame), and of the lattice a beam hypothesis is scored on.

Per frame t, as the header of decode_fused.hip states it:
    hid = tanh(E1[:, t] + act(dec_out W1d^T + b1));  z = hid W2^T + b2
    pick = first arg-max of z; with unk >= 0 and pick == unk the stream decoder's retake rule: the <unk> logit counts as 0
           and the arg-max is retaken (<unk> stays iff every other logit is below 0, or equals 0 at a higher index);
           a row without one comparable logit emits blank
    score increment = logsumexp(z) - max z
    prediction-network step on the pick: embedding, L LSTM layers (gate order i, f, g, o; both biases), projection
    dec_out, h, c are replaced only where the pick is not blank.

A bf16 search feeds its own picks back, so one near-tie makes every later frame differ from a free-running reference.
``forced`` [B, T] therefore replaces the replay's own picks as what the prediction network consumes and what decides the
commit: the prediction network's state is a function of the token history alone, so a replay forced onto the device's
tokens knows the logits the device should have seen on EVERY frame, and each pick, each score increment and the final
state can be judged on its own.  The replay's own pick (its rule applied to its logits) is still reported per frame.

``store=torch.bfloat16`` rounds where the kernels hold bf16: the ``act(...)`` of the joint's first product, ``hid``, the
embedding row and the carried h as operands of the gate products (the kernels convert both to bf16 fragments on load; the
fp32 h and c themselves stay unrounded), the layer outputs y between the layers and into the projection, ``dec_out``.
``round_g=True`` adds the one rounding the composed path (decode.hip, general kernels) has on top: the input half of the
gate pre-activations, x W_ih^T + b_ih + b_hh, passes through a bf16 buffer before h W_hh^T is added.  The logits and the
score stay unrounded (fp32 on the device).  Weights are taken as given - the caller hands over the converted ones.

``mutate`` names ONE deliberate arithmetic error (MUTATIONS); tests/test_search_ref_host.py uses them to show that the
bounds of tests/test_search_kernels_gpu.py would notice each.  CASES, ``problem`` and ``bounds`` are what the GPU test
runs; they live here so that the host test can judge every case without a GPU.
"""
import collections

import numpy as np
import torch

from oracle import models_ref as M

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16

Net = collections.namedtuple("Net", "W1d b1 W2 b2 emb w_ih w_hh b_ih b_hh Wp bp blank")
Replay = collections.namedtuple("Replay", "logits pick gap margin inc dec h c fired kept")

DROPS = ("drop_w1d", "drop_w2", "drop_ih", "drop_hh", "drop_wp")           # the last 32 of K of one product
MUTATIONS = DROPS + ("commit_on_blank", "no_commit", "ties_high", "unk_always_ax", "score_second")


def _rt(x, store):
    """x rounded to ``store`` (round-to-nearest-even, torch's cast), back in float64."""
    return x if store is None else x.to(store).to(F64)


def _d(t):
    return t.detach().to(device="cpu", dtype=F64)


def make_net(W1d, b1, W2, b2, emb, w_ih, w_hh, b_ih, b_hh, Wp, bp, blank=M.NUL):
    """A Net of float64 CPU copies of the operands as given (any dtype, any device)."""
    return Net(_d(W1d), _d(b1), _d(W2), _d(b2), _d(emb), [_d(w) for w in w_ih], [_d(w) for w in w_hh],
               [_d(b) for b in b_ih], [_d(b) for b in b_hh], _d(Wp), _d(bp), int(blank))


def net_from_sd(sd, P, cd=None, emb_dtype=None, blank=M.NUL):
    """The Net of a state dict for an encoder output of width P: the matrices rounded to the compute dtype ``cd`` (None:
    as they are), the embedding table to ``emb_dtype``, the biases fp32 - what decode._SearchNet hands to the kernels."""
    c = (lambda w: w) if cd is None else (lambda w: w.to(cd))
    L = M.n_dec_layers(sd)
    emb = sd["decoder.embed.weight"]
    return make_net(c(sd["joint.joint.0.weight"])[:, P:], sd["joint.joint.0.bias"], c(sd["joint.joint.2.weight"]),
                    sd["joint.joint.2.bias"], emb if emb_dtype is None else emb.to(emb_dtype),
                    [c(sd["decoder.lstm.weight_ih_l%d" % k]) for k in range(L)],
                    [c(sd["decoder.lstm.weight_hh_l%d" % k]) for k in range(L)],
                    [sd["decoder.lstm.bias_ih_l%d" % k] for k in range(L)],
                    [sd["decoder.lstm.bias_hh_l%d" % k] for k in range(L)],
                    c(sd["decoder.proj.weight"]), sd["decoder.proj.bias"], blank)


def _k(K, mutate, which):
    return K - 32 if mutate == which else K


def joint_logits(net, e1, dec, store=None, mutate=None):
    """e1 [B, J] (the joint's encoder rows of one frame), dec [B, P2] -> logits [B, V]."""
    k1 = _k(net.W1d.shape[1], mutate, "drop_w1d")
    a = _rt(dec[:, :k1] @ net.W1d[:, :k1].t() + net.b1, store)
    hid = _rt(torch.tanh(e1 + a), store)
    kj = _k(net.W2.shape[1], mutate, "drop_w2")
    return hid[:, :kj] @ net.W2[:, :kj].t() + net.b2


def pred_step(net, tok, h, c, store=None, round_g=False, mutate=None):
    """One prediction-network step on the symbols ``tok`` [B] from (h, c) [L, B, H]: (dec_new [B, P2], h_new, c_new).
    A symbol outside the table is clamped into it, as the kernels clamp."""
    V = net.emb.shape[0]
    x = _rt(net.emb[torch.as_tensor(np.asarray(tok), dtype=torch.long).clamp(0, V - 1)], store)
    hs, cs = [], []
    for l in range(len(net.w_ih)):
        H = net.w_hh[l].shape[1]
        kx, kh = _k(net.w_ih[l].shape[1], mutate, "drop_ih"), _k(H, mutate, "drop_hh")
        g_in = x[:, :kx] @ net.w_ih[l][:, :kx].t() + net.b_ih[l] + net.b_hh[l]
        if round_g:
            g_in = _rt(g_in, store)
        pre = g_in + _rt(h[l], store)[:, :kh] @ net.w_hh[l][:, :kh].t()
        i, f, g, o = pre.split(H, dim=1)
        cn = torch.sigmoid(f) * c[l] + torch.sigmoid(i) * torch.tanh(g)
        hn = torch.sigmoid(o) * torch.tanh(cn)
        hs.append(hn)
        cs.append(cn)
        x = _rt(hn, store)
    kp = _k(net.Wp.shape[1], mutate, "drop_wp")
    dec = _rt(x[:, :kp] @ net.Wp[:, :kp].t() + net.bp, store)
    return dec, torch.stack(hs), torch.stack(cs)


def _first_argmax(z, high=False):
    """numpy's arg-max returns the FIRST maximum; ``high``: the last one (the ties_high mutation)."""
    if high:
        return z.shape[1] - 1 - np.argmax(z[:, ::-1], axis=1)
    return np.argmax(z, axis=1)


def pick_rows(z, unk=-1, blank=M.NUL, mutate=None):
    """z [B, V] float64 numpy -> dict of [B] arrays: ``pick``; ``gap`` = largest minus second-largest logit; ``margin`` =
    the smallest difference the pick depends on (``gap``, and where the <unk> rule fired also |best other logit - 0| and,
    if <unk> was replaced, the gap between the two best others); ``second`` = the second-largest logit; ``fired`` /
    ``kept``: the arg-max was <unk> / and stayed."""
    with np.errstate(invalid="ignore"):            # (rows of NaN or -inf: inf - inf)
        return _pick_rows(z, unk, blank, mutate)


def _pick_rows(z, unk, blank, mutate):
    B, V = z.shape
    rows = np.arange(B)
    high = mutate == "ties_high"
    a = _first_argmax(z, high)
    m = z[rows, a]
    rest = z.copy()
    rest[rows, a] = -np.inf
    second = rest.max(axis=1) if V > 1 else np.full(B, -np.inf)
    gap = m - second
    pick, margin = a.copy(), gap.copy()
    fired = np.zeros(B, dtype=bool)
    kept = np.zeros(B, dtype=bool)
    if unk >= 0:
        zx = z.copy()
        zx[:, unk] = -np.inf
        ax = _first_argmax(zx, high)
        mx = zx[rows, ax]
        zx[rows, ax] = -np.inf
        gap_x = mx - (zx.max(axis=1) if V > 2 else np.full(B, -np.inf))
        fired = a == unk
        kept = fired & ((0.0 > mx) | ((0.0 == mx) & (unk < ax)))
        if mutate == "unk_always_ax":
            pick = np.where(fired, ax, a)
        else:
            pick = np.where(fired, np.where(kept, unk, ax), a)
        margin = np.where(fired, np.minimum(gap, np.abs(mx)), gap)
        margin = np.where(fired & ~kept, np.minimum(margin, gap_x), margin)
    dead = ~(z > -np.inf).any(axis=1)              # all NaN or all -inf: nothing compared greater than the sentinel
    pick = np.where(dead, min(max(blank, 0), V - 1), pick)
    return dict(pick=pick.astype(np.int64), gap=gap, margin=margin, second=second, fired=fired, kept=kept)


def replay(net, E1, dec_out, h, c, unk=-1, forced=None, store=None, round_g=False, mutate=None):
    """E1 [B, T, J]; dec_out [B, P2], h, c [L, B, H]: the state before the call; forced [B, T] or None (free running).
    Returns Replay: logits [B, T, V], pick / gap / margin / inc [B, T] (numpy), and the state AFTER every frame:
    dec [T, B, P2], h, c [T, L, B, H] (torch float64); fired / kept [B, T]: the <unk> rule's outcomes."""
    assert mutate is None or mutate in MUTATIONS, mutate
    E1, dec, h, c = _d(E1), _d(dec_out), _d(h), _d(c)
    B, T, _ = E1.shape
    if forced is not None:
        forced = np.asarray(forced, dtype=np.int64).reshape(B, T)
    out = collections.defaultdict(list)
    for t in range(T):
        z = joint_logits(net, E1[:, t], dec, store, mutate)
        zn = z.numpy()
        p = pick_rows(zn, unk, net.blank, mutate)
        top = p["second"] if mutate == "score_second" else zn.max(axis=1)
        inc = np.log(np.exp(zn - zn.max(axis=1, keepdims=True)).sum(axis=1)) + zn.max(axis=1) - top
        tok = p["pick"] if forced is None else forced[:, t]
        dec_new, h_new, c_new = pred_step(net, tok, h, c, store, round_g, mutate)
        keep = torch.from_numpy(tok != net.blank)
        if mutate == "commit_on_blank":
            keep = torch.ones_like(keep)
        elif mutate == "no_commit":
            keep = torch.zeros_like(keep)
        dec = torch.where(keep[:, None], dec_new, dec)
        h = torch.where(keep[None, :, None], h_new, h)
        c = torch.where(keep[None, :, None], c_new, c)
        for key, v in (("logits", z), ("pick", p["pick"]), ("gap", p["gap"]), ("margin", p["margin"]), ("inc", inc),
                       ("dec", dec), ("h", h), ("c", c), ("fired", p["fired"]), ("kept", p["kept"])):
            out[key].append(v)
    st = lambda k: np.stack(out[k], axis=1)                                     # noqa: E731
    return Replay(torch.stack(out["logits"], 1), st("pick"), st("gap"), st("margin"), st("inc"), torch.stack(out["dec"]),
                  torch.stack(out["h"]), torch.stack(out["c"]), st("fired"), st("kept"))


def init_state(net, B, store=None, round_g=False, bos=M.BOS):
    """decoder(BOS) from a zero state for every row: what decode.init_search_state computes."""
    L, H = len(net.w_hh), net.w_hh[0].shape[1]
    zero = torch.zeros(L, B, H, dtype=F64)
    return pred_step(net, np.full(B, bos), zero, zero, store, round_g)


def lattice_logp(net, E1_b, tokens, store=None, round_g=False, bos=M.BOS):
    """Dense log-softmax lattice lp [T, U + 1, V] (float64 numpy) of ONE utterance (E1_b [T, J]) for the label sequence
    ``tokens``: the prediction network reads BOS + tokens from a zero state (the beam searches' empty hypothesis), the
    joint every (t, u) pair.  tests/nbest_ref.path_logp re-scores a hypothesis (tokens, frames) on it."""
    E1_b = _d(E1_b)
    L, H = len(net.w_hh), net.w_hh[0].shape[1]
    h = c = torch.zeros(L, 1, H, dtype=F64)
    decs = []
    for tok in [bos] + [int(k) for k in tokens]:
        dec, h, c = pred_step(net, np.array([tok]), h, c, store, round_g)
        decs.append(dec[0])
    decs = torch.stack(decs)
    rows = [torch.log_softmax(joint_logits(net, e[None, :].expand(decs.shape[0], -1), decs, store), dim=1) for e in E1_b]
    return torch.stack(rows).numpy()


# ---------------------------------------------------------------------------------------------------------------------
# The GPU test's cases.  bf16 loads 32 k per k-step, fp32 16: the fp32 batch edges sit at half the K.  P = the encoder
# output's width (the offset of W1d inside the joint's first matrix); ``fused``: the route the shape takes.
Case = collections.namedtuple("Case", "J V E H P2 L B T P fused seed scale blank_bias")

CASES = collections.OrderedDict([
    # one k-step in every product (all other requested k-steps clamped and skipped), waves 2-3 of dec_joint_hidden
    # leave, one slice, one live row in a 16-row tile
    ("min", Case(32, 64, 32, 32, 32, 1, 1, 16, 32, True, 11, 6.0, 2.0)),
    # last slice 36 wide, 1 1/2 column blocks, the second row tile partial
    ("ragged", Case(96, 100, 64, 96, 96, 2, 21, 13, 32, True, 12, 6.0, 5.0)),
    # second load batch in every K loop in bf16 (P2, J > 640; E, H > 256 with tails of 32 and 288; H > 512); 18 slices:
    # the strided slice merge runs twice for two shares; last slice 4 wide; one row alone in the second tile
    ("kbatch", Case(672, 1092, 288, 544, 672, 2, 17, 8, 32, True, 213, 6.0, 2.0)),
    # 10 projection blocks share 32 state values: two blocks get an empty share
    ("commit_a", Case(32, 64, 32, 32, 640, 1, 16, 8, 32, True, 14, 6.0, 2.0)),
    # 3 blocks, 11 + 11 + 10 values
    ("commit_b", Case(32, 64, 32, 32, 160, 1, 16, 8, 32, True, 15, 6.0, 3.0)),
    # composed: pick_kernel with V % 64 != 0 and B % 4 != 0, add_tanh_rows, commit_kernel
    ("odd", Case(40, 101, 24, 40, 24, 2, 5, 9, 24, False, 16, 6.0, 7.0)),
    # composed, V < 64: idle lanes carry the sentinel through the wave arg-max
    ("narrow", Case(32, 40, 24, 32, 24, 1, 5, 9, 24, False, 217, 6.0, 3.0)),
])
# not among the greedy cases: the beam test's shapes - ``min`` with three utterances, and ``ragged`` with the blank raised
# further: the best-first beam search pops until a blank-extended hypothesis beats every open one, which at ``ragged``'s
# own blank bias takes more than 3000 pops on some frames (float64 restatement of the search, W = 4); at 9 it takes 90
# at the most, at ``beam_min`` 141, both well inside the 400 the test allows - and the exact-ties shape (18 slices of
# one k-step: J = 32)
EXTRA = collections.OrderedDict([
    ("beam_min", Case(32, 64, 32, 32, 32, 1, 3, 8, 32, True, 18, 6.0, 2.0)),
    ("beam_ragged", Case(96, 100, 64, 96, 96, 2, 21, 13, 32, True, 12, 6.0, 9.0)),
    ("ties", Case(32, 1092, 32, 32, 32, 1, 3, 8, 32, True, 19, 6.0, 2.0)),
])
ALL = collections.OrderedDict(list(CASES.items()) + list(EXTRA.items()))
# <unk> of the stream-mode runs (tokenizer.UNK) and the model variant they use: see ``make_problem``
UNK = M.UNK
STREAM = dict(unk_boost=5.0, shift=6.0)
# exact ties: the output row and bias of column 5 copied onto 6 (the same lane), 21 (another wave), 69 (another slice) and
# 1089 (slice 17: it lands on the merge share of slice 1) and all five raised together by ``boost`` so that they win;
# the stream-mode run has <unk> = 5 and every bias lowered by ``shift``, which puts the retake rule's zero among the
# values the tied columns take
TIES = dict(cols=(5, 6, 21, 69, 1089), boost=5.0, unk=5, shift=6.0)


def cfg_of(cs):
    """The Transducer configuration of a Case; the encoder is never run (its output is drawn at random)."""
    return dict(vocab_embed_size=cs.E, vocab_size=cs.V, input_size=8, enc_hidden_size=32, enc_layers=1,
                enc_proj_size=cs.P, dec_hidden_size=cs.H, dec_layers=cs.L, dec_proj_size=cs.P2, joint_size=cs.J)


def make_problem(cs, stream=False, ties=False):
    """(sd, enc_out [B, T, P] fp32): ``M.make_state_dict`` sharpened as tests/sync_beam_ref.sharpened does - the output
    layer scaled by ``scale``, the blank's bias raised by ``blank_bias`` - so that most frames have a clear winner and
    both blanks and tokens are picked.  Where a product has more than 32 of K its LAST 32 COLUMNS are multiplied by 4: a
    dropped k-step cannot hide behind the other K - 32.  ``stream``: the <unk> bias is raised by STREAM['unk_boost'] and
    every output bias lowered by STREAM['shift'] - the shift changes no arg-max and no softmax, only where the retake
    rule's zero lies among the other logits, so that both of its outcomes occur.  ``ties``: see TIES."""
    sd = M.make_state_dict(cfg_of(cs), cs.seed)
    sd["joint.joint.2.weight"] *= cs.scale
    sd["joint.joint.2.bias"] *= cs.scale
    sd["joint.joint.2.bias"][M.NUL] += cs.blank_bias
    tails = ["joint.joint.0.weight", "joint.joint.2.weight", "decoder.proj.weight"]
    tails += ["decoder.lstm.weight_%s_l%d" % (k, l) for k in ("ih", "hh") for l in range(cs.L)]
    for key in tails:
        K = cs.P2 if key == "joint.joint.0.weight" else sd[key].shape[1]
        if K > 32:
            sd[key][:, -32:] *= 4
    if ties:
        cols = list(TIES["cols"])
        sd["joint.joint.2.weight"][cols] = sd["joint.joint.2.weight"][cols[0]].clone()
        sd["joint.joint.2.bias"][cols] = sd["joint.joint.2.bias"][cols[0]] + TIES["boost"]
        if stream:
            sd["joint.joint.2.bias"] -= TIES["shift"]
    elif stream:
        sd["joint.joint.2.bias"][UNK] += STREAM["unk_boost"]
        sd["joint.joint.2.bias"] -= STREAM["shift"]
    g = torch.Generator(device="cpu").manual_seed(1000 + cs.seed)
    return sd, torch.randn(cs.B, cs.T, cs.P, generator=g)


_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def problem(name, stream=False):
    """make_problem of ALL[name], built once; callers leave it unchanged."""
    return _once(("problem", name, stream), lambda: make_problem(ALL[name], stream, name == "ties"))


def host_inputs(name, cd, stream=False, emb_dtype=None):
    """(net, E1 [B, T, J], (dec_out, h, c)) of a case as the HOST restates the operands of the device call: the weights
    rounded to ``cd`` by torch's cast, E1 = the encoder output (in cd) times the encoder half of the joint's first
    matrix, stored in cd; the state = decoder(BOS).  The GPU test takes all three from the device instead."""
    def make():
        cs = ALL[name]
        sd, enc = problem(name, stream)
        store = None if cd == F32 else cd
        net = net_from_sd(sd, cs.P, None if cd == F32 else cd, emb_dtype)
        w1e = sd["joint.joint.0.weight"][:, :cs.P]
        E1 = _rt(_rt(enc.to(F64), store) @ _rt(w1e.to(F64), store).t(), store)
        return net, E1, init_state(net, cs.B, store, store is not None and not cs.fused)
    return _once(("host", name, cd, stream, emb_dtype), make)


Bounds = collections.namedtuple("Bounds", "Z S H C DEC")
# fp32: one bound for every quantity, the absolute tolerance the suite already applies to fp32 search scores
# (tests/test_beam_gpu.py, rtol / atol 1e-4).  Reasoning: fp32's unit roundoff is 2^-24 = 6e-8; the longest product here
# sums 672 terms with sum |a_k b_k| of a few units at the most (|z| <= ~20, |h|, |c|, |dec| <= ~2), so a sum in any order
# is within 672 x 6e-8 x a few = 1e-4 of the exact one, and tanhf / expf add a few ulps; the cell is contractive (|f| < 1),
# so the error of the carried state does not grow with the <= 16 frames.
F32_BOUND = 1e-4


def measure(net, E1, state, unk=-1, store=BF16, round_g=False):
    """(b) of the host test: the rounded replay running free, the exact replay forced onto its tokens; the largest
    difference of the logits, of the score increments and of the state after any frame.
    Returns (dict ERR_*, rounded replay, exact replay)."""
    rounded = replay(net, E1, *state, unk=unk, store=store, round_g=round_g)
    exact = replay(net, E1, *state, unk=unk, forced=rounded.pick)
    err = dict(Z=(rounded.logits - exact.logits).abs().max().item(), S=float(np.abs(rounded.inc - exact.inc).max()),
               H=(rounded.h - exact.h).abs().max().item(), C=(rounded.c - exact.c).abs().max().item(),
               DEC=(rounded.dec - exact.dec).abs().max().item())
    return err, rounded, exact


def host_measure(name, stream=False, emb_dtype=None):
    """``measure`` on ``host_inputs(name, bf16)``, once."""
    def make():
        net, E1, state = host_inputs(name, BF16, stream, emb_dtype)
        unk = -1 if not stream else TIES["unk"] if name == "ties" else UNK
        return measure(net, E1, state, unk, BF16, not ALL[name].fused)
    return _once(("measure", name, stream, emb_dtype), make)


def bounds(name, cd, stream=False, emb_dtype=None):
    """The GPU test's bounds of a case: bf16: 3 x the ERR_* of ``host_measure`` - the device shares the replay's rounding
    points and differs from it by fp32 summation order and the fast exp / tanh of the bf16 cell, each far below one bf16
    rounding, but either can move a value across a rounding boundary; the factor 3 pays for that.  fp32: F32_BOUND."""
    if cd == F32:
        return Bounds(*([F32_BOUND] * 5))
    err = host_measure(name, stream, emb_dtype)[0]
    return Bounds(*[3.0 * err[k] for k in Bounds._fields])


def lattice_error(name):
    """ERR_LP of a case: the largest difference between the bf16-rounded and the exact log-softmax lattice, over the
    lattices of every row's greedy token sequence (the rounded free replay's).  The GPU test's bound on a beam
    hypothesis' ``token_logp`` is 3 x this, on ``logp`` 3 x this x the number of terms of the path."""
    def make():
        cs = ALL[name]
        net, E1, state = host_inputs(name, BF16)
        run = host_measure(name)[1]
        worst = 0.0
        for b in range(cs.B):
            tokens = [int(k) for k in run.pick[b] if k != net.blank]
            a = lattice_logp(net, E1[b], tokens, store=BF16, round_g=not cs.fused)
            worst = max(worst, float(np.abs(a - lattice_logp(net, E1[b], tokens)).max()))
        return worst
    return _once(("lattice", name), make)
