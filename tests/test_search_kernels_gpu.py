"""GPU: the search frame kernels - dec_joint_hidden, dec_logits_pick, dec_lstm_step, dec_proj_commit of
csrc/decode_fused.hip and, for shapes they do not cover, add_tanh_rows, pick_kernel, commit_kernel of csrc/decode.hip
around the general kernels - in bf16 and fp32 against the float64 replay of tests/search_ref.py, at the kernels' tile
edges (the cases and what each is there for: search_ref.CASES).

A bf16 search feeds its own picks back and one near-tie flips a token, so no free-running reference can be matched token
for token.  Every check here therefore FORCES the replay onto the device's own tokens: the prediction network's state is
a function of the token history alone, so the replay knows the logits the device should have seen on every frame, and
each pick, each score increment and the final state is judged on its own.  The replay reads the device's operands: the
joint's encoder rows (decode.joint_rows), the initial state and the converted weights (decode._SearchNet) are copied from
the device before the call.  Every case asserts the route it is there for through edgedict_decode_fused_ok.

Bounds.  bf16: BOUND_* = 3 x ERR_* of the same case, ERR_* = the bf16-rounded replay against the exact one on the CPU
(search_ref.measure; tests/test_search_ref_host.py prints them and shows that every arithmetic mutation of the replay
overshoots the bounds five times):

    case           ERR_Z    ERR_S    ERR_H    ERR_C    ERR_DEC
    min            7.0e-03  2.4e-03  8.9e-04  1.9e-03  1.1e-03
    ragged         3.8e-02  1.3e-02  5.4e-03  7.9e-03  3.2e-03
    ragged stream  3.5e-02  1.8e-02  4.4e-03  7.2e-03  2.9e-03
    kbatch         5.3e-03  2.8e-03  2.2e-03  3.8e-03  7.3e-04
    commit_a       4.9e-03  3.7e-03  1.4e-03  2.9e-03  1.5e-03
    commit_b       7.4e-03  4.0e-03  1.3e-03  3.3e-03  1.5e-03
    odd            3.2e-02  1.2e-02  2.3e-03  3.4e-03  4.0e-03
    narrow         7.6e-03  4.4e-03  1.3e-03  2.1e-03  9.9e-04
    lattice (beam) ERR_LP: beam_min 9.9e-03, beam_ragged 6.0e-02

The device shares the replay's rounding points and differs from the rounded replay by fp32 summation order and the fast
exp / tanh of the bf16 cell - each far below one bf16 rounding, but either can move a value across a rounding boundary:
the factor 3 pays for that.  fp32: search_ref.F32_BOUND = 1e-4 for every quantity against the unrounded replay, the score
as in tests/test_beam_gpu.py (rtol / atol 1e-4).  A frame is DECIDED where the replay's decision margin is at least
2 x BOUND_Z; there the device's pick must be the replay's.

No dimension of ``odd`` or ``narrow`` had to move: the general kernels take them as they are.

Measured on an MI355X (44 tests, 2.2 s).  In bf16 the device lands on the rounded replay's own values almost everywhere -
the rounding points are the kernels' - and leaves it only where a value fell on the other side of a bf16 rounding:

    run (bf16)      decided / frames  dec_out err / bound   h err / bound        c err / bound        score err / T BOUND_S  worst increment / BOUND_S
    min                  15 / 16      0       / 3.2e-03     5.5e-08 / 2.7e-03    1.1e-07 / 5.8e-03    8.6e-07 / 1.1e-01      4.0e-07 / 7.1e-03
    ragged              236 / 273     9.8e-04 / 9.5e-03     3.5e-05 / 1.6e-02    5.8e-05 / 2.4e-02    4.6e-03 / 4.9e-01      4.6e-03 / 3.7e-02
    ragged stream       229 / 273     9.8e-04 / 8.6e-03     3.5e-05 / 1.3e-02    5.8e-05 / 2.2e-02    4.6e-03 / 6.9e-01      4.6e-03 / 5.3e-02
    kbatch              115 / 136     4.9e-04 / 2.2e-03     2.2e-05 / 6.7e-03    4.5e-05 / 1.1e-02    1.1e-03 / 6.6e-02      1.1e-03 / 8.3e-03
    commit_a            118 / 128     0       / 4.6e-03     7.0e-08 / 4.2e-03    1.0e-07 / 8.7e-03    2.3e-06 / 8.9e-02      3.5e-07 / 1.1e-02
    commit_b            118 / 128     0       / 4.5e-03     8.6e-08 / 3.8e-03    1.3e-07 / 9.9e-03    2.1e-06 / 9.7e-02      4.4e-07 / 1.2e-02
    odd                  44 / 45      0       / 1.2e-02     1.2e-07 / 6.7e-03    2.6e-07 / 1.0e-02    1.2e-06 / 3.3e-01      6.4e-07 / 3.6e-02
    narrow               44 / 45      0       / 3.0e-03     5.9e-08 / 3.9e-03    9.6e-08 / 6.3e-03    1.5e-06 / 1.2e-01      2.9e-07 / 1.3e-02
    min, bf16 table      15 / 16      0       / 2.7e-03     5.5e-08 / 3.4e-04    1.1e-07 / 7.2e-04    8.6e-07 / 1.2e-01
    ragged, bf16 table  240 / 273     9.8e-04 / 8.3e-03     3.5e-05 / 6.0e-03    5.8e-05 / 6.5e-03    4.6e-03 / 5.6e-01

Every decided frame carried the replay's pick and no pick was below the float64 maximum at all.  fp32 (bound 1e-4, every
frame decided): dec_out <= 2.4e-07, h <= 4.9e-07, c <= 8.7e-07, score <= 6.7e-06, a frame's increment <= 2.7e-06.  The
tied columns won 17 (bf16) / 18 (fp32) of 24 frames.  Beam: beam_min 12 hypotheses, beam_ragged 84; token_logp within
7.8e-07 (bf16, bound 3.0e-02 / 1.8e-01) and 1.6e-06 (fp32), logp within 3.4e-07 per term.
"""
import collections
import ctypes

import numpy as np
import pytest
import torch

import nbest_ref
import search_ref as R

pytestmark = pytest.mark.gpu

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
DTYPES = [BF16, F32]
_ID = {BF16: "bf16", F32: "fp32"}.get


def _runs():
    """(case, stream mode) of the greedy runs."""
    for name in R.CASES:
        yield name, False
    yield "ragged", True


_MODELS = {}


def _model(name, cd, stream=False):
    """The Transducer of a problem on the device in the compute dtype ``cd``, built once.  Its encoder is never run."""
    key = (name, cd, stream)
    if key not in _MODELS:
        from edgedict_amd.models import Transducer
        sd, _ = R.problem(name, stream)
        m = Transducer(enc_dropout=0.0, dec_dropout=0.0, output_loss=False, **R.cfg_of(R.ALL[name]))
        m.load_state_dict(sd, strict=True)
        m = m.cuda().eval()
        m.compute_dtype = _ID(cd)
        _MODELS[key] = m
    return _MODELS[key]


Inputs = collections.namedtuple("Inputs", "model enc E1 state net")


def _clone(state):
    from edgedict_amd.decode import SearchState
    return SearchState(state.dec_out.clone(), state.h.clone(), state.c.clone())


_INPUTS = {}


def _inputs(name, cd, stream=False):
    """What one search call reads, on the device, and the replay's float64 copy of the weights: once per run."""
    key = (name, cd, stream)
    if key not in _INPUTS:
        from edgedict_amd import decode
        cs = R.ALL[name]
        model = _model(name, cd, stream)
        enc = R.problem(name, stream)[1].cuda().to(cd)
        with torch.no_grad():
            E1 = decode.joint_rows(model, enc)
            state = decode.init_search_state(model, cs.B)
        assert E1.dtype == cd and tuple(E1.shape) == (cs.B * cs.T, cs.J) and E1.is_contiguous()
        assert state.dec_out.dtype == cd and state.h.dtype == state.c.dtype == F32
        torch.cuda.synchronize()
        _INPUTS[key] = Inputs(model, enc, E1, state, _net(model, cd, cs.P))
    return _INPUTS[key]


def _net(model, cd, P, emb=None):
    """The replay's Net from the tensors decode._SearchNet hands to the kernels."""
    from edgedict_amd import decode
    sn = decode._SearchNet(model, cd)
    assert all(w.dtype == cd for w in [sn.w1c, sn.w2c, sn.wpc] + sn.w_ih + sn.w_hh) and sn.emb.dtype == F32
    return R.make_net(sn.w1c[:, P:], sn.b1, sn.w2c, sn.b2, sn.emb if emb is None else emb, sn.w_ih, sn.w_hh, sn.b_ih,
                      sn.b_hh, sn.wpc, sn.bp, model.blank)


def _assert_route(name, cd, emb_dtype=F32):
    """The shape takes the route the case is there for."""
    from edgedict_amd import _lib
    cs = R.ALL[name]
    got = _lib.load().edgedict_decode_fused_ok(_lib.dtype_code(cd), _lib.dtype_code(emb_dtype), cs.J, cs.V, cs.E, cs.H, cs.P2)
    assert got == int(cs.fused), "%s: fused route %d, the case is there for %d" % (name, got, cs.fused)


def _greedy(model, E1, row_stride, frame_stride, B, T, P, state, unk=-1, emb=None):
    """edgedict_greedy_decode called as decode.run_search calls it, but on joint rows at any address and strides (elements)
    and, with ``emb``, another embedding table.  ``state`` is advanced in place.  Returns (tokens [B, T] int32, score [B])."""
    from edgedict_amd import _lib, decode
    cd = E1.dtype
    net = decode._SearchNet(model, cd)
    if emb is not None:
        net.emb = emb
    lib = _lib.load()
    nbytes = lib.edgedict_greedy_workspace_bytes(_lib.dtype_code(cd), B, net.J, net.V, net.E, net.L, net.H, net.P2)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    tokens = torch.full((B, T), -1, dtype=torch.int32, device="cuda")
    score = torch.zeros(B, dtype=F32, device="cuda")
    rc = lib.edgedict_greedy_decode(
        _lib.dtype_code(cd), _lib.ptr(E1), ctypes.c_longlong(row_stride), ctypes.c_longlong(frame_stride), B, T,
        *net.args(P), _lib.ptr(state.h), _lib.ptr(state.c), _lib.ptr(state.dec_out), int(model.blank), int(unk),
        _lib.ptr(tokens), tokens.stride(0), _lib.ptr(score), _lib.ptr(ws), _lib.stream_ptr())
    _lib.check(rc, "greedy_decode")
    torch.cuda.synchronize()
    del net, ws
    return tokens, score


Result = collections.namedtuple("Result", "tokens score dec h c")


def _host(tokens, score, state):
    return Result(tokens.cpu().numpy().astype(np.int64), score.double().cpu().numpy(), state.dec_out.double().cpu(),
                  state.h.double().cpu(), state.c.double().cpu())


def _unk(name, stream):
    return -1 if not stream else R.TIES["unk"] if name == "ties" else R.UNK


_RESULTS = {}


def _result(name, cd, stream=False):
    """ONE decode.run_search call over all frames of the case, made once: (Result, the replay forced onto its tokens)."""
    key = (name, cd, stream)
    if key not in _RESULTS:
        from edgedict_amd import decode
        inp = _inputs(name, cd, stream)
        _assert_route(name, cd)
        state = _clone(inp.state)
        with torch.no_grad():
            tokens, score = decode.run_search(inp.model, inp.enc, state, unk=_unk(name, stream), want_score=True)
        torch.cuda.synchronize()
        got = _host(tokens, score, state)
        _RESULTS[key] = (got, _forced(name, cd, inp, got.tokens, _unk(name, stream)))
    return _RESULTS[key]


def _forced(name, cd, inp, tokens, unk, net=None):
    """The replay on the device's operands, forced onto the device's tokens: bf16-rounded for a bf16 search."""
    cs = R.ALL[name]
    store = None if cd == F32 else BF16
    return R.replay(net or inp.net, inp.E1.view(cs.B, cs.T, cs.J), inp.state.dec_out, inp.state.h, inp.state.c, unk=unk,
                    forced=tokens, store=store, round_g=store is not None and not cs.fused)


def _judge(tag, name, cd, stream, got, rep, bound):
    """Checks 1-4 of a whole search call against the forced replay; prints the worst errors beside the bounds."""
    cs = R.ALL[name]
    B, T, V = cs.B, cs.T, cs.V
    # 1. every token is a symbol
    assert got.tokens.shape == (B, T) and ((got.tokens >= 0) & (got.tokens < V)).all()
    # 2. the picks: on decided frames the replay's own; in the greedy mode never further than 2 BOUND_Z below the maximum
    z = rep.logits.numpy()
    decided = rep.margin >= 2 * bound.Z
    short = z.max(axis=-1) - np.take_along_axis(z, got.tokens[..., None], axis=-1)[..., 0]
    undecided = 1.0 - decided.mean()
    wrong = int((got.tokens != rep.pick)[decided].sum())
    assert wrong == 0, "%s: %d of %d decided frames picked another symbol than the replay" % (tag, wrong, decided.sum())
    if not stream:
        assert short.max() <= 2 * bound.Z, (tag, short.max(), 2 * bound.Z)
        assert (short[decided] == 0).all()
    assert undecided <= 0.25, (tag, undecided)
    # 3. the final state, whole and on the last (partial) 16-row tile alone
    r0 = B - (B % 16 or 16)
    worst = {}
    for key, a, b, lim, rows in (("dec", got.dec, rep.dec[-1], bound.DEC, lambda t: t[r0:]),
                                 ("h", got.h, rep.h[-1], bound.H, lambda t: t[:, r0:]),
                                 ("c", got.c, rep.c[-1], bound.C, lambda t: t[:, r0:])):
        assert a.shape == b.shape and torch.isfinite(a).all(), (tag, key)
        worst[key] = ((a - b).abs().max().item(), rows(a - b).abs().max().item(), lim)
    # 4. the score: the sum of the increments
    want = rep.inc.sum(axis=1)
    s_err = float(np.abs(got.score - want).max())
    print("\nsearch %s: %d frames, %d decided, all equal; max z - z[pick] %.2e (2 BOUND_Z %.2e); final state err whole / last "
          "tile / bound: %s; score err %.2e (T BOUND_S %.2e)"
          % (tag, B * T, decided.sum(), short.max(), 2 * bound.Z,
             ", ".join("%s %.2e / %.2e / %.2e" % ((k,) + v) for k, v in worst.items()), s_err, T * bound.S))
    for key, (whole, tail, lim) in worst.items():
        assert whole <= lim and tail <= lim, (tag, key, whole, tail, lim)
    if cd == F32:
        np.testing.assert_allclose(got.score, want, rtol=1e-4, atol=1e-4)
    else:
        assert s_err <= T * bound.S, (tag, s_err, T * bound.S)


@pytest.mark.parametrize("cd", DTYPES, ids=_ID)
@pytest.mark.parametrize("name,stream", list(_runs()))
def test_search_call_against_the_forced_replay(hip_lib, name, stream, cd):
    """One call over all frames: tokens inside the vocabulary; on every decided frame the pick of the replay (greedy mode:
    the float64 arg-max; stream mode: the retake rule's outcome), on every frame within 2 BOUND_Z of the maximum; at most
    25 % undecided frames; the final dec_out, h and c within their bounds, whole and on the last row tile; the score
    within T x BOUND_S of the sum of the float64 increments."""
    got, rep = _result(name, cd, stream)
    _judge("%s%s %s" % (name, " stream" if stream else "", _ID(cd)), name, cd, stream, got, rep, R.bounds(name, cd, stream))


@pytest.mark.parametrize("cd", DTYPES, ids=_ID)
@pytest.mark.parametrize("name,stream", list(_runs()))
def test_frame_by_frame_equals_the_single_call_and_commits_only_non_blank_rows(hip_lib, name, stream, cd):
    """T calls of one frame each on the same joint rows, carrying the state, a fresh zero score per call: tokens and final
    state bit-equal to the single call; each frame's score increment within BOUND_S of the replay's (fp32: rtol / atol
    1e-4); rows whose pick is blank have dec_out, h and c bit-equal to before the call, the other rows have not."""
    cs = R.CASES[name]
    inp = _inputs(name, cd, stream)
    got, rep = _result(name, cd, stream)
    bound = R.bounds(name, cd, stream)
    state = _clone(inp.state)
    esz = inp.E1.element_size()
    worst = 0.0
    for t in range(cs.T):
        before = _clone(state)
        frame = inp.E1.view(cs.B, cs.T, cs.J)[:, t]                     # row b of frame t at b * T * J (+ t * J)
        assert frame.data_ptr() == inp.E1.data_ptr() + t * cs.J * esz
        tok, score = _greedy(inp.model, frame, cs.T * cs.J, cs.J, cs.B, 1, cs.P, state, _unk(name, stream))
        tok = tok.cpu().numpy()[:, 0]
        assert np.array_equal(tok, got.tokens[:, t]), (name, t)
        inc = score.double().cpu().numpy()
        worst = max(worst, float(np.abs(inc - rep.inc[:, t]).max()))
        if cd == F32:
            np.testing.assert_allclose(inc, rep.inc[:, t], rtol=1e-4, atol=1e-4)
        else:
            assert np.abs(inc - rep.inc[:, t]).max() <= bound.S, (name, t, np.abs(inc - rep.inc[:, t]).max(), bound.S)
        blank = torch.from_numpy(tok == inp.model.blank).cuda()
        for key, a, b in (("dec_out", state.dec_out, before.dec_out), ("h", state.h.transpose(0, 1), before.h.transpose(0, 1)),
                          ("c", state.c.transpose(0, 1), before.c.transpose(0, 1))):
            same = (a == b).reshape(cs.B, -1).all(dim=1)
            assert bool(same[blank].all()), "%s frame %d: %s of a row that picked blank changed" % (name, t, key)
            assert not bool(same[~blank].any()), "%s frame %d: %s of a row that picked a symbol did not change" % (name, t, key)
    end = _host(torch.from_numpy(got.tokens), torch.zeros(cs.B), state)
    assert torch.equal(end.dec, got.dec) and torch.equal(end.h, got.h) and torch.equal(end.c, got.c)
    print("\nsearch %s%s %s frame by frame: worst score increment err %.2e (BOUND_S %.2e)"
          % (name, " stream" if stream else "", _ID(cd), worst, bound.S))


@pytest.mark.parametrize("cd", DTYPES, ids=_ID)
@pytest.mark.parametrize("stream", [False, True], ids=["greedy", "unk5"])
def test_exact_ties_go_to_the_lowest_index(hip_lib, stream, cd):
    """V = 1092, J = 32: the output row and bias of column 5 on 6 (the same lane), 21 (another wave), 69 (another slice)
    and 1089 (slice 17, the merge share of slice 1), raised together so that they win: identical columns give
    bit-identical logits on the device, so wherever they beat every other column by more than 2 BOUND_Z the pick is 5;
    with <unk> = 5 it is 6 where their value is above 2 BOUND_Z (the retake finds the equal next column) and stays 5 where
    it is below -2 BOUND_Z."""
    got, rep = _result("ties", cd, stream)
    bound = R.bounds("ties", cd, stream)
    cs = R.ALL["ties"]
    assert ((got.tokens >= 0) & (got.tokens < cs.V)).all()
    z = rep.logits.numpy()
    cols = list(R.TIES["cols"])
    value = z[:, :, cols[0]]
    rest = z.copy()
    rest[:, :, cols] = -np.inf
    win = value - rest.max(axis=-1) > 2 * bound.Z
    print("\nsearch ties %s %s: the tied columns win %d of %d frames" % ("unk5" if stream else "greedy", _ID(cd), win.sum(), win.size))
    assert int(win.sum()) >= 8
    if not stream:
        assert (got.tokens[win] == 5).all(), got.tokens[win]
    else:
        up, down = win & (value > 2 * bound.Z), win & (value < -2 * bound.Z)
        assert int(up.sum()) >= 3 and int(down.sum()) >= 3
        assert (got.tokens[up] == 6).all() and (got.tokens[down] == 5).all(), (got.tokens[up], got.tokens[down])
    # where another column wins decidedly, it is picked
    lose = (rest.max(axis=-1) - value > 2 * bound.Z) & (rep.margin >= 2 * bound.Z)
    assert np.array_equal(got.tokens[lose], rep.pick[lose])


@pytest.mark.parametrize("cd", DTYPES, ids=_ID)
def test_strided_joint_rows_inside_a_nan_buffer(hip_lib, cd):
    """``ragged`` with the joint's rows inside a larger NaN-filled buffer - row stride > T J, frame stride > J: tokens,
    score and state bit-equal to the call on the contiguous rows."""
    name = "ragged"
    cs = R.CASES[name]
    inp = _inputs(name, cd)
    _assert_route(name, cd)
    a_state, b_state = _clone(inp.state), _clone(inp.state)
    a = _greedy(inp.model, inp.E1, cs.T * cs.J, cs.J, cs.B, cs.T, cs.P, a_state)
    buf = torch.full((cs.B, cs.T + 2, cs.J + 16), float("nan"), dtype=cd, device="cuda")
    view = buf[:, 1:cs.T + 1, 8:8 + cs.J]
    view.copy_(inp.E1.view(cs.B, cs.T, cs.J))
    assert buf.stride(0) > cs.T * cs.J and buf.stride(1) > cs.J and view.data_ptr() % 16 == 0
    b = _greedy(inp.model, view, buf.stride(0), buf.stride(1), cs.B, cs.T, cs.P, b_state)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(a_state.dec_out, b_state.dec_out) and torch.equal(a_state.h, b_state.h) and torch.equal(a_state.c, b_state.c)
    # and the helper's contiguous call is run_search's
    got, _ = _result(name, cd)
    assert np.array_equal(a[0].cpu().numpy(), got.tokens) and torch.equal(a_state.h.double().cpu(), got.h)
    assert torch.isfinite(a[1]).all() and torch.isfinite(a_state.h).all()


@pytest.mark.parametrize("name", ["min", "ragged"])
def test_bf16_embedding_table(hip_lib, name):
    """The bf16 search with a bf16 embedding table - the branch of dec_lstm_step that reads the table without converting,
    which the Python layer never takes (it hands over the fp32 master table): judged like a whole call against the replay
    with the table rounded."""
    cs = R.CASES[name]
    inp = _inputs(name, BF16)
    _assert_route(name, BF16, BF16)
    emb = inp.model.decoder.embed.weight.detach().to(BF16).contiguous()
    state = _clone(inp.state)
    tokens, score = _greedy(inp.model, inp.E1, cs.T * cs.J, cs.J, cs.B, cs.T, cs.P, state, emb=emb)
    got = _host(tokens, score, state)
    net = _net(inp.model, BF16, cs.P, emb)
    _judge("%s bf16 table" % name, name, BF16, False, got, _forced(name, BF16, inp, got.tokens, -1, net),
           R.bounds(name, BF16, emb_dtype=BF16))


@pytest.mark.parametrize("cd", DTYPES, ids=_ID)
@pytest.mark.parametrize("name", ["beam_min", "beam_ragged"])
def test_beam_hypotheses_are_scored_on_the_replays_lattice(hip_lib, name, cd):
    """decode.beam_search_nbest_rows, W = 4: for EVERY returned hypothesis each ``token_logp[u]`` against the replay's
    log-softmax at (frames[u], prefix of u tokens) and ``logp`` against the path sum (nbest_ref.path_logp) on the lattice
    the replay computes from the device's operands.  bf16: 3 x ERR_LP per term (search_ref.lattice_error), times the
    number of terms for ``logp``; fp32: rtol / atol 2e-4 as in tests/test_beam_gpu.py.  Which hypotheses are popped and
    kept is not judged here: in bf16 that depends on near-ties, and the fp32 searches pin it against the oracle already.
    This covers the logits-out form of dec_logits_pick, first = 2 of dec_lstm_step, the pred == nullptr form of
    dec_proj_commit and beam_expand's log-softmax."""
    from edgedict_amd import decode
    cs = R.ALL[name]
    inp = _inputs(name, cd)
    _assert_route(name, cd)
    with torch.no_grad():
        res = decode.beam_search_nbest_rows(inp.model, inp.E1, cs.B, cs.T, cs.P, None, 4, 400)
    torch.cuda.synchronize()
    store = None if cd == F32 else BF16
    lim = 3 * R.lattice_error(name) if store is not None else None
    E1 = inp.E1.view(cs.B, cs.T, cs.J).double().cpu()
    worst_tok = worst_path = 0.0
    n = 0
    assert len(res) == cs.B
    for b, r in enumerate(res):
        assert 1 <= len(r) <= 4
        for tokens, frames, tlp, logp in zip(r.tokens, r.frames, r.token_logp, r.logp):
            assert ((tokens > 0) & (tokens < cs.V)).all() and ((frames >= 0) & (frames < cs.T)).all()
            assert (np.diff(frames) >= 0).all() and np.isfinite(tlp).all() and np.isfinite(logp)
            lp = R.lattice_logp(inp.net, E1[b], tokens, store=store)
            total, terms = nbest_ref.path_logp(lp, tokens, frames)
            terms_n = cs.T + len(tokens)
            if len(tokens):
                worst_tok = max(worst_tok, float(np.abs(tlp - terms).max()))
            worst_path = max(worst_path, abs(float(logp) - total) / terms_n)
            if store is None:
                np.testing.assert_allclose(tlp, terms, rtol=2e-4, atol=2e-4)
                np.testing.assert_allclose(float(logp), total, rtol=2e-4, atol=2e-4)
            else:
                assert len(tokens) == 0 or np.abs(tlp - terms).max() <= lim, (b, np.abs(tlp - terms).max(), lim)
                assert abs(float(logp) - total) <= lim * terms_n, (b, float(logp), total, lim * terms_n)
            n += 1
    print("\nsearch beam %s %s: %d hypotheses, worst token_logp err %.2e, worst logp err per term %.2e (bound per term %s)"
          % (name, _ID(cd), n, worst_tok, worst_path, "%.2e" % lim if lim else "rtol / atol 2e-4"))
