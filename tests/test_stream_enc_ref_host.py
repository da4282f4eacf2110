"""CPU: the float64 replay of the fused streaming encoder step (tests/stream_enc_ref.py) pinned before the GPU test
(tests/test_stream_encoder_gpu.py) leans on it: (a) unrounded, it IS oracle.models_ref.encoder_forward; (b) rounded, every
stored buffer is bf16; (c) for every GPU case the rounded replay stays inside the bound the GPU test applies, so the
reference alone does not use that bound up; (d) every arithmetic mutation of the replay moves a result by at least five
times that bound at the cases that are there for its edge - the GPU test would fail if a kernel made that error.
The argument refusals of the native call are here too: they are raised before anything touches a device."""
import ctypes

import pytest
import torch

import stream_enc_ref as R
from oracle import models_ref as M

F64, BF16 = torch.float64, torch.bfloat16
BF16_TOL = 2e-2              # OUT_TOL[BF16] of tests/test_lstm_gpu.py: the bound of the GPU test's end-to-end check


def _random_sd(I0, H, L, P, seed):
    cfg = dict(vocab_embed_size=8, vocab_size=12, input_size=I0, enc_hidden_size=H, enc_layers=L, enc_proj_size=P,
               dec_hidden_size=8, dec_layers=1, dec_proj_size=8, joint_size=8)
    return {k: v.double() for k, v in M.make_state_dict(cfg, seed).items() if k.startswith("encoder.")}


# (B, T, I0, H, L, time reductions, carried state)
ORACLE_CASES = [
    (3, 1, 16, 8, 1, (), False),            # T = 1, L = 1, no state
    (3, 1, 16, 8, 1, (0,), True),           # T = 1 under a reduction: the lone frame is halved; L = 1 reduced = last layer
    (2, 5, 24, 16, 3, (0, 2), True),        # odd T twice (5 -> 3 -> 2), reductions on layer 0 and on the last layer
    (2, 3, 24, 16, 3, (1,), False),         # odd T under a reduction in the middle, no carried state
    (4, 4, 8, 8, 2, (), True),              # no reduction
    (1, 7, 16, 8, 4, (0, 1, 3), True),      # 7 -> 4 -> 2 -> 2 -> 1
]


@pytest.mark.parametrize("B,T,I0,H,L,red,state", ORACLE_CASES)
def test_unrounded_replay_is_the_oracle_encoder(B, T, I0, H, L, red, state):
    sd = _random_sd(I0, H, L, 5, seed=7 + T)
    g = torch.Generator(device="cpu").manual_seed(11)
    xs = torch.randn(B, T, I0, generator=g, dtype=F64)
    hid = (torch.randn(L, B, H, generator=g, dtype=F64), torch.randn(L, B, H, generator=g, dtype=F64)) if state else None
    want, (wh, wc) = M.encoder_forward(sd, xs, hid, time_reductions=red, explicit=True)
    got = R.encoder_steps64(sd, xs, hid, red)
    proj = got.out @ sd["encoder.proj.weight"].t() + sd["encoder.proj.bias"]
    assert got.T_out == want.shape[1] and got.out.dtype == F64
    for a, b in ((proj, want), (got.h, wh), (got.c, wc)):
        assert a.shape == b.shape
        assert (a - b).abs().max().item() <= 1e-12
    # and torch's own LSTM primitive agrees with the spelled-out recurrence both are written in
    prim = M.encoder_forward(sd, xs, hid, time_reductions=red)[0]
    assert (proj - prim).abs().max().item() <= 1e-10


def test_layer_steps_are_the_oracle_layer_and_take_a_kernels_own_rows():
    g = torch.Generator(device="cpu").manual_seed(5)
    r = lambda *s: torch.randn(*s, generator=g, dtype=F64)            # noqa: E731
    X, w_ih, w_hh, b_ih, b_hh, h0, c0 = r(3, 4, 16), r(32, 16), r(32, 8), r(32), r(32), r(3, 8), r(3, 8)
    want = M.lstm_layer(X, w_ih, w_hh, b_ih, b_hh, h0, c0, explicit=True)
    got = R.layer_steps64(X, w_ih, w_hh, b_ih, b_hh, h0, c0)
    for a, b in zip(got, want):
        assert (a - b).abs().max().item() <= 1e-12
    # its own rows handed back as the stored ones: the same run; other rows: step 0 alone is unchanged
    again = R.layer_steps64(X, w_ih, w_hh, b_ih, b_hh, h0, c0, Y_stored=got[0])
    assert all(torch.equal(a, b) for a, b in zip(again, got))
    other = R.layer_steps64(X, w_ih, w_hh, b_ih, b_hh, h0, c0, Y_stored=got[0] + 0.25)
    assert torch.equal(other[0][:, 0], got[0][:, 0]) and not torch.equal(other[0][:, 1], got[0][:, 1])


@pytest.mark.parametrize("name", list(R.CASES))
def test_rounded_replay_stores_bf16_and_stays_inside_the_gpu_bound(name):
    """(b) every buffer the native call stores in bf16 is bf16-representable in the rounded replay, the states are not
    rounded; (c) rounded against unrounded: max |a - b| <= 2e-2 * max(|b|, 1e-3) for the output and both states of EVERY
    GPU case, with the seeds and depths as listed (none had to be changed).  Largest ratios: c 1.03e-2 (k8_step),
    h 1.01e-2 (h96), out 7.4e-3 (h96); the lines are printed with -s."""
    cs = R.CASES[name]
    exact, rounded = R.replay(name), R.replay(name, BF16)
    assert set(rounded.stored) == {"input copy", "X"} | {"%s %d" % (k, l) for k in ("h copy", "Y", "act") for l in range(cs.L)}
    for key, buf in rounded.stored.items():
        assert torch.equal(buf, buf.to(BF16).to(F64)), key
    assert torch.equal(rounded.out, rounded.stored["act %d" % (cs.L - 1)])
    assert not torch.equal(rounded.h, rounded.h.to(BF16).to(F64))
    assert not torch.equal(rounded.c, rounded.c.to(BF16).to(F64))
    T = cs.T
    for l in range(cs.L):
        T = (T + 1) // 2 if l in cs.red else T
    assert rounded.T_out == exact.T_out == T and tuple(rounded.out.shape) == (cs.B, T, cs.H)
    worst = {}
    for key, a, b in (("out", rounded.out, exact.out), ("h", rounded.h, exact.h), ("c", rounded.c, exact.c)):
        err, scale = (a - b).abs().max().item(), max(b.abs().max().item(), 1e-3)
        worst[key] = err / scale
    print("\nstream encoder replay %s rounded vs exact: %s" % (name, ", ".join("%s %.2e" % kv for kv in worst.items())))
    for key, v in worst.items():
        assert v <= BF16_TOL, (name, key, v)


def _applies(cs, mutation):
    """Is the mutation an error at all at this case?"""
    T_layer, odd_under_reduction = cs.T, False
    for l in range(cs.L):
        if l in cs.red:
            odd_under_reduction |= T_layer % 2 == 1
            T_layer = (T_layer + 1) // 2
    return {"drop_x_tail": True, "no_b_hh": True, "swap_fg": True,
            "drop_h_tail": cs.state or cs.T > 1,            # h is zero otherwise
            "h0_zero": cs.state,
            "no_residual": cs.L > 1,
            "lone_not_halved": odd_under_reduction}[mutation]


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_every_mutation_moves_a_result_by_five_times_the_gpu_bound(mutation):
    """(d) the replay with one arithmetic error - the last 8-group of K dropped from the x product, of H from the h
    product, b_hh omitted, the f and g gates swapped, step 0 reading zero for the carried h, the residual omitted, the lone
    last frame of an odd-T reduction not halved - against the replay without it, bf16 stores in both: at EVERY GPU case
    where the mutation changes anything (a product has a tail everywhere; a carried state, a second layer or an odd T
    under a reduction only where the case has one) the output or a state moves by >= 5 x 2e-2 x max(|ref|, 1e-3), whole
    buffer, the widest of the scales the GPU test applies.  The 4x weight on the last 8 columns of every matrix and the
    H-independent bias scale (stream_enc_ref.problem) are what makes this hold at K = 520 and H = 544."""
    hit = []
    for name, cs in R.CASES.items():
        if not _applies(cs, mutation):
            continue
        sd, x, hid = R.problem(name)
        ref = R.replay(name, BF16)
        mut = R.encoder_steps64(sd, x, hid, cs.red, store=BF16, mutate=mutation)
        moved = max((a - b).abs().max().item() / max(b.abs().max().item(), 1e-3)
                    for a, b in ((mut.out, ref.out), (mut.h, ref.h), (mut.c, ref.c)))
        print("\nstream encoder replay %s with %s: moved by %.2f of the scale" % (name, mutation, moved))
        assert moved >= 5 * BF16_TOL, (name, mutation, moved)
        hit.append(name)
    # the cases that exist for the edge the mutation stands for
    need = {"drop_x_tail": {"k8_step", "k8_tile", "k40", "k240_b16", "k240_b65", "k520"},
            "drop_h_tail": {"h32", "h96", "h160", "h544"},
            "no_b_hh": {"k240_b1", "k240_b130"}, "swap_fg": {"k240_b1", "k240_b130"},
            "h0_zero": {"k8_step", "k8_tile", "h32", "h544", "deep"},
            "no_residual": {"h32", "h96", "odd_t", "deep"},
            "lone_not_halved": {"h96", "odd_t", "deep"}}[mutation]
    assert need <= set(hit), (mutation, need - set(hit))


def test_native_argument_errors_are_status_codes(hip_lib):
    """edgedict_stream_encoder_step validates before it touches the device - the pointers below are never dereferenced,
    and a refusal at a later layer has not already advanced the state of an earlier one."""
    fake = ctypes.c_void_p(256)
    arr = (ctypes.c_void_p * 2)(256, 256)
    t_out = ctypes.c_int(-7)

    def call(B=2, T=1, I0=16, H=32, L=2, red=(1, 1), x_dtype=1, xs=fake):
        r = (ctypes.c_int * L)(*red)
        return hip_lib.edgedict_stream_encoder_step(xs, x_dtype, B, T, I0, H, L, fake, fake, arr, arr, arr, arr, arr, arr, r,
                                                    fake, fake, fake, ctypes.byref(t_out), fake, None)
    assert call(H=48) == -1
    assert b"H % 32" in hip_lib.edgedict_last_error()
    assert call(I0=12) == -1
    assert b"I0 % 8" in hip_lib.edgedict_last_error()
    for red in ((3, 1), (1, 0), (1, 4)):                      # at the first layer and behind a valid one
        assert call(red=red) == -1
        assert b"time reduction must be 1 or 2" in hip_lib.edgedict_last_error()
    assert call(x_dtype=2) == -1
    assert b"dtype" in hip_lib.edgedict_last_error()
    assert call(xs=None) == -1
    assert b"null" in hip_lib.edgedict_last_error()
    assert call(B=0) == -1
    assert t_out.value == -7
    ws = hip_lib.edgedict_stream_encoder_workspace_bytes
    assert ws(0, 1, 16, 32, 1) == 0 and ws(2, 1, 16, 32, 1) > 0
