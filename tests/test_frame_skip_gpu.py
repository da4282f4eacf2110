"""GPU: blank-frame skipping ahead of the RNN-T beam searches (csrc/frame_skip.hip; loss.ctc_blank_skip,
decode.gather_frames / skip_blank_frames, ``skip_blank=`` of the beam searches) against the fp64 oracle
tests/frame_skip_ref.py (pinned by tests/test_frame_skip_host.py), against torch indexing, and end to end against the
``_enc`` searches run on a torch-gathered encoder output.

Decisions are compared EXACTLY, which holds only where no frame's blank posterior is a near-tie with the threshold: every
set of logits goes through ``frame_skip_ref.separate`` and is asserted to have no frame within 1e-3 of it (ten times the
1e-4 the fp32 row passes are held to) - a condition on the inputs.

The kernel test's blank column is offset per frame by -4 or +6 over N(0, 0.5) logits, so a frame's blank log-odds are
about ``-4 - log(V - 1)`` or ``6 - log(V - 1)``; its threshold is the posterior at the midpoint, ``sigmoid(1 - log(V - 1)
- 1 / 8)`` (0.7 at V = 2, 2.3e-3 at V = 1032), so both outcomes occur whatever V is."""
import functools
import math

import numpy as np
import pytest
import torch

import frame_skip_ref as FR
import sync_beam_ref as S
from oracle import models_ref as M
from test_lm_fusion_gpu import _lm, _lm_sd
from test_sync_beam_gpu import CFG, _same_bits

pytestmark = pytest.mark.gpu
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
LP_TOL = dict(rtol=1e-5, atol=1e-4)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ------------------------------------------------------------------------------------------- 1. the decision
def _threshold(V):
    return 1.0 / (1.0 + math.exp(-(1.0 - math.log(V - 1) - 0.125)))


@functools.lru_cache(maxsize=None)
def _case(dtype, T, V, kind="mixed"):
    """(logits in ``dtype`` on the CPU, act_lens, threshold, oracle): computed once, read only."""
    g = torch.Generator().manual_seed(1000 * T + V)
    B = 3
    z = 0.5 * torch.randn(B, T, V, generator=g)
    up = torch.rand(B, T, generator=g) < 0.5
    if kind == "mixed":
        act = [T, T // 2, 0]                   # T, a value below T, 0
    else:
        act = [T, T, T - 1]
        up[1], up[2] = True, False             # an all-blank and a never-blank utterance beside a mixed one
    z[:, :, 0] += torch.where(up, 6.0, -4.0)
    thr = _threshold(V)
    z = FR.separate(z.to(DTYPES[dtype]), act, thr)
    return z, act, thr, FR.skip(z, act, thr)


def _run_skip(z, act, thr):
    from edgedict_amd.loss import ctc_blank_skip
    out = ctc_blank_skip(z.cuda(), torch.tensor(act, dtype=torch.int32).cuda(), thr)
    return [o.cpu() for o in out]


def _compare_skip(z, act, thr, want):
    assert not FR.in_margin(z, act, thr).any()
    wmap, wkept, wlp = want
    fmap, kept, lp = _run_skip(z, act, thr)
    assert fmap.dtype == torch.int32 and kept.dtype == torch.int32 and lp.dtype == torch.float32
    assert np.array_equal(kept.numpy(), wkept), (kept, wkept)
    assert np.array_equal(fmap.numpy(), wmap)
    err = float(np.abs(lp.double().numpy() - wlp).max())
    print("lp_blank: max abs error %.3g, kept %s of %s" % (err, wkept.tolist(), act))
    np.testing.assert_allclose(lp.double().numpy(), wlp, **LP_TOL)
    for b, n in enumerate(act):
        assert (lp[b, n:] == 0).all() and (lp[b] <= 0).all()
    again = _run_skip(z, act, thr)
    for a, b in zip((fmap, kept, lp), again):
        assert torch.equal(a, b)
    assert torch.equal(_bits(lp), _bits(again[2]))


@pytest.mark.parametrize("V", [2, 5, 72, 1030, 1032])
@pytest.mark.parametrize("T", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_blank_skip_matches_the_oracle(hip_lib, dtype, T, V):
    z, act, thr, want = _case(dtype, T, V)
    _compare_skip(z, act, thr, want)
    wmap, wkept, _ = want
    if T >= 63:     # both outcomes inside the first 64-frame pass of the full-length utterance
        first = int((wmap[0, :wkept[0]] < 64).sum())
        assert 0 < first < min(T, 64), (first, T)
    assert wkept[2] == 0 and (wmap[2] == -1).all()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_all_blank_and_never_blank_utterances(hip_lib, dtype):
    T = 130
    z, act, thr, want = _case(dtype, T, 72, "uniform")
    _compare_skip(z, act, thr, want)
    _, wkept, _ = want
    assert 0 < wkept[0] < T and wkept[1] == 0 and wkept[2] == T - 1


def test_threshold_one_keeps_every_frame(hip_lib):
    z, act, _, _ = _case("f32", 65, 72)
    fmap, kept, lp = _run_skip(z, act, 1.0)
    assert kept.tolist() == act
    for b, n in enumerate(act):
        assert fmap[b, :n].tolist() == list(range(n)) and (fmap[b, n:] == -1).all()


# ------------------------------------------------------------------------------------------- 2. the gather
@pytest.mark.parametrize("where", ["aligned", "enc_offset", "out_offset"])
@pytest.mark.parametrize("P", [8, 20, 320])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_gather_equals_torch_indexing_bit_for_bit(hip_lib, dtype, P, where):
    """P x element size: 32 / 80 / 1280 bytes (f32, 16-byte copies; 1280 takes two passes of the wave) and 16 / 40 / 640
    (bf16: 40 is no multiple of 16 - element copies).  ``enc_offset`` / ``out_offset``: a base pointer one element past
    a 16-byte boundary, made by slicing - element copies whatever P is."""
    from edgedict_amd.decode import gather_frames
    dt = DTYPES[dtype]
    B, T = 3, 70
    g = torch.Generator().manual_seed(P)
    keep = torch.rand(B, T, generator=g) < 0.5
    keep[1] = False
    keep[2, 40:] = False
    kept = keep.sum(1).to(torch.int32)
    fmap = torch.full((B, T), -1, dtype=torch.int32)
    for b in range(B):
        fmap[b, :kept[b]] = torch.nonzero(keep[b])[:, 0].to(torch.int32)
    Tc = int(kept.max())
    assert kept[1] == 0 and 0 < kept[2] < Tc and Tc > 4
    flat = torch.randn(B * T * P + 8, generator=g).to(dt).cuda()
    off = 1 if where == "enc_offset" else 0
    enc = flat[off:off + B * T * P].view(B, T, P)
    assert enc.is_contiguous() and enc.data_ptr() % 16 == (off * flat.element_size())
    obuf = torch.full((B * Tc * P + 8,), float("nan"), dtype=dt, device="cuda")
    ooff = 1 if where == "out_offset" else 0
    out = obuf[ooff:ooff + B * Tc * P].view(B, Tc, P)
    got = gather_frames(enc, fmap.cuda(), kept.cuda(), Tc, out=out)
    assert got.data_ptr() == out.data_ptr()
    want = torch.zeros(B, Tc, P, dtype=dt, device="cuda")
    for b in range(B):
        n = int(kept[b])
        want[b, :n] = enc[b, fmap[b, :n].long().cuda()]
    assert torch.equal(_bits(got), _bits(want))
    for b in range(B):
        assert (_bits(got[b, int(kept[b]):]) == 0).all()            # pad rows: zero bits
    assert torch.isnan(obuf[:ooff]).all() and torch.isnan(obuf[ooff + B * Tc * P:]).all()     # nothing outside
    if where == "aligned":
        fresh = gather_frames(enc, fmap.cuda(), kept.cuda(), Tc)
        assert torch.equal(_bits(fresh), _bits(want))
        one = gather_frames(enc, fmap.cuda(), kept.cuda(), 1)
        assert torch.equal(_bits(one), _bits(want[:, :1]))


# ------------------------------------------------------------------------------------------- 3. end to end
THR = 0.5
XLEN = [140, 100, 131]                  # encoder frames 70, 50, 66: the scan of utterance 0 crosses a 64-frame pass


class _Setup:
    """The smallest model of tests/test_sync_beam_gpu.py (CFG) with a CTC head whose blank bias puts the median frame's
    blank posterior on THR, 3 utterances of about 70 encoder frames, and the model's own head logits on them."""

    def __init__(self, dtype):
        from edgedict_amd.models import Transducer
        sd = S.sharpened(M.make_state_dict(CFG, 4), blank_bias=2.0)
        xs, _, _, _ = M.make_batch(CFG, 4, 3, 140, 4, ragged=False)
        self.xlen = torch.tensor(XLEN, dtype=torch.int32)
        for b, n in enumerate(XLEN):
            xs[b, n:] = 0
        torch.manual_seed(7)
        m = Transducer(enc_dropout=0.0, dec_dropout=0.0, output_loss=False, ctc_weight=0.3, **CFG)
        m.load_state_dict(sd, strict=False)
        with torch.no_grad():
            m.ctc_head.weight *= 4.0
            m.ctc_head.bias.zero_()
        m = m.cuda().eval()
        m.compute_dtype = dtype
        self.m, self.xs = m, xs.cuda()
        with torch.no_grad():
            enc, _ = m.encoder(self.xs)
            self.enc = enc.contiguous()
            self.lens = m.scale_length(self.enc, self.xlen).numpy().astype(np.int32)
            assert self.lens.tolist() == [70, 50, 66]
            # blank log-odds per frame from the head's weights, on the host: the median frame goes onto THR
            z = self.enc.double().cpu().numpy() @ m.ctc_head.weight.double().cpu().numpy().T
            live = np.arange(z.shape[1])[None, :] < self.lens[:, None]
            zm = z[:, :, 1:].max(axis=2)
            odds = z[:, :, 0] - (zm + np.log(np.exp(z[:, :, 1:] - zm[:, :, None]).sum(axis=2)))
            m.ctc_head.bias[0] = float(math.log(THR / (1.0 - THR)) - np.median(odds[live]))
            self.head = m._ctc_logits
            self.raw = self.head(self.enc).contiguous()

    def feed(self, logits_cpu):
        """From here on the model's head returns ``logits_cpu`` (the separated form of its own output) - after checking
        that what it was asked for is the batch's encoder output, bit for bit."""
        dev = logits_cpu.to(self.raw.dtype).cuda()

        def fed(h_enc):
            assert torch.equal(self.head(h_enc).contiguous(), self.raw)
            return dev

        self.m._ctc_logits = fed

    def gathered(self, fmap, kept):
        Tc = int(kept.max())
        out = torch.zeros(self.enc.shape[0], Tc, self.enc.shape[2], dtype=self.enc.dtype, device="cuda")
        for b in range(out.shape[0]):
            out[b, :kept[b]] = self.enc[b, torch.from_numpy(fmap[b, :kept[b]].astype(np.int64)).cuda()]
        return out


@functools.lru_cache(maxsize=None)
def _setup(dtype):
    return _Setup(dtype)


def _mapped(results, fmap):
    for b, r in enumerate(results):
        r.frames = [fmap[b, f.astype(np.int64)].astype(np.int32) for f in r.frames]
    return results


def _separated(s, thr, edit=None):
    z = s.raw.cpu().clone()
    if edit is not None:
        edit(z)
    z = FR.separate(z, s.lens, thr)
    assert not FR.in_margin(z, s.lens, thr).any()
    s.feed(z)
    return FR.skip(z, s.lens, thr)


EM = 256        # the sharpened model's best-first search needs more than the default 8 W pops on some frame


def _searches(m, which):
    """(public N-best entry point, its ``_enc`` form, the public best-of entry point); the best-first ones with
    ``max_expansions=EM``, which passes through the skipping path as every other search argument."""
    from edgedict_amd import decode
    if which == "sync":
        return m.sync_beam_search_nbest, decode.sync_beam_search_nbest_enc, m.sync_beam_search
    p = functools.partial
    return (p(m.beam_search_nbest, max_expansions=EM), p(decode.beam_search_nbest_enc, max_expansions=EM),
            p(m.beam_search, max_expansions=EM))


@pytest.mark.parametrize("W", [1, 4])
@pytest.mark.parametrize("which", ["sync", "best_first"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_search_with_skipping_is_the_enc_search_on_the_gathered_frames(hip_lib, dtype, which, W):
    s = _setup(dtype)
    fmap, kept, _ = _separated(s, THR)
    share = kept.sum() / s.lens.sum()
    print("kept", kept.tolist(), "of", s.lens.tolist())
    assert 0.25 < share < 0.75 and (kept > 0).all()
    assert (fmap[0, :kept[0]] < 64).any() and (fmap[0, :kept[0]] >= 64).any()
    public, enc_form, _ = _searches(s.m, which)
    with torch.no_grad():
        want = _mapped(enc_form(s.m, s.gathered(fmap, kept), kept, W), fmap)
        got = public(s.xs, s.xlen, W=W, skip_blank=THR)
    # (the best-first search cuts its list B in insertion order: at W = 1 that is always the root's blank child, the
    # empty sequence - its W = 1 case compares scores alone)
    assert len(got) == 3 and (sum(len(t) for r in got for t in r.tokens) > 0) == ((which, W) != ("best_first", 1))
    for b in range(3):
        _same_bits(got[b], want[b])
        for f in got[b].frames:
            assert f.dtype == np.int32 and np.isin(f, fmap[b, :kept[b]]).all()


@pytest.mark.parametrize("which", ["sync", "best_first"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_threshold_one_is_the_search_without_skipping(hip_lib, dtype, which):
    s = _setup(dtype)
    _, kept, _ = _separated(s, 1.0)
    assert kept.tolist() == s.lens.tolist()
    public, _, _ = _searches(s.m, which)
    with torch.no_grad():
        got = public(s.xs, s.xlen, W=4, skip_blank=1.0)
        want = public(s.xs, s.xlen, W=4, skip_blank=None)
    for b in range(3):
        _same_bits(got[b], want[b])
    assert sum(len(t) for r in got for t in r.tokens) > 0


@pytest.mark.parametrize("which", ["sync", "best_first"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_a_wholly_skipped_utterance_is_empty_and_leaves_its_neighbours_alone(hip_lib, dtype, which):
    s = _setup(dtype)

    def all_blank(z):
        z[1, :, 0] += 40.0

    fmap, kept, _ = _separated(s, THR, all_blank)
    assert kept[1] == 0 and kept[0] > 0 and kept[2] > 0
    public, enc_form, best = _searches(s.m, which)
    with torch.no_grad():
        want = _mapped(enc_form(s.m, s.gathered(fmap, kept), kept, 4), fmap)
        got = public(s.xs, s.xlen, W=4, skip_blank=THR)
    assert len(got[1]) == 1 and len(got[1].tokens[0]) == 0 and len(got[1].frames[0]) == 0 and got[1].logp[0] == 0.0
    for b in range(3):
        _same_bits(got[b], want[b])
    assert sum(len(t) for t in got[0].tokens) > 0 and sum(len(t) for t in got[2].tokens) > 0
    # ... and with the best-of forms
    with torch.no_grad():
        seqs, scores = best(s.xs, s.xlen, W=4, skip_blank=THR)
    for b in range(3):
        assert np.array_equal(seqs[b], got[b].tokens[0])
    assert len(seqs[1]) == 0 and scores[1].item() == 0.0


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_every_utterance_wholly_skipped(hip_lib, dtype):
    s = _setup(dtype)

    def all_blank(z):
        z[:, :, 0] += 40.0

    _, kept, _ = _separated(s, THR, all_blank)
    assert not kept.any()
    with torch.no_grad():
        for fn in (s.m.sync_beam_search_nbest, s.m.beam_search_nbest):
            for r in fn(s.xs, s.xlen, W=4, skip_blank=THR):
                assert len(r) == 1 and len(r.tokens[0]) == 0 and r.logp[0] == 0.0
        for fn in (s.m.sync_beam_search, s.m.beam_search):
            seqs, scores = fn(s.xs, s.xlen, W=4, skip_blank=THR)
            assert all(len(q) == 0 for q in seqs) and (scores == 0).all()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_lm_and_bias_pass_through(hip_lib, dtype):
    from edgedict_amd import decode
    from edgedict_amd.bias import ContextGraph
    s = _setup(dtype)
    fmap, kept, _ = _separated(s, THR)
    kw = dict(lm=_lm(_lm_sd(40, 16, 32, 2, seed=2, scale=4.0), dtype), lm_weight=0.6, length_bonus=0.3, lm_bos=1,
              bias=ContextGraph([[17, 39]], 2.5, CFG["vocab_size"]))
    with torch.no_grad():
        want = _mapped(decode.sync_beam_search_nbest_enc(s.m, s.gathered(fmap, kept), kept, 4, **kw), fmap)
        got = s.m.sync_beam_search_nbest(s.xs, s.xlen, W=4, skip_blank=THR, **kw)
        plain = _mapped(decode.sync_beam_search_nbest_enc(s.m, s.gathered(fmap, kept), kept, 4), fmap)
    for b in range(3):
        _same_bits(got[b], want[b])
    assert any(not np.array_equal(g.logp, p.logp) for g, p in zip(got, plain))      # the fusion did act
