"""GPU: training the LSTM language model on the engine - LMModel.loss / forward / score, LMTrainer - against a float64 CPU
restatement of the reference's model and loop (models.py:224-261, cli/train_lm.py:60-93) from nn.Embedding, nn.LSTM,
nn.Linear, log_softmax and NLLLoss(ignore_index=0), built from the same reference-keyed state dict.

Models: LMModel(40, 16, 32, 2, dropout=0) and the tied LMModel(40, 32, 32, 1, tie_weights=True).  Batch: B = 3, T = 7,
ragged, padded with 0; sentence 0 holds token 0 in its middle, so token 0 occurs as an INPUT in front of a valid target
(the reference's nn.Embedding has no padding_idx: row 0 must receive gradient)."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PLAIN = (40, 16, 32, 2, False)
TIED = (40, 32, 32, 1, True)
SENTENCES = [[12, 0, 7, 39, 3, 21, 8], [30, 5, 17, 2], [9, 26, 38, 14, 6]]
TRAIN_STEPS, TRAIN_LR = 40, 2e-2


def _lm_sd(ntoken, ninp, nhid, nlayers, tied, seed=3):
    """A reference-keyed LMModel state dict (the keys torch.save(model.state_dict()) writes in cli/train_lm.py:109)."""
    torch.manual_seed(seed)
    emb = torch.nn.Embedding(ntoken, ninp)
    rnn = torch.nn.LSTM(ninp, nhid, nlayers, batch_first=True)
    dec = torch.nn.Linear(nhid, ntoken)
    sd = {"encoder.weight": emb.weight.detach().clone() * 0.5}
    sd.update({"rnn." + k: v.detach().clone() for k, v in rnn.state_dict().items()})
    sd["decoder.weight"] = sd["encoder.weight"] if tied else dec.weight.detach().clone()
    sd["decoder.bias"] = dec.bias.detach().clone()
    return sd


def _batch():
    from edgedict_amd.lm import seq_collate
    return seq_collate([torch.tensor(s) for s in SENTENCES])


class RefLM(torch.nn.Module):
    """The reference's LMModel restated in float64 on the CPU (dropout 0)."""

    def __init__(self, sd, tied):
        super().__init__()
        ntoken, ninp = sd["encoder.weight"].shape
        nhid = sd["rnn.weight_hh_l0"].shape[1]
        nl = sum(1 for k in sd if k.startswith("rnn.weight_hh_l"))
        self.encoder = torch.nn.Embedding(ntoken, ninp)
        self.rnn = torch.nn.LSTM(ninp, nhid, nl, batch_first=True)
        self.decoder = torch.nn.Linear(nhid, ntoken)
        if tied:
            self.decoder.weight = self.encoder.weight
        self.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
        self.double()

    def forward(self, inputs):
        out, _ = self.rnn(self.encoder(inputs))
        return torch.log_softmax(self.decoder(out).reshape(-1, self.decoder.out_features), dim=-1)

    def loss(self, inputs, targets):
        return torch.nn.NLLLoss(ignore_index=0)(self(inputs), targets.flatten())


@functools.lru_cache(maxsize=None)
def _reference(cfg):
    """-> (loss, {name: gradient}, log-probs [B * T, V]) of the float64 restatement on the fixed batch."""
    sd = _lm_sd(*cfg)
    ref = RefLM(sd, cfg[4])
    inputs, targets = _batch()
    loss = ref.loss(inputs, targets)
    loss.backward()
    with torch.no_grad():
        logp = ref(inputs)
    return loss.item(), {k: p.grad.clone() for k, p in ref.named_parameters()}, logp


def reference_curve(cfg, steps, lr):
    """The restatement trained as cli/train_lm.py:86-93 does (Adam, clip_grad_norm_ 1.0) on the fixed batch: the loss
    before every step, and after the last."""
    ref = RefLM(_lm_sd(*cfg), cfg[4])
    opt = torch.optim.Adam(ref.parameters(), lr=lr)
    inputs, targets = _batch()
    curve = []
    for _ in range(steps):
        ref.zero_grad()
        loss = ref.loss(inputs, targets)
        curve.append(loss.item())
        loss.backward()
        torch.nn.utils.clip_grad_norm_(ref.parameters(), 1.0)
        opt.step()
    with torch.no_grad():
        curve.append(ref.loss(inputs, targets).item())
    return curve


def _engine(cfg, dtype="fp32", dropout=0.0, train=True):
    from edgedict_amd.lm import LMModel
    ntoken, ninp, nhid, nl, tied = cfg
    lm = LMModel(ntoken, ninp, nhid, nl, dropout=dropout, tie_weights=tied)
    lm.load_state_dict(_lm_sd(*cfg), strict=True)
    lm = lm.cuda()
    assert (lm.decoder.weight is lm.encoder.weight) == tied
    lm.compute_dtype = dtype
    return lm.train(train)


def _check_grads(lm, grads, what):
    worst = 0.0
    names = [n for n, _ in lm.named_parameters()]
    assert set(names) == set(grads), (names, sorted(grads))
    for name, p in lm.named_parameters():
        ref = grads[name]
        assert p.grad is not None, name
        got = p.grad.double().cpu()
        err = (got - ref).abs().max().item() / max(ref.abs().max().item(), 1e-6)
        worst = max(worst, err)
        assert err < 2e-3, (what, name, err)
    return worst


@pytest.mark.parametrize("flat", [False, True], ids=["autograd", "flat"])
@pytest.mark.parametrize("cfg", [PLAIN, TIED], ids=["plain", "tied"])
def test_fp32_loss_and_gradients_match_the_restatement(hip_lib, cfg, flat):
    """model.loss within 1e-5 relative; every parameter gradient max|got - ref| / max|ref| < 2e-3 - with plain autograd
    accumulation, and with FlatParams (the weight gradients accumulate in place on the auxiliary stream).  The tied
    parameter holds the sum of the embedding's and the decoder's gradients (the restatement's autograd sum); embedding
    row 0 receives gradient."""
    from edgedict_amd.optim import FlatParams
    want, grads, _ = _reference(cfg)
    lm = _engine(cfg)
    fp = FlatParams(lm) if flat else None
    inputs, targets = _batch()
    loss, (h, c) = lm.loss(inputs.cuda(), targets.cuda())
    assert loss.dim() == 0 and not h.requires_grad and not c.requires_grad
    assert h.shape == c.shape == (cfg[3], 3, cfg[2])
    loss.backward()
    torch.cuda.synchronize()
    rel = abs(loss.item() - want) / want
    worst = _check_grads(lm, grads, "loss")
    print("lm.loss", cfg, "flat" if flat else "autograd", "loss rel err %.3g, worst gradient err %.3g" % (rel, worst))
    assert rel < 1e-5, (loss.item(), want)
    assert lm.encoder.weight.grad[0].abs().max().item() > 0
    assert grads["encoder.weight"][0].abs().max().item() > 0
    if flat:
        assert lm.encoder.weight.grad.data_ptr() == fp.grad.data_ptr() + 4 * fp.offsets[0]


@pytest.mark.parametrize("cfg", [PLAIN, TIED], ids=["plain", "tied"])
def test_reference_loop_runs_as_written(hip_lib, cfg):
    """cli/train_lm.py:85-91: init_hidden, model(inputs, hidden), NLLLoss(ignore_index=0)(logits, targets.flatten()),
    backward - the same loss and gradients as model.loss, within the same bounds."""
    want, grads, logp = _reference(cfg)
    lm = _engine(cfg)
    inputs, targets = _batch()
    inputs, targets = inputs.cuda(), targets.cuda()
    hidden = lm.init_hidden(inputs.shape[0])
    lm.zero_grad()
    logits, _ = lm(inputs, hidden)
    assert logits.dtype == torch.float32 and logits.shape == (21, 40)
    loss = torch.nn.NLLLoss(ignore_index=0)(logits, targets.flatten())
    loss.backward()
    rel = abs(loss.item() - want) / want
    e_lp = (logits.detach().double().cpu() - logp).abs().max().item()
    worst = _check_grads(lm, grads, "reference loop")
    print("reference loop", cfg, "loss rel err %.3g, log-prob err %.3g, worst gradient err %.3g" % (rel, e_lp, worst))
    assert rel < 1e-5, (loss.item(), want)


def test_forward_under_no_grad_is_bit_equal_to_frozen_parameters(hip_lib):
    """Regression guard: the differentiable path changes nothing of what forward computes."""
    inputs, _ = _batch()
    inputs = inputs.cuda()
    for dtype in ("fp32", "bf16"):
        lm = _engine(PLAIN, dtype, train=False)
        live, (hl, cl) = lm(inputs, lm.init_hidden(3))
        assert live.requires_grad
        with torch.no_grad():
            a, (ha, ca) = lm(inputs, lm.init_hidden(3))
        for p in lm.parameters():
            p.requires_grad_(False)
        b, (hb, cb) = lm(inputs, lm.init_hidden(3))
        assert not a.requires_grad and not b.requires_grad
        assert torch.equal(a, b) and torch.equal(ha, hb) and torch.equal(ca, cb)
        assert torch.equal(live.detach(), a) and torch.equal(hl, ha) and torch.equal(cl, ca)


@pytest.mark.parametrize("cfg", [PLAIN, TIED], ids=["plain", "tied"])
def test_bf16_loss_is_close_to_fp32_and_gradients_are_finite(hip_lib, cfg):
    """Loss within 2e-2 relative of fp32 (the bound of test_stack_and_per_layer_steps_agree_in_bf16)."""
    inputs, targets = _batch()
    out = {}
    for dtype in ("fp32", "bf16"):
        lm = _engine(cfg, dtype)
        loss, _ = lm.loss(inputs.cuda(), targets.cuda())
        loss.backward()
        out[dtype] = loss.item()
        for name, p in lm.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all(), (dtype, name)
            assert p.grad.abs().max().item() > 0, (dtype, name)
    rel = abs(out["bf16"] - out["fp32"]) / out["fp32"]
    print("lm.loss bf16 vs fp32", cfg, "rel %.3g" % rel)
    assert rel < 2e-2, out


def test_score_is_the_sum_of_forwards_gathered_log_probs(hip_lib):
    """score(tokens, lengths) = sum over each sentence's tokens of forward's log-prob of that token (atol 1e-4, fp32),
    and what lies in the padded tail does not change it."""
    lm = _engine(PLAIN, train=False)
    inputs, targets = _batch()
    lengths = torch.tensor([len(s) for s in SENTENCES])
    with torch.no_grad():
        logp, _ = lm(inputs.cuda(), None)
    logp = logp.view(3, 7, 40).double().cpu()
    want = torch.stack([sum(logp[b, u, SENTENCES[b][u]] for u in range(len(SENTENCES[b]))) for b in range(3)])
    got = lm.score(targets, lengths)
    assert got.dtype == torch.float32 and got.shape == (3,) and not got.requires_grad
    junk = targets.clone()
    junk[1, 4:] = torch.tensor([33, 0, 39])
    junk[2, 5:] = 11
    wider = torch.cat([junk, torch.full((3, 2), 5)], 1)
    err = (got.double().cpu() - want).abs().max().item()
    print("lm.score: max err %.3g" % err)
    assert err <= 1e-4
    assert torch.equal(lm.score(junk, lengths), got)
    assert torch.equal(lm.score(junk, lengths, check_tokens=True), got)      # junk behind a sentence's end is not checked
    bad = targets.clone()
    bad[0, 6] = 40          # the last token: an input to nothing
    with pytest.raises(ValueError, match="outside"):
        lm.score(bad, lengths, check_tokens=True)
    assert (lm.score(bad, lengths) > got).tolist() == [True, False, False]     # unchecked: the token adds an exact 0
    assert (lm.score(wider.cuda(), lengths.cuda()).cpu() - got.cpu()).abs().max().item() <= 1e-4
    # the whole-sentence log-probability of the restatement
    _, _, ref_logp = _reference(PLAIN)
    ref_logp = ref_logp.view(3, 7, 40)
    ref = torch.stack([sum(ref_logp[b, u, SENTENCES[b][u]] for u in range(len(SENTENCES[b]))) for b in range(3)])
    assert (got.double().cpu() - ref).abs().max().item() <= 1e-4


def test_trainer_learns_one_batch(hip_lib):
    """On one fixed batch the loss after TRAIN_STEPS = 40 steps at lr = 2e-2 is below half the initial loss.

    N and lr were chosen on the CPU: the float64 restatement with torch.optim.Adam and clip_grad_norm_(1.0)
    (reference_curve(PLAIN, 40, 2e-2)) goes
        step  0: 3.7063   step 10: 1.9845   step 20: 0.9389   step 30: 0.5151   step 40: 0.3392
    i.e. it is below a quarter of its initial loss (0.9266) from step 21 on and at 9.2 % of it at step 40."""
    from edgedict_amd.lm import LMTrainer
    lm = _engine(PLAIN)
    tr = LMTrainer(lm, lr=TRAIN_LR, max_grad_norm=1.0)
    inputs, targets = _batch()
    inputs, targets = inputs.cuda(), targets.cuda()
    losses = [tr.train_step(inputs, targets) for _ in range(TRAIN_STEPS)]
    assert all(l.is_cuda and l.dim() == 0 and not l.requires_grad for l in losses)
    first, _ = _reference(PLAIN)[:2]
    mean, ppl = tr.evaluate([(inputs, targets)])
    curve = [l.item() for l in losses]
    print("trainer: loss %.4f -> %.4f after %d steps (evaluate: %.4f, perplexity %.3f)"
          % (curve[0], mean, TRAIN_STEPS, mean, ppl))
    assert abs(curve[0] - first) / first < 1e-5
    assert np.isfinite(curve).all()
    assert mean < 0.5 * curve[0], (curve[0], mean)
    assert abs(ppl - np.exp(mean)) < 1e-9 * ppl
    assert lm.training        # evaluate restores the mode


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_training_with_dropout_runs_and_gives_finite_gradients(hip_lib, dtype):
    from edgedict_amd.lm import LMTrainer
    lm = _engine(PLAIN, dtype, dropout=0.5)
    tr = LMTrainer(lm, lr=1e-3)
    inputs, targets = _batch()
    loss = tr.train_step(inputs.cuda(), targets.cuda())
    assert torch.isfinite(loss).all()
    for name, p in lm.named_parameters():
        assert torch.isfinite(p.grad).all() and torch.isfinite(p).all(), name
    assert tr.optimizer.grad_norm.item() > 0


def test_saved_checkpoint_loads_strictly_and_fuses_into_the_beam_search(hip_lib, tmp_path):
    """save -> a fresh LMModel.load_state_dict(strict=True) -> FusionLM -> a W = 2 beam search with lm= on the tiny
    transducer."""
    from edgedict_amd.lm import FusionLM, LMModel, LMTrainer
    from edgedict_amd.models import Transducer
    lm = _engine(PLAIN)
    tr = LMTrainer(lm, lr=1e-3)
    inputs, targets = _batch()
    tr.train_step(inputs.cuda(), targets.cuda())
    path = str(tmp_path / "librispeech_lm_model.pt")
    tr.save(path)
    sd = torch.load(path)
    assert set(sd) == set(_lm_sd(*PLAIN)) and all(v.device.type == "cpu" for v in sd.values())
    fresh = LMModel(40, 16, 32, 2)
    fresh.load_state_dict(sd, strict=True)
    fresh = fresh.cuda().eval()
    for k, v in lm.state_dict().items():
        assert torch.equal(fresh.state_dict()[k], v), k
    assert not torch.equal(sd["decoder.weight"], _lm_sd(*PLAIN)["decoder.weight"])     # the step did move the weights
    fused = FusionLM(fresh, torch.float32, 0.3)
    assert (fused.L, fused.E, fused.H, fused.V) == (2, 16, 32, 40)
    G = np.load(os.path.join(os.path.dirname(__file__), "golden", "beam_tiny.npz"))
    cfg = dict(vocab_embed_size=16, vocab_size=40, input_size=24, enc_hidden_size=32, enc_layers=2,
               enc_proj_size=24, dec_hidden_size=32, dec_layers=2, dec_proj_size=24, joint_size=32)
    m = Transducer(enc_dropout=0.0, dec_dropout=0.0, output_loss=False, **cfg)
    m.load_state_dict({k[3:]: torch.from_numpy(G[k]) for k in G.files if k.startswith("sd/")}, strict=True)
    m = m.cuda().eval()
    m.compute_dtype = "fp32"
    xs, xlen = torch.from_numpy(G["xs"]), torch.from_numpy(G["xlen"])
    with torch.no_grad():
        seqs, scores = m.beam_search(xs.cuda(), xlen, W=2, max_expansions=400, lm=fresh, lm_weight=0.3)
    assert len(seqs) == xs.shape[0] and all(np.isfinite(float(s)) for s in scores)
