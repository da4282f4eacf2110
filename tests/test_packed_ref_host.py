"""Host: the float64 restatement of the packed joint + loss chain (oracle/packed_ref.py) is pinned before any kernel
is measured against it (tests/test_packed_lattice_gpu.py): the packing round-trips, the packed chain equals the dense
oracle on padded tensors whatever the padding holds, and on tiny lattices costs and gradients equal the sum over all
alignments (oracle/rnnt_loss_bruteforce.py) for a blank at either end of the vocabulary."""
import numpy as np
import pytest
import torch

from oracle import models_ref as M
from oracle import packed_ref as PR
from oracle import rnnt_loss_bruteforce as BF
from oracle import rnnt_loss_ref as R

# (act_lens, label_lens): the longest utterance is not always row 0
BATCHES = [
    ([5, 5, 5], [3, 3, 3]),                 # all full
    ([4, 9, 2, 7], [1, 6, 3, 2]),           # one full + ragged
    ([6, 3, 6, 2], [0, 4, 2, 4]),           # an utterance with U_b = 0
    ([1, 8, 5], [2, 5, 5]),                 # an utterance with T_b = 1
    ([3, 1, 7, 7], [2, 0, 4, 1]),           # a one-cell box
    ([6], [4]),                             # B = 1
    ([1], [0]),                             # B = 1, one cell
]


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


@pytest.mark.parametrize("al,ll", BATCHES)
def test_pack_unpack_round_trip(al, ll):
    B, T, U1 = len(al), max(al), max(ll) + 1
    off, m = PR.offsets(al, ll)
    assert m == sum(t * (u + 1) for t, u in zip(al, ll))
    assert off.tolist() == [sum(t * (u + 1) for t, u in list(zip(al, ll))[:b]) for b in range(B)]
    dense = torch.randn(B, T, U1, 3, generator=_gen(1), dtype=torch.float64)
    packed = PR.pack(dense, al, ll)
    assert packed.shape == (m, 3)
    # the stated row order, cell by cell
    for b in range(B):
        for t in range(al[b]):
            for u in range(ll[b] + 1):
                assert torch.equal(packed[int(off[b]) + t * (ll[b] + 1) + u], dense[b, t, u])
    back = PR.unpack(packed, al, ll, fill=-7.5)
    inside = (torch.arange(T)[None, :, None] < torch.tensor(al)[:, None, None]) & \
             (torch.arange(U1)[None, None, :] <= torch.tensor(ll)[:, None, None])
    assert torch.equal(back[inside], dense[inside])
    assert (back[~inside] == -7.5).all()
    assert torch.equal(PR.pack(back, al, ll), packed)
    # no trailing dimensions, explicit extents
    flat = torch.arange(m, dtype=torch.float64)
    wide = PR.unpack(flat, al, ll, T=T + 2, U1=U1 + 1, fill=0.0)
    assert wide.shape == (B, T + 2, U1 + 1) and torch.equal(PR.pack(wide, al, ll), flat)


@pytest.mark.parametrize("blank", [0, 2, 10])
@pytest.mark.parametrize("al,ll", BATCHES)
def test_packed_chain_equals_dense_oracle_on_padded_tensors(al, ll, blank):
    B, T, U1 = len(al), max(al), max(ll) + 1
    P, P2, J, V = 5, 4, 6, 11
    g = _gen(100 * B + T + blank)
    enc = torch.randn(B, T, P, generator=g, dtype=torch.float64)
    dec = torch.randn(B, U1, P2, generator=g, dtype=torch.float64)
    sd = {"joint.joint.0.weight": torch.randn(J, P + P2, generator=g, dtype=torch.float64),
          "joint.joint.0.bias": torch.randn(J, generator=g, dtype=torch.float64),
          "joint.joint.2.weight": torch.randn(V, J, generator=g, dtype=torch.float64),
          "joint.joint.2.bias": torch.randn(V, generator=g, dtype=torch.float64)}
    labels = torch.randint(0, V, (B, U1 - 1), generator=g, dtype=torch.int32)
    w1 = sd["joint.joint.0.weight"]
    # dense oracle
    dense_logits = M.joint_forward(sd, enc, dec).clone().requires_grad_(True)
    costs_d, grads_d = R.rnnt_loss_torch_fast(dense_logits.detach(), labels, torch.tensor(al), torch.tensor(ll), blank=blank)
    # packed restatement
    E1 = (enc @ w1[:, :P].t()).requires_grad_(True)
    D1 = (dec @ w1[:, P:].t() + sd["joint.joint.0.bias"]).requires_grad_(True)
    hid = PR.joint_hidden(E1, D1, al, ll)
    logits = hid @ sd["joint.joint.2.weight"].t() + sd["joint.joint.2.bias"]
    assert (logits.detach() - PR.pack(dense_logits.detach(), al, ll)).abs().max().item() <= 1e-12
    costs_p, grads_p = PR.loss_from_packed_logits(logits, labels, al, ll, blank=blank)
    assert ((costs_p - costs_d).abs() <= 1e-12 * costs_d.abs()).all(), (costs_p, costs_d)
    assert (grads_p - PR.pack(grads_d, al, ll)).abs().max().item() <= 1e-12
    # whatever the padding holds, the dense oracle sees the same thing: its gradient there is zero
    padded = PR.unpack(logits.detach(), al, ll, T=T, U1=U1, fill=3.25)
    costs_f, grads_f = R.rnnt_loss_torch_fast(padded, labels, torch.tensor(al), torch.tensor(ll), blank=blank)
    assert ((costs_p - costs_f).abs() <= 1e-12 * costs_f.abs()).all()
    assert torch.equal(PR.unpack(PR.pack(grads_f, al, ll), al, ll, T=T, U1=U1, fill=0.0), grads_f)
    assert (grads_p - PR.pack(grads_f, al, ll)).abs().max().item() <= 1e-12
    # the numpy recursion (independent loops) agrees too
    costs_n, grads_n = R.rnnt_loss(padded.numpy(), labels.numpy(), al, ll, blank=blank)
    assert np.abs(costs_p.numpy() - costs_n).max() <= 1e-12 * np.abs(costs_n).max()
    assert np.abs(PR.unpack(grads_p, al, ll, T=T, U1=U1).numpy() - grads_n).max() <= 1e-12
    # joint_hidden_bwd is autograd through joint_hidden, with exact zeros outside the boxes
    dhid = torch.randn(hid.shape, generator=g, dtype=torch.float64)
    hid.backward(dhid)
    dE1, dD1 = PR.joint_hidden_bwd(dhid, hid.detach(), al, ll, T=T, U1=U1)
    assert (dE1 - E1.grad).abs().max().item() <= 1e-12 and (dD1 - D1.grad).abs().max().item() <= 1e-12
    dense_dp = PR.unpack(dhid * (1.0 - hid.detach() ** 2), al, ll, T=T, U1=U1, fill=0.0)
    assert (dE1 - dense_dp.sum(2)).abs().max().item() <= 1e-12 and (dD1 - dense_dp.sum(1)).abs().max().item() <= 1e-12
    for b in range(B):
        assert (dE1[b, al[b]:] == 0).all() and (dD1[b, ll[b] + 1:] == 0).all()


@pytest.mark.parametrize("T,U1,V,seed", [(1, 1, 2, 0), (2, 3, 5, 1), (3, 2, 3, 2), (4, 4, 5, 3), (4, 3, 2, 4), (3, 4, 4, 5)])
def test_packed_loss_equals_the_sum_over_all_alignments(T, U1, V, seed):
    """The lattices of test_rnnt_loss_gpu.test_hip_loss_equals_the_sum_over_all_alignments, packed."""
    rng = np.random.default_rng(900 + seed)
    B = 4
    acts = (2.0 * rng.normal(size=(B, T, U1, V))).astype(np.float32)
    labels = rng.integers(1, V, size=(B, max(U1 - 1, 1))).astype(np.int32)[:, :U1 - 1]
    al = rng.integers(1, T + 1, size=B).astype(np.int32)
    ll = rng.integers(0, U1, size=B).astype(np.int32)
    al[0], ll[0] = T, U1 - 1
    for blank in sorted({0, 1, V - 1}):
        c_bf, g_bf = BF.rnnt_loss(acts.astype(np.float64), labels, al, ll, blank=blank)
        packed = PR.pack(torch.tensor(acts).double(), al, ll)
        costs, grads = PR.loss_from_packed_logits(packed, torch.tensor(labels), al, ll, blank=blank)
        np.testing.assert_allclose(costs.numpy(), c_bf, rtol=1e-12, atol=0)
        np.testing.assert_allclose(PR.unpack(grads, al, ll, T=T, U1=U1, fill=0.0).numpy(), g_bf, rtol=0, atol=1e-12)
