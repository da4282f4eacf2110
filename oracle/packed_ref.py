"""ORACLE (test infrastructure only - never imported by the product path).

Float64 restatement of the joint network + RNN-T loss on the PACKED lattice (edgedict_amd.models._JointLossFn):
only the cells inside each utterance's (T_b, U_b + 1) box exist, and the row of cell (b, t, u) is

    off[b] + t (U_b + 1) + u,        off[b] = sum_{b' < b} T_b' (U_b' + 1).

Everything here is plain torch on the CPU, one utterance at a time, written from this project's own oracle: the
joint's hidden layer is ``oracle/models_ref.joint_forward`` with its first Linear already applied
(tanh(E1[b, t] + D1[b, u])), the loss is ``oracle/rnnt_loss_ref.rnnt_loss_torch_fast`` run on each utterance's own
box.  ``joint_hidden`` is differentiable, so autograd through it gives the packed chain's gradients.

PARITY STATUS: pinned by tests/test_packed_ref_host.py against the dense oracle on padded tensors and against
oracle/rnnt_loss_bruteforce.py.
"""
import torch

from . import rnnt_loss_ref as R


def _lens(act_lens, label_lens):
    al = [int(x) for x in act_lens]
    ll = [int(x) for x in label_lens]
    assert len(al) == len(ll) and all(t >= 1 for t in al) and all(u >= 0 for u in ll)
    return al, ll


def offsets(act_lens, label_lens):
    """(off int64 [B], M): first packed row of every utterance and the number of rows."""
    al, ll = _lens(act_lens, label_lens)
    off, m = [], 0
    for t, u in zip(al, ll):
        off.append(m)
        m += t * (u + 1)
    return torch.tensor(off, dtype=torch.int64), m


def pack(dense, act_lens, label_lens):
    """dense [B, T, U1, ...] -> packed [M, ...]: the cells of every box in (b, t, u) order."""
    al, ll = _lens(act_lens, label_lens)
    rest = dense.shape[3:]
    return torch.cat([dense[b, :t, :u + 1].reshape(t * (u + 1), *rest) for b, (t, u) in enumerate(zip(al, ll))], 0)


def unpack(packed, act_lens, label_lens, T=None, U1=None, fill=0.0):
    """packed [M, ...] -> dense [B, T, U1, ...] with ``fill`` outside the boxes (T, U1 default to the longest box)."""
    al, ll = _lens(act_lens, label_lens)
    T = max(al) if T is None else T
    U1 = max(ll) + 1 if U1 is None else U1
    off, m = offsets(al, ll)
    assert packed.shape[0] == m, (packed.shape, m)
    out = packed.new_full((len(al), T, U1) + tuple(packed.shape[1:]), fill)
    for b, (t, u) in enumerate(zip(al, ll)):
        o = int(off[b])
        out[b, :t, :u + 1] = packed[o:o + t * (u + 1)].reshape(t, u + 1, *packed.shape[1:])
    return out


def joint_hidden(E1, D1, act_lens, label_lens):
    """E1 [B, T, J], D1 [B, U1, J] -> packed tanh(E1[b, t] + D1[b, u]) [M, J] (float64, differentiable)."""
    al, ll = _lens(act_lens, label_lens)
    E1, D1 = E1.double(), D1.double()
    J = E1.shape[-1]
    return torch.cat([torch.tanh(E1[b, :t, None, :] + D1[b, None, :u + 1, :]).reshape(t * (u + 1), J)
                      for b, (t, u) in enumerate(zip(al, ll))], 0)


def joint_hidden_bwd(dhid, hid, act_lens, label_lens, T=None, U1=None):
    """Backward of ``joint_hidden`` from the packed [M, J] gradient and output:
    dpre = dhid (1 - hid^2);  dE1[b, t] = sum_u dpre;  dD1[b, u] = sum_t dpre;  exact zeros outside the boxes."""
    al, ll = _lens(act_lens, label_lens)
    T = max(al) if T is None else T
    U1 = max(ll) + 1 if U1 is None else U1
    off, m = offsets(al, ll)
    assert dhid.shape == hid.shape and hid.shape[0] == m
    J = hid.shape[1]
    dpre = dhid.double() * (1.0 - hid.double() ** 2)
    dE1 = torch.zeros(len(al), T, J, dtype=torch.float64)
    dD1 = torch.zeros(len(al), U1, J, dtype=torch.float64)
    for b, (t, u) in enumerate(zip(al, ll)):
        o = int(off[b])
        box = dpre[o:o + t * (u + 1)].reshape(t, u + 1, J)
        dE1[b, :t] = box.sum(1)
        dD1[b, :u + 1] = box.sum(0)
    return dE1, dD1


def loss_from_packed_logits(logits, labels, act_lens, label_lens, blank=0):
    """logits [M, V] (packed), labels int [B, >= max U_b] -> (costs [B], dlogits [M, V]) in float64:
    per-utterance costs and the gradient of their SUM.  Every utterance is run through the DP oracle on its own
    (T_b, U_b + 1) box, so no cell outside a box - there is none in the packed layout - can enter."""
    al, ll = _lens(act_lens, label_lens)
    off, m = offsets(al, ll)
    assert logits.dim() == 2 and logits.shape[0] == m, (logits.shape, m)
    V = logits.shape[1]
    labels = torch.as_tensor(labels)
    costs = torch.zeros(len(al), dtype=torch.float64)
    grads = torch.empty(m, V, dtype=torch.float64)
    for b, (t, u) in enumerate(zip(al, ll)):
        o, n = int(off[b]), t * (u + 1)
        box = logits[o:o + n].detach().double().reshape(1, t, u + 1, V)
        c, g = R.rnnt_loss_torch_fast(box, labels[b:b + 1, :u], torch.tensor([t]), torch.tensor([u]), blank=blank)
        costs[b] = c[0]
        grads[o:o + n] = g.reshape(n, V)
    return costs, grads
