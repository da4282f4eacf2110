"""CPU: hit / miss of the weight-image caches (models._WeightCache, encoder_stack.packed_weights) for every way of changing
a weight that needs no device.  The kernels behind a miss (ops.cast / ops.transpose / ops.lstm_pack_weights, the native
stack packer) are replaced by counting torch stand-ins: what is asserted is WHEN an image is rebuilt, and that the image
then holds the new values.  tests/test_weight_coherence_gpu.py checks the same routes end to end on the device."""
import gc
import types
import weakref

import pytest
import torch
from torch import nn

BF16, F32 = torch.bfloat16, torch.float32
KINDS = [(BF16, False), (F32, True), (BF16, True), (F32, "lstm_fwd"), (F32, "lstm_bwd")]


@pytest.fixture
def cache(monkeypatch):
    from edgedict_amd import models, ops
    calls = []

    def cast(src, dtype):
        calls.append("cast")
        return src.to(dtype)

    def transpose(src, dtype):
        calls.append("transpose")
        return src.t().contiguous().to(dtype)

    def pack(src, fwd, bwd):
        calls.append("pack")
        return (src * 2.0 if fwd else None, src * 3.0 if bwd else None)

    monkeypatch.setattr(ops, "cast", cast)
    monkeypatch.setattr(ops, "transpose", transpose)
    monkeypatch.setattr(ops, "lstm_pack_weights", pack)
    c = models._WeightCache()
    c.calls = calls
    return c


def _expect(p, dtype, kind):
    w = p.detach()
    if kind == "lstm_fwd":
        return w * 2.0
    if kind == "lstm_bwd":
        return w * 3.0
    return (w.t().contiguous() if kind else w).to(dtype)


def _warm(cache, p):
    imgs = [cache.get(p, d, k) for d, k in KINDS]
    n = len(cache.calls)
    assert n == len(KINDS)
    assert all(cache.get(p, d, k) is o for (d, k), o in zip(KINDS, imgs))
    assert len(cache.calls) == n                               # all hits
    del cache.calls[:]
    return imgs


def _assert_fresh(cache, p, old):
    """Every kind of image misses once, holds p's current values, and hits afterwards."""
    for (d, k), o in zip(KINDS, old):
        n = len(cache.calls)
        img = cache.get(p, d, k)
        assert len(cache.calls) == n + 1, (d, k)
        assert img is not o
        assert torch.equal(img, _expect(p, d, k)), (d, k)
        assert cache.get(p, d, k) is img and len(cache.calls) == n + 1


def _lin():
    torch.manual_seed(0)
    return nn.Linear(8, 12)


def _adam(**kw):
    def make(params):
        return torch.optim.Adam(params, lr=0.1, **kw)
    return make


ROUTES = {}


def route(name):
    def deco(fn):
        ROUTES[name] = fn
        return fn
    return deco


def _opt_step(m, make):
    opt = make([m.weight])
    m.weight.grad = torch.ones_like(m.weight)
    opt.step()


@route("sgd")
def _(m):
    _opt_step(m, lambda ps: torch.optim.SGD(ps, lr=0.1))


@route("adam")
def _(m):
    _opt_step(m, _adam())


@route("adam_foreach")
def _(m):
    _opt_step(m, _adam(foreach=True))


@route("adam_fused")
def _(m):
    try:
        opt = _adam(fused=True)([m.weight])
    except (RuntimeError, TypeError, ValueError) as exc:       # this torch build has no fused Adam for CPU tensors
        pytest.skip("no fused Adam on the CPU here: %s" % exc)
    m.weight.grad = torch.ones_like(m.weight)
    opt.step()


@route("no_grad_mul_")
def _(m):
    with torch.no_grad():
        m.weight.mul_(0.5)


@route("load_state_dict")
def _(m):
    m.load_state_dict({k: v * 0.5 for k, v in m.state_dict().items()})


@route("load_state_dict_assign")
def _(m):
    m.load_state_dict({k: v * 0.5 for k, v in m.state_dict().items()}, assign=True)


@route("new_parameter")
def _(m):
    m.weight = nn.Parameter(m.weight.detach() * 0.5)


@route("data_swap")
def _(m):
    m.weight.data = m.weight.detach() * 0.5


@route("data_swap_twice")
def _(m):
    new = m.weight.detach() * 0.5
    m.weight.data = m.weight.detach().clone()
    gc.collect()
    m.weight.data = new.clone()


@route("module_apply_round_trip")
def _(m):
    # what model.to(device) does to every parameter (`param.data = fn(param.data)`), with a change while it is away
    m.double()
    with torch.no_grad():
        m.weight.mul_(0.5)
    m.float()


@route("data_mul_then_weights_changed")
def _(m):
    import edgedict_amd
    m.weight.data.mul_(0.5)
    edgedict_amd.weights_changed()


@pytest.mark.parametrize("name", sorted(ROUTES))
def test_every_visible_route_misses_once_and_rebuilds_from_the_new_values(cache, name):
    m = _lin()
    before = m.weight.detach().clone()
    old = _warm(cache, m.weight)
    ROUTES[name](m)
    assert not torch.equal(m.weight.detach(), before)
    _assert_fresh(cache, m.weight, old)


def test_every_torch_optimizer_step_bumps_the_parameter_epoch():
    """torch's fused optimisers leave `_version` alone (observed: Adam(fused=True) on this build), so the version counter
    cannot be what makes a torch.optim step visible: the global step hook in config.py is."""
    from edgedict_amd import config
    m = _lin()
    for make in (lambda ps: torch.optim.SGD(ps, lr=0.1), _adam(), _adam(foreach=True)):
        epoch, ver = config.param_epoch(), m.weight._version
        _opt_step(m, make)
        assert config.param_epoch() == epoch + 1 and m.weight._version > ver
    # the one route that depends on the hook: the fused kernel changes the values and not the counter
    try:
        _adam(fused=True)([nn.Parameter(torch.zeros(1))])
    except (RuntimeError, TypeError, ValueError):
        return                                               # no fused Adam for CPU tensors in this build: the GPU file has it
    epoch, ver, before = config.param_epoch(), m.weight._version, m.weight.detach().clone()
    _opt_step(m, _adam(fused=True))
    assert not torch.equal(m.weight.detach(), before)
    assert m.weight._version == ver, "fused Adam now bumps _version: the hook in config.py is no longer the only witness"
    assert config.param_epoch() == epoch + 1


def test_a_write_through_data_is_invisible_until_weights_changed_is_called(cache):
    """The documented limit ("Changing weights"): `p.data` is a detached alias with a version counter of
    its own.  The cache keeps answering with the old images - this pins that the public call is what ends it."""
    import edgedict_amd
    from edgedict_amd import config
    m = _lin()
    old = _warm(cache, m.weight)
    n = len(cache.calls)
    m.weight.data.mul_(0.5)
    assert all(cache.get(m.weight, d, k) is o for (d, k), o in zip(KINDS, old)) and len(cache.calls) == n
    epoch = config.param_epoch()
    edgedict_amd.weights_changed()
    assert config.param_epoch() == epoch + 1
    _assert_fresh(cache, m.weight, old)


def test_an_entry_keeps_its_source_alive_so_the_address_cannot_come_back(cache):
    """`p.data = a; p.data = b` with no look-up in between: set_data keeps `_version`, so only the address tells b from the
    tensor the image was built from.  The entry holds that tensor: it outlives the swap, no later tensor can take its
    address, and when the entry is replaced the old source goes."""
    m = _lin()
    p = m.weight
    cache.get(p, BF16, False)
    entry = cache._store[(id(p), BF16, False)]
    src = weakref.ref(entry[3])
    ptr0, ver0 = p.data_ptr(), p._version
    assert entry[3].data_ptr() == ptr0 and entry[3].untyped_storage().data_ptr() == p.untyped_storage().data_ptr()
    del entry
    p.data = p.detach().clone()
    gc.collect()
    assert src() is not None and src().data_ptr() == ptr0                   # still allocated: pinned by the entry
    blocks = [torch.empty_like(p) for _ in range(64)]                       # ... so none of these can be handed its block
    assert all(b.data_ptr() != ptr0 for b in blocks)
    p.data = blocks[0].copy_(src() * 0.5)
    assert p._version == ver0 and p.data_ptr() != ptr0
    img = cache.get(p, BF16, False)
    assert torch.equal(img, (p.detach()).to(BF16)) and cache.calls == ["cast", "cast"]
    gc.collect()
    assert src() is None                                                    # the replaced entry let go of it


def test_same_dtype_untransposed_is_the_master_itself(cache):
    m = _lin()
    w = cache.get(m.weight, F32, False)
    assert w.data_ptr() == m.weight.data_ptr() and cache.calls == []
    m.weight.data.mul_(0.5)                                                  # an alias: nothing to go stale
    assert torch.equal(cache.get(m.weight, F32, False), m.weight.detach())


def test_switching_the_compute_dtype_around_a_change(cache):
    m = _lin()
    p = m.weight
    a16, a32t = cache.get(p, BF16, True), cache.get(p, F32, True)
    with torch.no_grad():
        p.mul_(0.5)
    b32t = cache.get(p, F32, True)                                           # the change is seen in fp32 mode ...
    assert b32t is not a32t and torch.equal(b32t, p.detach().t().contiguous())
    b16 = cache.get(p, BF16, True)                                           # ... and the bf16 image did not survive it
    assert b16 is not a16 and torch.equal(b16, p.detach().t().contiguous().to(BF16))
    assert cache.calls == ["transpose"] * 4


def test_entries_of_dead_parameters_are_dropped_on_the_next_miss(cache):
    m, other = _lin(), _lin()
    _warm(cache, m.weight)
    _warm(cache, other.weight)
    assert len(cache._store) == 2 * len(KINDS)
    srcs = [weakref.ref(v[3]) for k, v in cache._store.items() if k[0] == id(m.weight)]
    del m
    gc.collect()
    assert len(cache._store) == 2 * len(KINDS)                               # nothing happens on its own ...
    n = len(cache.calls)
    cache.get(other.weight, BF16, False)                                     # ... nor on a hit
    assert len(cache.calls) == n and len(cache._store) == 2 * len(KINDS)
    with torch.no_grad():
        other.weight.mul_(0.5)
    cache.get(other.weight, BF16, False)                                     # a miss sweeps
    assert len(cache._store) == len(KINDS)
    gc.collect()
    assert all(s() is None for s in srcs)


def test_a_recycled_id_does_not_inherit_the_dead_parameters_image(cache):
    m = _lin()
    img = cache.get(m.weight, BF16, False)
    key = (id(m.weight), BF16, False)
    entry = cache._store[key]
    twin = nn.Parameter(m.weight.detach() * 0.5)
    # an entry under the twin's id that matches its key in everything but the object it belongs to
    cache._store[(id(twin), BF16, False)] = ((twin.data_ptr(), twin._version, entry[0][2]), img, entry[2], entry[3])
    got = cache.get(twin, BF16, False)
    assert got is not img and torch.equal(got, twin.detach().to(BF16))


# ------------------------------------------------------------------------------ encoder_stack.packed_weights
@pytest.fixture
def packer(monkeypatch):
    """encoder_stack with the native packer replaced by a counter (the images stay uninitialised: only keys are looked at)."""
    from edgedict_amd import encoder_stack
    calls = []
    lib = types.SimpleNamespace(
        edgedict_stack_pack_weights=lambda *a: calls.append("pack") or 0,
        edgedict_stack_pack_sk=lambda *a: calls.append("sk") or 0)
    monkeypatch.setattr(encoder_stack, "_lib", types.SimpleNamespace(load=lambda: lib))
    monkeypatch.setattr(encoder_stack, "ptr", lambda t: None)
    monkeypatch.setattr(encoder_stack, "stream_ptr", lambda: None)
    monkeypatch.setattr(encoder_stack, "_PACKED", {})
    encoder_stack.calls = calls
    yield encoder_stack
    del encoder_stack.calls


def _layer(H=64, I=16):
    torch.manual_seed(1)
    return [nn.Parameter(torch.randn(4 * H, I)), nn.Parameter(torch.randn(4 * H, H)),
            nn.Parameter(torch.randn(4 * H)), nn.Parameter(torch.randn(4 * H))]


@pytest.mark.parametrize("which", [0, 1, 2, 3])
@pytest.mark.parametrize("how", ["no_grad_mul_", "data_swap", "data_swap_twice", "data_mul_then_weights_changed"])
def test_packed_layer_is_rebuilt_when_any_of_its_four_masters_changes(packer, which, how):
    import edgedict_amd
    lay = _layer()
    ent = packer.packed_weights(*lay)
    assert packer.calls == ["pack", "pack", "sk"]                            # forward images, backward images, split-K image
    assert packer.packed_weights(*lay) is ent and len(packer.calls) == 3
    p = lay[which]
    ptr0 = p.data_ptr()
    if how == "no_grad_mul_":
        with torch.no_grad():
            p.mul_(0.5)
    elif how == "data_swap":
        p.data = p.detach() * 0.5
    elif how == "data_swap_twice":
        new = p.detach() * 0.5
        p.data = p.detach().clone()
        gc.collect()
        p.data = new.clone()
        assert p.data_ptr() != ptr0                                          # the entry holds the first tensor
    else:
        p.data.mul_(0.5)
        assert packer.packed_weights(*lay) is ent                            # invisible ...
        edgedict_amd.weights_changed()                                       # ... until this
    new_ent = packer.packed_weights(*lay, backward_images=False)
    assert new_ent is not ent and packer.calls == ["pack", "pack", "sk", "pack"]
    assert new_ent.bwd_key is None
    packer.fill_backward_images(new_ent, lay[0], lay[1])                     # built lazily, under the NEW key
    assert new_ent.bwd_key == new_ent.key and packer.calls[4:] == ["pack", "sk"]
    packer.fill_backward_images(new_ent, lay[0], lay[1])
    assert len(packer.calls) == 6
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(new_ent.pinned, lay))


def test_packed_layer_entry_pins_its_sources_and_dead_layers_are_swept(packer):
    lay, other = _layer(), _layer()
    ent = packer.packed_weights(*lay)
    packer.packed_weights(*other)
    srcs = [weakref.ref(t) for t in ent.pinned]
    ptrs = [t.data_ptr() for t in ent.pinned]
    for p in lay:
        p.data = p.detach().clone()
    gc.collect()
    assert all(s() is not None and s().data_ptr() == a for s, a in zip(srcs, ptrs))
    del ent, lay
    gc.collect()
    assert len(packer._PACKED) == 2
    with torch.no_grad():
        other[2].mul_(0.5)
    packer.packed_weights(*other)                                            # a miss sweeps the dead layer's entry
    assert len(packer._PACKED) == 1
    gc.collect()
    assert all(s() is None for s in srcs)


def test_weights_changed_is_exported_and_documented():
    import os
    import edgedict_amd
    assert callable(edgedict_amd.weights_changed)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "INTEGRATION.md")) as f:
        assert "edgedict_amd.weights_changed()" in f.read()
