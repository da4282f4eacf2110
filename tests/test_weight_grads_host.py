"""CPU: side.WeightGrads decides, without a device, which weight parameters of an autograd Function get a gradient and
whether their products accumulate into the existing .grad buffers on the auxiliary stream or are returned to autograd."""
import types

import torch

from edgedict_amd import config, side


def _p(grad="f32"):
    """A parameter stand-in: only its .grad is looked at."""
    g = {"f32": lambda: torch.zeros(4, 3), "bf16": lambda: torch.zeros(4, 3, dtype=torch.bfloat16),
         "strided": lambda: torch.zeros(3, 4).t(), None: lambda: None}[grad]()
    return types.SimpleNamespace(grad=g)


def _wg(needs, params, first=0):
    return side.WeightGrads(types.SimpleNamespace(needs_input_grad=needs), first, params)


def test_every_live_parameter_in_place_defers():
    ps = (_p(), _p(), _p())
    wg = _wg((True, True, True), ps)
    assert wg.defer and wg.live == ps and wg.need == [True, True, True]
    assert wg.grads == [None, None, None]


def test_one_live_parameter_not_in_place_returns_them_all():
    for odd in (None, "bf16", "strided"):
        ps = (_p(), _p(odd), _p())
        wg = _wg((True, True, True), ps)
        assert not wg.defer and wg.live == ps, odd


def test_frozen_and_absent_parameters_are_not_live_and_do_not_decide():
    w, frozen = _p(), _p(None)
    wg = _wg((True, True, False, True), (w, frozen, None), first=1)    # needs_input_grad[0] is the Function's input
    assert wg.need == [True, False, False] and wg.live == (w,) and wg.defer
    wg = _wg((False, True), (_p(), None))                                # bias absent, weight frozen
    assert wg.live == () and not wg.defer


def test_nothing_live_is_a_no_op():
    wg = _wg((False, False), (_p(), _p()))
    with wg:
        wg.gemm(0, None, None)
        wg.colsum(1, None)
    assert wg.grads == [None, None]


def test_switch_off_returns_everything(monkeypatch):
    monkeypatch.setattr(config, "DEFER_WEIGHT_GRADS", False)
    wg = _wg((True, True), (_p(), _p()))
    assert not wg.defer and len(wg.live) == 2


def test_accumulates_in_place():
    assert side.accumulates_in_place(_p())
    for odd in (None, "bf16", "strided"):
        assert not side.accumulates_in_place(_p(odd)), odd
