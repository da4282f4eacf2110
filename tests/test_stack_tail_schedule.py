"""CPU: what the encoder stack's backward pass enqueues around its last BPTT launches (EDGEDICT_STACK_TAIL,
csrc/encoder_stack.hip), read off the scheduler's dry run (``edgedict_stack_schedule_events``: every enqueued piece of
work as (kind, layer, arg, stream), in enqueue order - the dry run is serial, so "enqueued after" is a position).

Checked at the E6D2 geometry and at a 3-layer geometry with one time reduction, for the default setting against
EDGEDICT_STACK_TAIL=0 (the order before the switch existed):
  * every layer's LayerNorm parameter sum is enqueued after that layer's last LayerNorm-backward chunk (on a stream of the
    same kind) and before the end of the pass - exactly one sum per layer;
  * ``grads_final`` fires once per layer, in the same layer order as with =0, after all of that layer's gradient work
    (both products, the bias gradient) has been enqueued;
  * every consumer is enqueued after its producer: a layer's weight-gradient work after the launch that carries its frame
    0, the layer-0 dX product after the last launch and the input norm's gradient after that product, on its stream;
  * the same work is enqueued (same multiset of events, same launch count, same step -> launch map)."""
import os
from collections import Counter

import pytest

from edgedict_amd import encoder_stack as es

E = es

GEOMETRIES = {
    "e6d2": dict(T0=401, I0=240, H=1024, reductions=[1, 2, 1, 1, 1, 1], B=64, chunk=16),
    "l3": dict(T0=37, I0=40, H=64, reductions=[1, 2, 1], B=3, chunk=4),
}
FLAGS = {"plain": 0, "dw_at_end": es.DW_AT_END, "serial": es.SERIAL}


def _dry(geo, tail, flags=0, sk=True):
    """(events, grads_final order, step_launch, n_launches) of one dry run under EDGEDICT_STACK_TAIL = tail."""
    old_env = os.environ.get("EDGEDICT_STACK_BWD_SK")
    os.environ["EDGEDICT_STACK_BWD_SK"] = "1" if sk else "0"
    es.tail_mode(tail)
    try:
        order = []
        ev = es.schedule_events(flags=flags, grads_final=order.append, **geo)
        order2 = []
        steps, _enq, n, _slots = es.schedule(backward=True, flags=flags, grads_final=order2.append, **geo)
        assert order == order2
        return ev, order, steps, n
    finally:
        es.tail_mode(-1)
        if old_env is None:
            os.environ.pop("EDGEDICT_STACK_BWD_SK", None)
        else:
            os.environ["EDGEDICT_STACK_BWD_SK"] = old_env


def _positions(ev, kind, layer=None):
    return [i for i, e in enumerate(ev) if e[0] == kind and (layer is None or e[1] == layer)]


@pytest.mark.parametrize("sk", [True, False], ids=["split_k", "launch_per_step"])
@pytest.mark.parametrize("flags", sorted(FLAGS))
@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
def test_tail_schedule(geo, flags, sk):
    g = GEOMETRIES[geo]
    L = len(g["reductions"])
    default = es.tail_mode()
    ev0, order0, steps0, n0 = _dry(g, 0, FLAGS[flags], sk)
    ev1, order1, steps1, n1 = _dry(g, default, FLAGS[flags], sk)

    for ev, order, steps, n in ((ev0, order0, steps0, n0), (ev1, order1, steps1, n1)):
        end = _positions(ev, E.EV_END)
        assert end == [len(ev) - 1], "the end of the pass is the last event"
        launches = _positions(ev, E.EV_LAUNCH)
        assert [ev[i][2] for i in launches] == list(range(n)), "launch events carry their index, in order"
        for l in range(L):
            # LayerNorm sum: once, after the layer's last LayerNorm-backward chunk, before the end
            sums = _positions(ev, E.EV_LN_SUM, l)
            chunks = _positions(ev, E.EV_LN_BWD, l)
            assert len(sums) == 1 and len(chunks) >= 1, (l, sums, len(chunks))
            assert sorted(ev[i][2] for i in chunks) == list(range(len(chunks))), "every chunk's partial rows are written once"
            assert chunks[-1] < sums[0] < end[0], (l, chunks[-1], sums[0])
            assert ev[sums[0]][3] == E.EVS_SIDE and ev[chunks[-1]][3] == E.EVS_SIDE
            # the layer's weight-gradient work: after the launch that carries its frame 0 (its BPTT is complete) ...
            carried = launches[int(steps[l][0])]
            work = [i for i, e in enumerate(ev) if e[1] == l and e[0] in (E.EV_DW, E.EV_BIAS)]
            assert sorted((ev[i][0], ev[i][2]) for i in work) == [(E.EV_DW, 0), (E.EV_DW, 1), (E.EV_BIAS, 0)], (l, work)
            assert min(work) > carried, (l, min(work), carried)
            # ... and grads_final once, after all of it
            final = _positions(ev, E.EV_GRADS_FINAL, l)
            assert len(final) == 1 and final[0] > max(work), (l, final, work)
        # the input norm's gradient: dX of layer 0 after the last launch, the column sums after it on the same stream
        dx0, inorm = _positions(ev, E.EV_DX0), _positions(ev, E.EV_IN_NORM)
        assert len(dx0) == 1 and len(inorm) == 1
        assert launches[-1] < dx0[0] < inorm[0] < end[0]
        assert ev[dx0[0]][3] == ev[inorm[0]][3]
        assert order == [ev[i][1] for i in _positions(ev, E.EV_GRADS_FINAL)], "the callback fires where the event says"

    # against the order before the switch: same callbacks in the same order, same work, same launches
    assert order1 == order0 and len(order1) == L
    assert n1 == n0
    assert all((a == b).all() for a, b in zip(steps0, steps1))
    assert Counter(e[:3] for e in ev0) == Counter(e[:3] for e in ev1), "the same work is enqueued, only elsewhere"


@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
def test_bias_column_sums_of_the_last_two_layers_run_beside_their_products(geo):
    """Switch on: the bias gradients of layers 1 and 0 go to the side stream, ahead of the layer's products (so that the
    bandwidth-bound sum starts first); every other layer's stays behind its products on the weight-gradient stream."""
    g = GEOMETRIES[geo]
    L = len(g["reductions"])
    ev, _order, _steps, _n = _dry(g, 1)
    for l in range(L):
        bias = _positions(ev, E.EV_BIAS, l)[0]
        prods = _positions(ev, E.EV_DW, l)
        if l <= 1:
            assert ev[bias][3] == E.EVS_SIDE and bias < min(prods), l
        else:
            assert ev[bias][3] == E.EVS_W and bias > max(prods), l
    ev0, _order, _steps, _n = _dry(g, 0)
    assert all(e[3] == E.EVS_W for e in ev0 if e[0] == E.EV_BIAS)


@pytest.mark.parametrize("env", [("EDGEDICT_STACK_DW_SEG", "1"), ("EDGEDICT_STACK_DW_SEG", "2"),
                                 ("EDGEDICT_STACK_TAIL_SPLIT", "2")], ids=["dw_seg1", "dw_seg2", "tail_split2"])
@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
def test_a_layer_issued_in_segments_keeps_its_bias_updates_on_one_stream(geo, env, monkeypatch):
    """EDGEDICT_STACK_DW_SEG / EDGEDICT_STACK_TAIL_SPLIT: a layer's weight gradients are issued in several calls, the first of which stores the
    gradient and the later ones add to it.  Those updates of one buffer must stay on ONE stream, in order: with the
    switch on no bias gradient of such a layer may move to the side stream (only a layer issued in a single call does),
    and the events are those of =0 exactly."""
    monkeypatch.setenv(*env)
    g = GEOMETRIES[geo]
    L = len(g["reductions"])
    ev0, order0, _steps, n0 = _dry(g, 0)
    ev1, order1, _steps, n1 = _dry(g, 1)
    split = 0
    for l in range(L):
        bias = _positions(ev1, E.EV_BIAS, l)
        streams = {ev1[i][3] for i in bias}
        assert len(streams) == 1, (l, streams)
        if len(bias) > 1:
            split += 1
            assert streams == {E.EVS_W}, (l, streams)
    assert split >= 2, "the geometry splits the two layers that finish last"
    for l in range(min(L, 2)):
        assert len(_positions(ev1, E.EV_BIAS, l)) > 1, l
    assert ev1 == ev0 and order1 == order0 and n1 == n0


def test_e6d2_launch_count_is_the_benched_one():
    ev, order, _steps, n = _dry(GEOMETRIES["e6d2"], es.tail_mode(), 0, True)
    assert n == 36 and order == [5, 4, 3, 2, 1, 0]


def test_tail_mode_overrides_and_restores_the_environment_setting():
    base = es.tail_mode()
    try:
        assert es.tail_mode(0) == 0
        assert es.tail_mode() == 0
        assert es.tail_mode(1) == 1 and es.tail_mode(8) == 1          # on / off: any non-zero value is "on"
    finally:
        assert es.tail_mode(-1) == base
