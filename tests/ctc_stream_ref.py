"""What the streaming CTC prefix beam search's tests share (csrc/ctc_decode.hip ``edgedict_ctc_stream_*``,
decode.StreamingCTCBeamSearch): the chunkings, the token tree a compaction leaves, and the compaction cases with the
capacities chosen for them (tests/test_ctc_stream_host.py verifies on the CPU, with the float64 oracle of
tests/ctc_beam_ref.py, that every case fits its capacity and would not fit without compaction)."""
import numpy as np


def chunking(kind, T):
    """The chunk lengths of ``T`` frames: ``ones``; ``357`` = 3, 5, 7 repeating (no multiple of the request ring's depth
    4); ``whole``; ``fours`` = 4, 4, ... and the remainder."""
    if kind == "ones":
        return [1] * T
    if kind == "whole":
        return [T]
    out, t, k = [], 0, 0
    while t < T:
        n = min((3, 5, 7)[k % 3] if kind == "357" else 4, T - t)
        out.append(n)
        t += n
        k += 1
    return out


CHUNKINGS = ("ones", "357", "whole", "fours")


def tree_after(paths):
    """``paths``: per hypothesis of a beam the list of (token, frame) from the root - a node of the token tree IS such a
    path, since a prefix creates a given token at most once per frame.  Returns ``(live, committed)``: the nodes the
    compaction keeps (the lowest common ancestor as the root, and every node between it and a hypothesis) and the tokens
    above and including that ancestor, which it commits."""
    paths = [tuple(p) for p in paths]
    k = 0
    while all(len(p) > k for p in paths) and len({p[k] for p in paths}) == 1:
        k += 1
    nodes = {p[:j] for p in paths for j in range(k + 1, len(p) + 1)}
    return 1 + len(nodes), k


# compaction cases: (shape of ctc_beam_ref.SHAPES, frames per advance, node_capacity).  W = 1: every advance commits the
# whole hypothesis, one node stays, NC = W + 3 W.  W = 10 on random logits keeps up to 164 nodes alive (ten hypotheses
# that share little), so NC = 200 there: above 164 + 3 W, far below the 417 nodes the utterance creates.
COMPACTION = [((5, 8, 1, 7), 3, 4), ((47, 32, 10, 16), 3, 200)]


def capacity_trace(z, W, cand, step, search_one):
    """Per advance of ``step`` frames over ``z``: ``(live nodes before, frames taken)`` by the oracle ``search_one``."""
    T = z.shape[0]
    out, t, live = [], 0, 1
    while t < T:
        n = min(step, T - t)
        out.append((live, n))
        t += n
        hyps = search_one(z[:t], W, cand)[0]
        live = tree_after([list(zip(h.tokens, h.frames)) for h in hyps])[0]
    return out, live
