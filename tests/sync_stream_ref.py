"""ORACLE (test infrastructure only): the streaming form of the frame-synchronous beam search (csrc/decode_sync.hip,
``edgedict_sync_stream_*``; decode.StreamingSyncBeamSearch) restated in Python floats: ``sync_beam_ref.search_core``'s
steps 1-5 driven chunk by chunk, with the engine's token tree made explicit so that the commit rule can be stated
exactly.

Node identities mirror the engine's: a kept token child that survives the folding gets a NEW node (parent = its
parent hypothesis' node, the token, the frame counted from the stream's start, lp); a blank child keeps its parent's
node; a folded pair keeps the blank child's node (the older one), so the token child's node is never created.  The same
token sequence can therefore live in two node chains: when it is pruned and later created again, the second creation
gets fresh nodes.

After each chunk the tree is compacted: the path from the root to the lowest common ancestor of the live hypotheses'
leaves (the root itself if any hypothesis sits on it) is appended to the committed log, the ancestor becomes the root and
only nodes a live leaf reaches are kept.  ``beam()`` ranks as step 6 does and returns whole hypotheses, committed log
first; between chunks the beam itself stays in beam order."""
import math


class _Row:
    __slots__ = ("seq", "logp", "tok", "state", "node")

    def __init__(self, seq, logp, tok, state, node):
        self.seq, self.logp, self.tok, self.state, self.node = seq, logp, tok, state, node


class StreamSearch:
    """One stream.  ``expand(t, tok, state) -> (lp, state after tok)`` as in ``search_core``; ``t`` counts from the
    stream's start."""

    def __init__(self, W, expand, root_state, root_tok, blank=0):
        self.W, self.expand, self.blank = W, expand, blank
        self.rows = [_Row((), 0.0, root_tok, root_state, -1)]
        self.tree = {}              # id -> (parent id or -1, token, frame, lp)
        self.next_id = 0
        self.frames_done = 0
        self.log = []               # committed (token, frame, lp)
        self.margin = float("inf")
        self.merges = 0

    def _frame(self, t):
        W, blank = self.W, self.blank
        cands, steps = [], []
        for i, h in enumerate(self.rows):
            lp, new_state = self.expand(t, h.tok, h.state)
            steps.append((lp, new_state))
            cands.extend((h.logp + float(lp[k]), i, k) for k in range(len(lp)))
        cands.sort(key=lambda c: (-c[0], c[1], c[2]))
        if len(cands) > W:
            self.margin = min(self.margin, cands[W - 1][0] - cands[W][0])
        new, place = [], {}
        for score, i, k in cands[:W]:
            h = self.rows[i]
            if k == blank:
                child = _Row(h.seq, score, h.tok, h.state, h.node)
            else:           # node: ("new", parent node, token, lp) until the folding is over
                child = _Row(h.seq + (k,), score, k, steps[i][1], ("new", h.node, k, float(steps[i][0][k])))
            j = place.get(child.seq)
            if j is None:
                place[child.seq] = len(new)
                new.append(child)
                continue
            self.merges += 1
            old = new[j]
            mx, mn = max(old.logp, child.logp), min(old.logp, child.logp)
            keep = child if k == blank else old
            new[j] = _Row(keep.seq, mx + math.log1p(math.exp(mn - mx)), keep.tok, keep.state, keep.node)
        for h in new:               # the surviving token children get their nodes, in beam order
            if isinstance(h.node, tuple):
                _, parent, k, lp = h.node
                self.tree[self.next_id] = (parent, k, t, lp)
                h.node = self.next_id
                self.next_id += 1
        self.rows = new

    def _path(self, node):
        path = []
        while node != -1:
            path.append(node)
            node = self.tree[node][0]
        return path[::-1]

    def advance(self, n_frames):
        """``n_frames`` more frames, then the compaction.  Returns the (token, frame, lp) triples this chunk committed."""
        for t in range(self.frames_done, self.frames_done + n_frames):
            self._frame(t)
        self.frames_done += n_frames
        paths = [self._path(h.node) for h in self.rows]
        common = 0
        while all(len(p) > common for p in paths) and len({p[common] for p in paths}) == 1:
            common += 1
        done = [self.tree[nd][1:] for nd in paths[0][:common]]
        self.log.extend(done)
        lca = paths[0][common - 1] if common else -1
        keep = {}
        for p in paths:
            for nd in p[common:]:
                parent, k, f, lp = self.tree[nd]
                keep[nd] = (-1 if parent == lca else parent, k, f, lp)
        self.tree = keep
        for h in self.rows:
            if h.node == lca:
                h.node = -1
        return done

    def live_nodes(self):
        return len(self.tree)

    def committed(self):
        return [k for k, _, _ in self.log]

    def beam(self):
        """The ranked beam in ``search_core``'s output form, every hypothesis the committed log followed by its tail."""
        order = sorted(range(len(self.rows)), key=lambda j: -self.rows[j].logp)
        out = []
        for j in order:
            h = self.rows[j]
            full = self.log + [self.tree[nd][1:] for nd in self._path(h.node)]
            assert tuple(k for k, _, _ in full) == h.seq, (full, h.seq)
            out.append(dict(tokens=[k for k, _, _ in full], frames=[f for _, f, _ in full],
                            token_logp=[lp for _, _, lp in full], logp=h.logp))
        return out


def common_token_prefix(beam):
    """Length of the longest common prefix of the beam's token sequences."""
    seqs = [h["tokens"] for h in beam]
    n = 0
    while all(len(s) > n for s in seqs) and len({s[n] for s in seqs}) == 1:
        n += 1
    return n
