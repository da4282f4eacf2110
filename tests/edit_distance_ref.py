"""Host oracle of the batched edit distance (csrc/edit_distance.hip, ``metrics.edit_distance``): the counts
``(dist, sub, del, ins)`` of turning a reference ``r`` into a hypothesis ``h`` - ``dist`` the Levenshtein distance and,
of all alignments of that distance, the one with the FEWEST insertions (hence the fewest deletions and the most
substitutions, since ``ins - del = len(h) - len(r)``).  An insertion is a hypothesis element without a reference
element, a deletion a reference element without a hypothesis element; elements are compared with ``==`` only.

``counts``        pure Python: a DP over ``(dist, ins)`` tuples with lexicographic ``min``, written from the definition -
                  no packing constant.
``counts_fast``   numpy, one row at a time (``np.minimum.accumulate`` resolves the deletion chain): for length 1023.
``enumerate_all`` the recursive enumeration of every alignment: what test_edit_distance_host.py pins the two on.
"""
import numpy as np


def _finish(dist, ins, H, R):
    dele = ins - (H - R)
    return (int(dist), int(dist - ins - dele), int(dele), int(ins))


def counts(h, r):
    h, r = [int(x) for x in h], [int(x) for x in r]
    H, R = len(h), len(r)
    prev = [(j, 0) for j in range(R + 1)]            # d(0, j): j deletions
    for i in range(1, H + 1):
        cur = [(i, i)]                               # d(i, 0): i insertions
        for j in range(1, R + 1):
            hit = h[i - 1] == r[j - 1]
            diag = prev[j - 1] if hit else (prev[j - 1][0] + 1, prev[j - 1][1])
            up = (prev[j][0] + 1, prev[j][1] + 1)    # insertion of h[i-1]
            left = (cur[j - 1][0] + 1, cur[j - 1][1])  # deletion of r[j-1]
            cur.append(min(diag, up, left))
        prev = cur
    return _finish(prev[R][0], prev[R][1], H, R)


def counts_fast(h, r):
    """The row form on one int64 key ``dist * BIG + ins`` (``BIG`` above any insertion count, so the key orders
    lexicographically): t[j] = min(up, diag) for j >= 1, then d[j] = j BIG + prefix-min(t[k] - k BIG)."""
    h = np.asarray(h, dtype=np.int64).reshape(-1)
    r = np.asarray(r, dtype=np.int64).reshape(-1)
    H, R = h.size, r.size
    BIG = np.int64(1 << 20)
    cols = np.arange(R + 1, dtype=np.int64) * BIG
    d = cols.copy()
    for i in range(1, H + 1):
        t = np.empty(R + 1, dtype=np.int64)
        t[0] = i * (BIG + 1)
        t[1:] = np.minimum(d[1:] + BIG + 1, d[:-1] + np.where(r == h[i - 1], 0, BIG))
        d = cols + np.minimum.accumulate(t - cols)
    return _finish(d[R] // BIG, d[R] % BIG, H, R)


def enumerate_all(h, r):
    """Every alignment of h against r, minimising (dist, ins) lexicographically."""
    h, r = [int(x) for x in h], [int(x) for x in r]
    H, R = len(h), len(r)
    best = [None]

    def walk(i, j, dist, ins):
        if i == H and j == R:
            if best[0] is None or (dist, ins) < best[0]:
                best[0] = (dist, ins)
            return
        if i < H and j < R:
            walk(i + 1, j + 1, dist + (h[i] != r[j]), ins)
        if i < H:
            walk(i + 1, j, dist + 1, ins + 1)
        if j < R:
            walk(i, j + 1, dist + 1, ins)

    walk(0, 0, 0, 0)
    return _finish(best[0][0], best[0][1], H, R)


def counts_nbest(hyps, hyp_lens, n_hyp, refs, ref_lens):
    """The kernel's contract on padded arrays: int32 [B, N, 4], -1 in the slots n >= n_hyp[b] (None: all live);
    lengths clamped into [0, U]."""
    hyps, refs = np.asarray(hyps), np.asarray(refs)
    hyp_lens, ref_lens = np.asarray(hyp_lens), np.asarray(ref_lens)
    B, N = hyp_lens.shape
    Uh = hyps.shape[2] if hyps.ndim == 3 else 0
    Ur = refs.shape[1] if refs.ndim == 2 else 0
    out = np.full((B, N, 4), -1, dtype=np.int32)
    for b in range(B):
        R = int(np.clip(ref_lens[b], 0, Ur))
        live = N if n_hyp is None else int(np.clip(n_hyp[b], 0, N))
        for n in range(live):
            H = int(np.clip(hyp_lens[b, n], 0, Uh))
            out[b, n] = counts_fast(hyps[b, n, :H] if H else [], refs[b, :R] if R else [])
    return out


def totals(rows, ref_lens):
    """What ``metrics.ErrorRate`` accumulates: rows of (dist, sub, del, ins) with the reference length of each."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 4)
    ref_lens = np.asarray(ref_lens, dtype=np.int64).reshape(-1)
    return dict(errors=int(rows[:, 0].sum()), substitutions=int(rows[:, 1].sum()), deletions=int(rows[:, 2].sum()),
                insertions=int(rows[:, 3].sum()), ref_len=int(ref_lens.sum()), sequences=int(rows.shape[0]),
                wrong_sequences=int((rows[:, 0] > 0).sum()))
