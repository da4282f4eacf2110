"""Shapes shared by test_rnnt_walks_gpu.py and test_rnnt_align_gpu.py (test-local code): which instantiation of the
lattice walk rnnt_alpha_beta<C, VIT> (csrc/rnnt_loss.hip) a label axis reaches, and one batch of utterance lengths that
puts every edge of that instantiation - the prefetch ring of D steps, the lane that owns the last live column, the
beta side's columns counted from the right - into one launch."""
import numpy as np

T_WALK = 17             # frames: T_b can sit at D - 1, D, D + 1 and 2 D + 1 for every ring depth D <= 8
B_WALK = 8              # rows of length_rows
# both sides of every dispatch boundary, and the limit
U1_WALK = [64, 65, 128, 129, 256, 257, 512, 513, 1024]


def variant(U1):
    """(C, D) of the walk the dispatcher picks for U1 = U + 1 label columns: C = ceil(U1 / 64) columns per lane rounded
    up to a power of two, D = the depth of that instantiation's prefetch ring."""
    assert 1 <= U1 <= 1024
    cols = (U1 + 63) // 64
    C = 1
    while C < cols:
        C *= 2
    D = 8 if C <= 2 else (4 if C <= 4 else (2 if C <= 8 else 1))
    return C, D


def length_rows(T, U1, rotate=0):
    """(act_lens, label_lens) int32 [8]: the (T_b, U_b) boxes of one batch, row 0 (the full box) moved to row
    ``rotate``."""
    C, D = variant(U1)
    assert T >= 2 * D + 1 and U1 >= 4
    # the largest U_b < U1 - 1 whose last live lane owns more than one and fewer than C columns: there the beta side's
    # columns counted from the right run below 0 in that lane.  C <= 2 has no such width: any U_b not used elsewhere.
    k = next((k for k in range(U1 - 2, -1, -1) if (k + 1) % C not in (0, 1)), U1 - 3)
    rows = [
        (T, U1 - 1),                    # the full box
        (1, U1 - 1),                    # one frame carries every label
        (T, 0),                         # no labels: lane 0 alone, one column
        (D + 1, C - 1),                 # a single live lane, full
        (D, C),                         # a second lane with one column
        (max(1, D - 1), U1 - 2),        # fewer frames than the ring is deep
        (2 * D + 1, k),
        (T - 1, (U1 - 1) // 2),
    ]
    rows = rows[-rotate:] + rows[:-rotate] if rotate else rows
    al = np.array([r[0] for r in rows], np.int32)
    ll = np.array([r[1] for r in rows], np.int32)
    assert al.max() == T and ll.max() == U1 - 1 and (al >= 1).all() and (ll >= 0).all()
    return al, ll
