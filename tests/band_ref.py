"""Restatement of the band-packed lattice's row layout (test-local code, shared by test_band_host.py and
test_band_gpu.py).  Only the live cells of a band table (arloss_ref.band_table: band[b, t] = (ulo, uhi), (0, -1) for a
frame without a live cell) exist as rows:

    row(b, t, u) = row_off[b, t] + (u - ulo[b, t]),     ulo[b, t] <= u <= uhi[b, t]

row_off = the exclusive prefix sum of the widths max(0, uhi - ulo + 1) in (b, t) order."""
import numpy as np
import torch


def band_offsets(band):
    """(row_off int64 [B, T], rows) of a band table [B, T, 2]."""
    band = np.asarray(band, dtype=np.int64)
    width = np.maximum(0, band[:, :, 1] - band[:, :, 0] + 1)
    flat = width.reshape(-1)
    off = np.concatenate([[0], np.cumsum(flat)[:-1]]) if flat.size else flat
    return off.reshape(width.shape).astype(np.int64), int(flat.sum())


def band_cells(band):
    """(b, t, u) int64 arrays of every band row, in row order."""
    band = np.asarray(band, dtype=np.int64)
    bs, ts, us = [], [], []
    for b in range(band.shape[0]):
        for t in range(band.shape[1]):
            lo, hi = band[b, t]
            for u in range(lo, hi + 1):
                bs.append(b)
                ts.append(t)
                us.append(u)
    return np.array(bs, dtype=np.int64), np.array(ts, dtype=np.int64), np.array(us, dtype=np.int64)


def band_row_tu(band):
    """t << 16 | u of every band row."""
    _, t, u = band_cells(band)
    return (t << 16) | u


def band_pack(x, band):
    """dense [B, T, U1, ...] (tensor or array) -> [rows, ...]: the live cells in row order."""
    b, t, u = band_cells(band)
    if torch.is_tensor(x):
        return x[torch.as_tensor(b), torch.as_tensor(t), torch.as_tensor(u)]
    return np.asarray(x)[b, t, u]


def band_unpack(y, band, fill, U1=None):
    """[rows, ...] -> dense [B, T, U1, ...] with ``fill`` on the dead cells (U1 defaults to the last live column + 1)."""
    band = np.asarray(band, dtype=np.int64)
    b, t, u = band_cells(band)
    assert y.shape[0] == len(b), (y.shape, len(b))
    U1 = int(band[:, :, 1].max()) + 1 if U1 is None else U1
    shape = (band.shape[0], band.shape[1], U1) + tuple(y.shape[1:])
    if torch.is_tensor(y):
        out = y.new_full(shape, fill)
        out[torch.as_tensor(b), torch.as_tensor(t), torch.as_tensor(u)] = y
        return out
    out = np.full(shape, fill, dtype=np.asarray(y).dtype)
    out[b, t, u] = y
    return out
