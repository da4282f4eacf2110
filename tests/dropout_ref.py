"""Host restatement of the counter-based dropout mask (csrc/common.hpp: ed_drop_hash / ed_drop_keep / ed_drop_thresh)
and of the seed schedule of the autograd glue (models._next_dropout_seed), in numpy: uint32 arithmetic carried in
uint64 and masked after every step.  The mask is a stateless function of (seed, contiguous element index), so every
dropout path of the product can be compared with a float64 reference UNDER THE IDENTICAL MASK.

Pinned on the host by tests/test_dropout_ref_host.py and against the device by tests/test_dropout_gpu.py."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)


def _u64(x):
    return np.asarray(x, dtype=np.uint64) & M32


def hash32(x):
    """ed_drop_hash: x ^= x>>16; x *= 0x7feb352d; x ^= x>>15; x *= 0x846ca68b; x ^= x>>16 (mod 2^32)."""
    x = _u64(x)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & M32
    x = x ^ (x >> np.uint64(16))
    return x


def thresh(p):
    """ed_drop_thresh: floor(float32(p) * 2^32) (the product is exact in float64)."""
    return np.uint64(int(float(np.float32(p)) * 4294967296.0))


def keep(seed, idx, p):
    """ed_drop_keep on element indices ``idx`` (any non-negative integers below 2^63): a bool array."""
    idx = np.asarray(idx, dtype=np.uint64)
    lo, hi = idx & M32, idx >> np.uint64(32)
    inner = hash32((lo * np.uint64(0x9e3779b9) + hi) & M32)
    return hash32((np.uint64(int(seed) & 0xFFFFFFFF) ^ inner) & M32) >= thresh(p)


def mask(shape, p, seed, first=0):
    """The keep mask of a contiguous tensor of ``shape`` (element ``i`` of its memory order has index first + i)."""
    n = int(np.prod(shape, dtype=np.int64))
    return keep(seed, np.arange(first, first + n, dtype=np.uint64), p).reshape(shape)


def scale(p):
    """The kernels' 1.f / (1.f - p) in float32."""
    return np.float32(1) / (np.float32(1) - np.float32(p))


def seeds(initial_seed, first_call, n):
    """models._next_dropout_seed for the calls first_call .. first_call + n - 1 (the counter AFTER its increment) under
    torch.initial_seed() == initial_seed."""
    return [(int(initial_seed) * 0x9E3779B1 + c * 0x85EBCA6B) & 0xFFFFFFFF for c in range(first_call, first_call + n)]
