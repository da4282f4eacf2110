"""CPU: the numpy restatement of the dropout mask (tests/dropout_ref.py) pinned so that it can serve as the oracle of
tests/test_dropout_gpu.py and of the dropout case of tests/test_stack_kernels_gpu.py - literal hash, mask and seed
values, the statistics a mask must have (keep rate, independence between the seeds of consecutive calls, no structure
along the rows or columns of a [B T, H] view), and the argument errors of ``edgedict_dropout`` raised before any
launch."""
import ctypes
import itertools

import numpy as np
import pytest

import dropout_ref as D


def _bits(b):
    return "".join(str(int(v)) for v in b)


def test_hash_keep_and_seed_literals():
    assert [int(v) for v in D.hash32([0, 1, 2, 0xFFFFFFFF])] == [0x0, 0x688990c0, 0xd1132181, 0x6768824a]
    assert _bits(D.keep(1234, np.arange(32), 0.5)) == "00001010101101100111000010111000"
    assert _bits(D.keep(0x85EBCA6B, np.arange(32), 0.1)) == "10111101111111111101111111111110"
    assert D.seeds(3, 1, 3) == [0x6092377e, 0xe67e01e9, 0x6c69cc54]
    assert _bits(D.mask((4, 8), 0.5, 1234).ravel()) == "00001010101101100111000010111000"


def test_seeds_restate_next_dropout_seed():
    import torch
    from edgedict_amd import models
    old, state = models._dropout_calls[0], torch.random.get_rng_state()
    try:
        for s, first in ((3, 1), (0, 1), (2 ** 40 + 17, 5)):
            torch.manual_seed(s)
            models._dropout_calls[0] = first - 1
            got = [models._next_dropout_seed() for _ in range(4)]
            assert got == D.seeds(s, first, 4) and models._dropout_calls[0] == first + 3
    finally:
        models._dropout_calls[0] = old
        torch.random.set_rng_state(state)


def test_threshold_and_scale_are_the_float32_ones():
    assert int(D.thresh(0.0)) == 0 and int(D.thresh(0.5)) == 2 ** 31
    assert int(D.thresh(0.1)) == int(np.floor(float(np.float32(0.1)) * 2.0 ** 32)) == 429496736
    assert D.scale(0.5) == np.float32(2) and D.scale(0.0) == np.float32(1)
    assert D.scale(0.1).dtype == np.float32 and D.scale(0.1) == np.float32(1) / np.float32(0.9)


def test_high_word_of_the_index_enters_the_hash():
    """i >> 32 is added to lo(i) * 0x9e3779b9 before the inner hash: no device test reaches it (2^32 elements)."""
    lo = np.arange(64, dtype=np.uint64)
    a, b = D.keep(7, lo, 0.5), D.keep(7, lo + (np.uint64(1) << np.uint64(32)), 0.5)
    assert (a != b).any()
    want = D.hash32(np.uint64(7) ^ D.hash32((lo * np.uint64(0x9e3779b9) + np.uint64(1)) & D.M32)) >= D.thresh(0.5)
    assert (b == want).all()
    assert (D.mask((64,), 0.5, 7, first=2 ** 32) == b).all()


@pytest.mark.parametrize("n", [4096, 65536, 2 ** 20])
def test_keep_rate_is_one_minus_p(n):
    idx = np.arange(n, dtype=np.uint64)
    for p, seed in itertools.product((0.1, 0.3, 0.4, 0.5, 0.9), (0, 1, 1234, 0xFFFFFFFF, 0x85EBCA6B)):
        rate = D.keep(seed, idx, p).mean()
        assert abs(rate - (1 - p)) <= 4 * np.sqrt(p * (1 - p) / n), (p, seed, n, rate)


def test_masks_of_consecutive_calls_are_pairwise_independent():
    n, p = 2 ** 18, 0.3
    masks = [D.mask((n,), p, s) for s in D.seeds(3, 1, 4)]
    for a, b in itertools.combinations(masks, 2):
        agree = (a == b).mean()
        assert abs(agree - 0.58) <= 4 * np.sqrt(0.58 * 0.42 / n), agree


def test_p_zero_keeps_everything_and_rows_and_columns_have_no_structure():
    for seed in (0, 1234, 0xFFFFFFFF):
        assert D.mask((3, 1000), 0.0, seed).all()
    m = D.mask((4160, 512), 0.1, 1234)
    rows, cols = m.mean(1), m.mean(0)
    assert 0.85 <= rows.min() and rows.max() <= 0.95, (rows.min(), rows.max())
    assert 0.88 <= cols.min() and cols.max() <= 0.92, (cols.min(), cols.max())


def test_native_argument_errors_are_status_codes(hip_lib):
    """edgedict_dropout validates before it touches the device: the pointers below are never dereferenced."""
    fake = ctypes.c_void_p(256)
    ll, f, u = ctypes.c_longlong, ctypes.c_float, ctypes.c_uint
    drop = hip_lib.edgedict_dropout
    for p in (1.0, 1.5, -0.1, float("nan")):
        assert drop(0, fake, fake, ll(8), f(p), u(1), None) == -1, p
        assert b"p must be" in hip_lib.edgedict_last_error()
    assert drop(7, fake, fake, ll(8), f(0.5), u(1), None) == -1
    assert b"dtype" in hip_lib.edgedict_last_error()
    assert drop(0, fake, fake, ll(-1), f(0.5), u(1), None) == -1
    assert b"size" in hip_lib.edgedict_last_error()
    assert drop(0, None, fake, ll(8), f(0.5), u(1), None) == -1
    assert b"null" in hip_lib.edgedict_last_error()
    assert drop(0, None, None, ll(0), f(0.5), u(1), None) == 0         # nothing to do: nothing to launch
    assert drop(1, None, None, ll(0), f(0.0), u(0), None) == 0
