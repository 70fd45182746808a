"""The conv kernels' division by launch constants (csrc/conv_common.h fast_div: multiply-high + shift, divisor 1 a case of its own), checked on the host
through havc_conv_fast_div, which runs the SAME inline function the kernels run.

The pixel index math of conv_pipe_kernel divides by Ho * Wo, Wo and the shuffle + blur kernels' tile counts; a wrong quotient is a wrong input address.
The form must be exact for every dividend below 2^31, so every divisor is checked at 0, d - 1, d, around a few hundred random multiples (k d - 1, k d:
the two values a rounding error of the multiplier would move first), at the largest pixel index of a 64-frame 560 x 560 tail launch, at 2^31 - 1, and
densely over 0 .. 2^20.
"""
import ctypes as C

import numpy as np
import pytest

from vsdeoldify_amd import _native as nat

# 1: H x 1 / 1 x W maps; 2, 3: tiny maps; 15, 18, 35: map widths and tile strides; 324 = 18^2, 1 225 = 35^2, 313 600 = 560^2: pixels per frame; 560: the
# tail's width; 2^16 +- 1 and 2^20 + 7: divisors next to a power of two, where the multiplier's rounding is largest
DIVISORS = [1, 2, 3, 15, 18, 35, 324, 1225, 560, 313600, 2**16 - 1, 2**16 + 1, 2**20 + 7]
TAIL_LAST_PIXEL = 64 * 560 * 560 - 1
assert TAIL_LAST_PIXEL == 20_070_399


def fast_div(d, n):
    lib = nat.load()
    n = np.ascontiguousarray(n, np.uint32)
    q = np.empty_like(n)
    rc = lib.havc_conv_fast_div(C.c_uint32(d), n.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.c_void_p), C.c_int64(n.size))
    assert rc == 0
    return q


@pytest.mark.parametrize("d", DIVISORS)
def test_fast_div_edges_and_multiples(d):
    r = np.random.default_rng(d)
    k = r.integers(1, (2**31 - 1) // d + 1, size=400, dtype=np.int64)
    k = np.concatenate([k, [1, 2, (2**31 - 1) // d]])
    n = np.concatenate([[0, d - 1, d, TAIL_LAST_PIXEL, 2**31 - 1], k * d - 1, k * d]).astype(np.int64)
    n = n[(n >= 0) & (n < 2**31)]
    got = fast_div(d, n)
    bad = np.nonzero(got.astype(np.int64) != n // d)[0]
    assert bad.size == 0, f"divisor {d}: {n[bad[0]]} // {d} = {n[bad[0]] // d}, fast_div gives {got[bad[0]]}"


@pytest.mark.parametrize("d", DIVISORS)
def test_fast_div_dense_sweep(d):
    n = np.arange(2**20 + 1, dtype=np.int64)
    got = fast_div(d, n)
    bad = np.nonzero(got.astype(np.int64) != n // d)[0]
    assert bad.size == 0, f"divisor {d}: {n[bad[0]]} // {d} = {n[bad[0]] // d}, fast_div gives {got[bad[0]]}"


def test_fast_div_top_of_the_range_for_every_small_divisor():
    """the last 4096 dividends below 2^31 (where the multiplier's error term is largest) against every divisor up to 4096 and the powers of two up to 2^31"""
    n = np.arange(2**31 - 4096, 2**31, dtype=np.int64)
    for d in list(range(1, 4097)) + [2**k for k in range(13, 32)] + [2**31 - 1]:
        got = fast_div(d, n)
        assert np.array_equal(got.astype(np.int64), n // d), d


def test_fast_div_rejects_what_it_does_not_cover():
    lib = nat.load()
    buf = np.zeros(1, np.uint32)
    p = buf.ctypes.data_as(C.c_void_p)
    assert lib.havc_conv_fast_div(C.c_uint32(0), p, p, C.c_int64(1)) != 0
    assert lib.havc_conv_fast_div(C.c_uint32(2**31 + 1), p, p, C.c_int64(1)) != 0
