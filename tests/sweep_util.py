"""Shared by tests/test_gpu_colour_sweep.py: the whole 8-bit RGB input space as images, and the rules by which the HIP colour kernels are compared
with the oracle over it.

Inputs.  Pixel i of the cube is the triple (i >> 16, (i >> 8) & 255, i & 255); the 2^24 pixels are cut into slabs of whole 4096-pixel rows.  A kernel
that takes two images gets the cube and the cube under the bijection i -> (i * K + c) mod 2^24 (K odd): each image still holds every triple once and
the pairing is far from the diagonal -- the structured substitute for the 2^48 pairs nobody can sweep.  byte_pairs() holds every (a, b) byte pair in
every channel, for kernels that work per channel.

Lab -> RGB.  The reference truncates clip(x, 0, 1) * 255, so a device libm that is one ulp away from numpy's may land on the other side of an integer.
lab2rgb_unclipped() restates oracle.zhang.lab2rgb in float64 without the final clip; a byte is left out of the comparison only where that value times
255 lies within LEFT_OUT_WINDOW of an integer.  libm and summation-order differences reach about 1e-13 on this chain, so the window is 10^4 times wider
than they need, and a chance hit costs 2e-9 per byte.  The share of left-out bytes is a property of the oracle alone and is capped at LEFT_OUT_CAP
before any output of the code under test is looked at.
"""
import numpy as np

from oracle import zhang

N_CUBE = 1 << 24
ROW = 4096
LEFT_OUT_WINDOW = 1e-9
LEFT_OUT_CAP = 5e-4
PARTNERS = ((0x9E3779, 0x5BD1E9), (0x2545F5, 0xC0FFEE))          # (K, c): K odd, so i -> (i K + c) mod 2^24 is a bijection


def triples(idx):
    """cube pixel indices -> uint8 [..., 3]"""
    idx = np.asarray(idx, np.int64)
    return np.stack([(idx >> 16) & 255, (idx >> 8) & 255, idx & 255], -1).astype(np.uint8)


def indices(img):
    """uint8 [..., 3] -> cube pixel indices (int64)"""
    a = np.asarray(img).astype(np.int64)
    return (a[..., 0] << 16) | (a[..., 1] << 8) | a[..., 2]


def cube_slabs(n_slabs=8):
    """yields n_slabs uint8 images [4096 / n_slabs, 4096, 3] that together hold every RGB triple exactly once (slab k: R in [256 k / n, 256 (k + 1) / n))"""
    assert ROW % n_slabs == 0
    rows = ROW // n_slabs
    for k in range(n_slabs):
        yield triples(np.arange(k * rows * ROW, (k + 1) * rows * ROW, dtype=np.int64)).reshape(rows, ROW, 3)


def partner(slab, K, c):
    """the image whose pixel is the cube pixel (i * K + c) mod 2^24, i the cube index of the pixel of `slab` at the same place"""
    assert K % 2 == 1 and 0 < K < N_CUBE and 0 <= c < N_CUBE
    return triples((indices(slab) * K + c) & (N_CUBE - 1))


def byte_pairs():
    """(a, b): two uint8 images [256, 256, 3]; in every channel the pair (a, b) runs through all 65 536 byte pairs (the channels in different orders)"""
    i, j = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    a = np.stack([i, i, i], -1).astype(np.uint8)
    b = np.stack([j, (j + 97) & 255, (j + 171) & 255], -1).astype(np.uint8)
    return a, b


def assert_same_bytes(got, want, inputs, label):
    """np.array_equal with a message one can act on: the number of differing pixels and the first ten as (input triple(s), got, want).
    inputs: the image, or the tuple of images, the two results were computed from (same height and width).  Returns the pixels compared."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint8, (label, got.shape, want.shape, got.dtype, want.dtype)
    if not np.array_equal(got, want):
        inputs = inputs if isinstance(inputs, (tuple, list)) else (inputs,)
        bad = (got != want).reshape(got.shape[0], got.shape[1], -1).any(-1)
        where = np.argwhere(bad)
        first = [(tuple(np.asarray(x)[y, xx].tolist() for x in inputs), got[y, xx].tolist(), want[y, xx].tolist()) for y, xx in where[:10]]
        raise AssertionError(f"{label}: {len(where)} of {bad.size} pixels differ; first (input(s), got, want): {first}")
    return got.shape[0] * got.shape[1]


# ---- Lab -> RGB: the oracle without its last clip, and the bytes an ulp of libm may flip -----------------------------------------------------------------
def lab2rgb_unclipped(lab):
    """oracle.zhang.lab2rgb in float64, operation for operation, returning the sRGB value BEFORE the clip to [0, 1]"""
    lab = np.asarray(lab, np.float64)
    L, a, b = lab[..., 0], lab[..., 1], lab[..., 2]
    y = (L + 16.0) / 116.0
    x = a / 500.0 + y
    z = y - b / 200.0
    z = np.where(z < 0, 0.0, z)
    out = np.stack([x, y, z], -1)
    mask = out > 0.2068966
    out = np.where(mask, np.power(out, 3.0), (out - 16.0 / 116.0) / 7.787)
    out = out * zhang.D65
    arr = out @ zhang.RGB_FROM_XYZ.T
    mask = arr > 0.0031308
    return np.where(mask, 1.055 * np.power(np.where(mask, arr, 1.0), 1 / 2.4) - 0.055, arr * 12.92)


def left_out(unclipped):
    """bool mask: bytes whose unclipped value times 255 lies within LEFT_OUT_WINDOW of an integer"""
    v = unclipped * 255.0
    return np.abs(v - np.rint(v)) < LEFT_OUT_WINDOW


def denormalise_lab(lab_norm):
    """float32 planes [3, H, W] of ColorMNet's normalised Lab -> float32 Lab [H, W, 3], in the float32 steps of inv_lll2rgb_trans
    (oracle.colormnet_net.lab_tensor_to_rgb): (x - [-1, 0, 0]) / float32([1 / 50, 1 / 110, 1 / 110])"""
    x = np.asarray(lab_norm, np.float32)
    mean = np.array([-1.0, 0.0, 0.0], np.float32).reshape(3, 1, 1)
    std = np.array([1 / 50., 1 / 110., 1 / 110.], np.float32).reshape(3, 1, 1)
    return np.ascontiguousarray(((x - mean) / std).transpose(1, 2, 0))


def perturb_ab(lab_norm, slab_index, amplitude=40.0, seed=24):
    """lab_norm with seeded uniform noise of +-amplitude Lab units on a and b (float32 planes): reaches the out-of-gamut clip, the fz < 0 clamp and the
    linear sRGB segment"""
    r = np.random.default_rng([seed, slab_index])
    out = np.array(lab_norm, np.float32, copy=True)
    out[1:] += (r.uniform(-amplitude, amplitude, out[1:].shape) / 110.0).astype(np.float32)
    return out
