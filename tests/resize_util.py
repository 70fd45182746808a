"""Shared by tests/test_resize_host.py and tests/test_gpu_resize.py: a float64 reference of the Spline64 resize and the rule by which a byte of the fp32
kernels (csrc/colorfilters.hip resize_h_kernel / resize_h_rows_kernel / resize_v_kernel / resize_v4_kernel) is accepted against it.

The reference has the taps of oracle/resample.py (same centres, support, start index and normalisation) but keeps them in float64, replicates edges and
runs the horizontal and then the vertical pass in float64.  Against it the two fp32 passes may err by at most

    eps = (n_h + n_v + 4) * 2^-24 * 255 * S_h * S_v            (n: taps per axis, S: max over outputs of sum |w|)

which is the recursive-summation bound of n_h + n_v rounded products and adds, plus the float32 rounding of the weights of both axes (the + 4), on values
of magnitude at most 255 * S_h * S_v.  The bound is derived, not measured.  A byte whose unrounded value v keeps |frac(v) - 0.5| >= eps must therefore be
exactly clip(floor(v + 0.5), 0, 255); elsewhere (a near-tie) either neighbouring byte is accepted.  The share of near-ties is a property of the reference
alone and is capped at 1 % before any output of the code under test is looked at.
"""
import collections
import ctypes

import numpy as np

from oracle import pipeline, resample

NEAR_TIE_CAP = 0.01

Ref64 = collections.namedtuple("Ref64", "v n_h n_v S_h S_v eps")


def taps64(src, dst):
    """oracle.resample.taps without the rounding of the weights to float32: (edge-replicated positions [dst, n], float64 weights [dst, n])"""
    scale = dst / src
    fscale = min(scale, 1.0)
    support = 4.0 / fscale
    n = int(np.ceil(2.0 * support)) + 1
    center = (np.arange(dst) + 0.5) / scale - 0.5
    start = np.floor(center - support).astype(np.int64) + 1
    pos = start[:, None] + np.arange(n)[None, :]
    w = resample.spline64((pos - center[:, None]) * fscale)
    w = w / w.sum(1, keepdims=True)
    return np.clip(pos, 0, src - 1), w


def ref64(clip_u8, dw, dh):
    """uint8 [n, sh, sw, 3] -> Ref64: v = unrounded float64 [n, dh, dw, 3], tap counts, max sum |w| per axis and the acceptance gap eps"""
    clip_u8 = np.asarray(clip_u8)
    assert clip_u8.ndim == 4 and clip_u8.dtype == np.uint8
    n, sh, sw, _ = clip_u8.shape
    px, wx = taps64(sw, dw)
    py, wy = taps64(sh, dh)
    # horizontal: the taps as a dense [dw, sw] matrix (edge replication adds the weights of clamped positions up), one float64 GEMM per block of rows;
    # the order of summation differs from the kernels', by rounding errors of 1e-13 that eps does not need to cover
    mh = np.zeros((dw, sw), np.float64)
    np.add.at(mh, (np.arange(dw)[:, None], px), wx)
    rows = clip_u8.reshape(n * sh, sw, 3)
    tmp = np.empty((n * sh, dw, 3), np.float64)
    step = max(1, (1 << 23) // (sw * 3))
    for r0 in range(0, n * sh, step):
        blk = rows[r0:r0 + step]
        a = blk.transpose(1, 0, 2).reshape(sw, -1).astype(np.float64)
        tmp[r0:r0 + step] = (mh @ a).reshape(dw, len(blk), 3).transpose(1, 0, 2)
    tmp = tmp.reshape(n, sh, dw, 3)
    # vertical: a tap loop over whole rows
    v = np.zeros((n, dh, dw, 3), np.float64)
    for t in range(py.shape[1]):
        v += wy[None, :, t, None, None] * tmp[:, py[:, t], :, :]
    n_h, n_v = px.shape[1], py.shape[1]
    S_h, S_v = float(np.abs(wx).sum(1).max()), float(np.abs(wy).sum(1).max())
    eps = (n_h + n_v + 4) * 2.0 ** -24 * 255.0 * S_h * S_v
    return Ref64(v, n_h, n_v, S_h, S_v, eps)


def near_ties(ref):
    """bool [n, dh, dw, 3]: bytes whose rounding the fp32 error may flip"""
    return np.abs(ref.v - np.floor(ref.v) - 0.5) < ref.eps


def rounded(ref):
    return np.clip(np.floor(ref.v + 0.5), 0, 255).astype(np.uint8)


def assert_near_tie_share(ref, label, per_pixel=False):
    """the condition of the acceptance rule, from the reference alone; returns the mask (per byte, or per pixel for the fused-luma comparison)"""
    tie = near_ties(ref)
    if per_pixel:
        tie = tie.any(-1)
    share = float(tie.mean())
    print(f"{label}: taps {ref.n_h} x {ref.n_v}, S {ref.S_h:.4f} x {ref.S_v:.4f}, eps {ref.eps:.3e}, near-tie share {share:.5f}"
          f" ({'pixels' if per_pixel else 'bytes'})")
    assert share < NEAR_TIE_CAP, (label, share)
    return tie


def check_bytes(got, ref, tie, label):
    """the acceptance rule on the plain resize: every byte of every frame; tie = assert_near_tie_share(ref, label)"""
    assert got.shape == ref.v.shape and got.dtype == np.uint8, (got.shape, ref.v.shape)
    want = rounded(ref)
    bad = (got != want) & ~tie
    lo = np.clip(np.floor(ref.v), 0, 255).astype(np.uint8)
    hi = np.clip(np.floor(ref.v) + 1, 0, 255).astype(np.uint8)
    bad_tie = tie & (got != lo) & (got != hi)
    off = int(((got != want) & tie).sum())
    print(f"{label}: {int(tie.sum())} near-tie bytes of {tie.size}, {off} of them differ from floor(v + 0.5); wrong bytes {int(bad.sum())} + {int(bad_tie.sum())}")
    assert not bad.any() and not bad_tie.any(), (label, int(bad.sum()), int(bad_tie.sum()), _first(bad | bad_tie, got, want))
    return int(tie.sum()), off


def check_fused(got, ref, tie, luma, label):
    """with luma_from: post_process of the accepted bytes; a pixel with a near-tie channel is left out (and counted against the same cap, per pixel);
    tie = assert_near_tie_share(ref, label, per_pixel=True)"""
    assert got.shape == ref.v.shape and got.dtype == np.uint8, (got.shape, ref.v.shape)
    want = pipeline.post_process(rounded(ref), luma)
    diff = (got != want).any(-1)
    bad = diff & ~tie
    off = int((diff & tie).sum())
    print(f"{label}: {int(tie.sum())} near-tie pixels of {tie.size} left out, {off} of them differ from post_process(floor(v + 0.5)); wrong pixels {int(bad.sum())}")
    assert not bad.any(), (label, int(bad.sum()), _first(bad, got, want))
    return int(tie.sum()), off


def _first(mask, got, want):
    """index, value and expectation of the first wrong byte / pixel (frame, row, column[, channel])"""
    idx = tuple(int(i) for i in np.argwhere(mask)[0])
    return idx, got[idx].tolist(), want[idx].tolist()


def plan(lib, sw, dw, n_rows):
    """havc_resize_plan -> (h_taps, h_variant, bytes of LDS the batched kernel reserves for a tile's source span)"""
    taps, var = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = lib.havc_resize_plan(sw, dw, n_rows, ctypes.byref(taps), ctypes.byref(var))
    assert rc >= 0, rc
    return taps.value, var.value, rc
