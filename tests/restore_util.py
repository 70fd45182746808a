"""Shared by tests/test_restore_host.py and tests/test_gpu_restore.py: a float64 reference of the Spline36 resize (havc_resize_n, filter 1) and the table of
cases the GPU test runs.  The acceptance rule is tests/resize_util.py's, unchanged: the same eps derivation (n_h + n_v + 4 roundings of 2^-24 on values of at
most 255 * S_h * S_v), a byte exact outside near-ties and either neighbour inside them, the near-tie share of the reference alone capped at 1 %.

Spline36 (support 3), the kernel of Avisynth / zimg:
    0 <= x < 1:             ((13/11 x - 453/209) x - 3/209) x + 1
    1 <= x < 2, t = x - 1:  ((-6/11 t + 270/209) t - 156/209) t
    2 <= x < 3, t = x - 2:  ((1/11 t - 45/209) t + 26/209) t
Same structure as the Spline64 tables: centre (i + 0.5) / scale - 0.5, the support widened by the down-sampling ratio, ceil(2 * support) + 1 taps from
floor(centre - support) + 1 on, weights normalised to sum 1, edges replicated.

The cases mirror tests/test_gpu_resize.py (a-h, the same shapes).  With support 3 instead of 4 the same shapes give fewer taps, so some land on another
instance of the batched kernel than their Spline64 twin (d: 22 taps -> 29, e: 25 -> 29, f: 32 -> 32); the variant and tap count of every case are asserted
through havc_resize_plan_filter before it runs.  f48 is added: the smallest ratio whose Spline36 pass has more than 32 taps with a staged span inside 4 KiB.
"""
import collections
import ctypes

import numpy as np

from tests import resize_util as RU

SPLINE64, SPLINE36 = 0, 1

Case = collections.namedtuple("Case", "seed n sh sw dw dh variant taps luma")
CASES = {
    "a": Case(0, 65, 513, 40, 130, 200, 9, 7, False),
    "b": Case(1, 33, 500, 96, 260, 124, 9, 7, True),
    "c": Case(2, 33, 500, 520, 260, 500, 17, 13, False),
    "d": Case(3, 65, 513, 42, 12, 100, 29, 22, False),
    "e": Case(4, 65, 513, 93, 24, 100, 29, 25, False),
    "f": Case(5, 33, 500, 1326, 260, 60, 32, 32, False),
    "f48": Case(8, 33, 500, 1347, 260, 60, 48, 33, False),
    "g1": Case(6, 1, 97, 1400, 260, 97, 0, 34, False),
    "g2": Case(6, 3, 50, 600, 96, 31, 0, 39, False),
    "h": Case(7, 1, 61, 83, 83, 61, 0, 7, True),
}


def spline36(x):
    x = np.abs(np.asarray(x, np.float64))
    t1, t2 = x - 1.0, x - 2.0
    return np.where(x < 1.0, ((13.0 / 11.0 * x - 453.0 / 209.0) * x - 3.0 / 209.0) * x + 1.0,
                    np.where(x < 2.0, ((-6.0 / 11.0 * t1 + 270.0 / 209.0) * t1 - 156.0 / 209.0) * t1,
                             np.where(x < 3.0, ((1.0 / 11.0 * t2 - 45.0 / 209.0) * t2 + 26.0 / 209.0) * t2, 0.0)))


def n_taps(src, dst):
    return int(np.ceil(2.0 * 3.0 / min(dst / src, 1.0))) + 1


def taps36(src, dst):
    """(edge-replicated positions [dst, n], float64 weights [dst, n])"""
    scale = dst / src
    fscale = min(scale, 1.0)
    support = 3.0 / fscale
    n = int(np.ceil(2.0 * support)) + 1
    center = (np.arange(dst) + 0.5) / scale - 0.5
    start = np.floor(center - support).astype(np.int64) + 1
    pos = start[:, None] + np.arange(n)[None, :]
    w = spline36((pos - center[:, None]) * fscale)
    w = w / w.sum(1, keepdims=True)
    return np.clip(pos, 0, src - 1), w


def ref36(clip_u8, dw, dh):
    """uint8 [n, sh, sw, 3] -> resize_util.Ref64 of the Spline36 resize: both passes in float64, horizontal first"""
    clip_u8 = np.asarray(clip_u8)
    assert clip_u8.ndim == 4 and clip_u8.dtype == np.uint8
    n, sh, sw, _ = clip_u8.shape
    px, wx = taps36(sw, dw)
    py, wy = taps36(sh, dh)
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
    v = np.zeros((n, dh, dw, 3), np.float64)
    for t in range(py.shape[1]):
        v += wy[None, :, t, None, None] * tmp[:, py[:, t], :, :]
    n_h, n_v = px.shape[1], py.shape[1]
    S_h, S_v = float(np.abs(wx).sum(1).max()), float(np.abs(wy).sum(1).max())
    eps = (n_h + n_v + 4) * 2.0 ** -24 * 255.0 * S_h * S_v
    return RU.Ref64(v, n_h, n_v, S_h, S_v, eps)


def case_operands(name):
    """(clip, luma or None) of a case: random uint8, seed = the case's, frame 0 random 0 / 255"""
    c = CASES[name]
    r = np.random.default_rng(c.seed)
    clip = r.integers(0, 256, (c.n, c.sh, c.sw, 3), dtype=np.uint8)
    clip[0] = r.integers(0, 2, clip[0].shape, dtype=np.uint8) * 255
    luma = r.integers(0, 256, (c.n, c.dh, c.dw, 3), dtype=np.uint8) if c.luma else None
    return clip, luma


def plan(lib, sw, dw, n_rows, filter_id):
    """havc_resize_plan_filter -> (h_taps, h_variant, bytes of LDS the batched kernel reserves for a tile's source span)"""
    taps, var = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = lib.havc_resize_plan_filter(sw, dw, n_rows, filter_id, ctypes.byref(taps), ctypes.byref(var))
    assert rc >= 0, rc
    return taps.value, var.value, rc
