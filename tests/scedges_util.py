"""Shared by tests/test_scedges_host.py and tests/test_gpu_scedges.py (and tools/scedges_bench.py): the numpy restatement of the pixel work behind
HAVC_SceneDetectEdges -- THE DEFINITION of havc_scene_edge_stats (csrc/scedge.hip).  It restates vs_edge_based_scenedetect steps 1-2
(vsslib/vsscdetect_edge.py:168-182) on the small RGB clip.  UNPINNED: TCanny, akarin, std.Convolution, std.MaskedMerge and zimg are native code that is
not in the reference tree, so there is nothing to execute it against.

  Y        = (cr R + cg G + cb B + bias) >> 16                                   scdetect.LUMA_LIMITED (default) or LUMA_FULL
  reflect  reflect-101 with period 2 (n - 1), applied as often as needed; n == 1 -> 0.  Every neighbourhood uses it.
  kirsch   four std.Convolution passes (saturate=False = absolute value, divisor 1: the matrices sum to 0) with the matrices the reference builds,
           each min(|sum|, 255) in integers; the maximum of the four
  E        'x 255 / sqrt 255 *' in float32, rounded half up: a 256-entry table
  tcanny   TCanny(mode=1, sigma) on E: r = max(int(3 sigma + 0.5), 1); weights exp(-x^2 / (2 sigma^2)) (float64 exp, rounded to float32) normalised by their
           float32 sum from tap -r to +r; vertical pass, then horizontal, taps added from -r to +r, every product and sum rounded to float32;
           gx = ((tr + r + br) - (tl + l + bl)) * 0.5, gy = ((tl + t + tr) - (bl + b + br)) * 0.5; float32 sqrt; int(gm + 0.5), at most 255
  mask     min(kirsch + tcanny, 255)
  diff     |Y_n - Y_j|, j = n + offset for n < N - offset, else N - offset: `gray[offset:] + gray[-offset]` (:174) is a clip of N - offset + 1 frames, and
           VapourSynth answers a request beyond a clip's end with its last frame
  masked   (diff * mask + 127) // 255                                            the project's std.MaskedMerge stand-in with a = 0
  per frame: sum_y, sad_prev (against frame max(n - 1, 0): what the misc.SCDetect stand-in reads), sad_next = sum of diff, sum_masked.
"""
import functools
import json
import math
import os

import numpy as np

from vsdeoldify_amd import scdetect as SD
from vsdeoldify_amd import scdetect_edge as SE

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scdetect_edges.npz")
TILE_H, TILE_W = 32, 64                                    # ET_H, ET_W of csrc/scedge.hip
# h x w.  1 x 1, 3 x 5, 7 x 9: smaller than the halo (r + 1 = 5), so reflection folds more than once; one tile; one tile + 1 in each direction; several
# tiles with ragged edges and more than one block per frame
SIZES = [(1, 1), (3, 5), (7, 9), (TILE_H, TILE_W), (TILE_H + 1, TILE_W + 1), (130, 257)]


@functools.lru_cache(maxsize=None)
def fixture():
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files}


def params(g, key):
    return json.loads(str(g[key]))


# ---- the definition ----------------------------------------------------------------------------------------------------------------------------------------
def reflect(i, n):
    i = np.asarray(i, np.int64)
    if n == 1:
        return np.zeros_like(i)
    m = np.mod(i, 2 * (n - 1))
    return np.where(m <= n - 1, m, 2 * (n - 1) - m)


def gray(clip, coeffs=SD.LUMA_LIMITED):
    cr, cg, cb, bias = coeffs
    c = np.asarray(clip).astype(np.int64)
    y = (cr * c[..., 0] + cg * c[..., 1] + cb * c[..., 2] + bias) >> 16
    assert y.min() >= 0 and y.max() <= 255
    return y.astype(np.uint8)


def shifted(plane, dy, dx):
    """plane[reflect(y + dy), reflect(x + dx)]"""
    h, w = plane.shape
    return plane[reflect(np.arange(h) + dy, h)][:, reflect(np.arange(w) + dx, w)]


def kirsch_matrices():
    """vsscdetect_edge.py:114-117, as written there"""
    w = [5] * 3 + [-3] * 5
    weights = [w[-i:] + w[:-i] for i in range(4)]
    return [(w[:4] + [0] + w[4:]) for w in weights]


def kirsch_passes(y):
    y = np.asarray(y).astype(np.int64)
    out = []
    for m in kirsch_matrices():
        s = np.zeros(y.shape, np.int64)
        for k, c in enumerate(m):
            s += c * shifted(y, k // 3 - 1, k % 3 - 1)
        out.append(np.minimum(np.abs(s), 255))
    return out


def kirsch(y):
    return np.maximum.reduce(kirsch_passes(y))


def enhance_table():
    x = np.arange(256, dtype=np.float32)
    v = np.sqrt(x / np.float32(255)) * np.float32(255)
    assert v.dtype == np.float32
    return np.minimum(np.floor(v + np.float32(0.5)), 255).astype(np.uint8)


def radius(sigma):
    return max(int(3 * sigma + 0.5), 1)


def weights(sigma):
    r = radius(sigma)
    w = np.array([math.exp(-float(k * k) / (2.0 * sigma * sigma)) for k in range(-r, r + 1)]).astype(np.float32)
    s = np.float32(0)
    for v in w:
        s = np.float32(s + v)
    return (w / s).astype(np.float32)


def blur(plane, sigma):
    """vertical pass, then horizontal; float32 throughout, tap -r first"""
    w, r = weights(sigma), radius(sigma)
    p = np.asarray(plane).astype(np.float32)
    for axis in (0, 1):
        acc = np.zeros(p.shape, np.float32)
        for k in range(-r, r + 1):
            acc = acc + w[k + r] * (shifted(p, k, 0) if axis == 0 else shifted(p, 0, k))
            assert acc.dtype == np.float32
        p = acc
    return p


def tcanny(plane, sigma=SE.DEF_CANNY_SIGMA):
    b = blur(plane, sigma)
    half = np.float32(0.5)
    tl, t, tr = shifted(b, -1, -1), shifted(b, -1, 0), shifted(b, -1, 1)
    l, r = shifted(b, 0, -1), shifted(b, 0, 1)
    bl, bt, br = shifted(b, 1, -1), shifted(b, 1, 0), shifted(b, 1, 1)
    gx = (((tr + r) + br) - ((tl + l) + bl)) * half
    gy = (((tl + t) + tr) - ((bl + bt) + br)) * half
    gm = np.sqrt(gx * gx + gy * gy)
    assert gm.dtype == np.float32
    return np.minimum((gm + half).astype(np.int64), 255)


def edge_mask(y, sigma=SE.DEF_CANNY_SIGMA):
    """the mask of one gray plane, int64"""
    return np.minimum(kirsch(y) + tcanny(enhance_table()[np.asarray(y, np.uint8)], sigma), 255)


def edge_stats_np(clip, offset=2, coeffs=SD.LUMA_LIMITED, sigma=SE.DEF_CANNY_SIGMA):
    """-> (dict of int64 arrays sum_y, sad_prev, sad_next, sum_masked, one entry per frame; mask u8 [n, h, w])"""
    y = gray(clip, coeffs).astype(np.int64)
    n = y.shape[0]
    assert 1 <= offset < n
    out = {k: np.zeros(n, np.int64) for k in ("sum_y", "sad_prev", "sad_next", "sum_masked")}
    mask = np.stack([edge_mask(f, sigma) for f in y])
    for i in range(n):
        diff = np.abs(y[i] - y[SE.next_index(i, n, offset)])
        out["sum_y"][i] = y[i].sum()
        out["sad_prev"][i] = np.abs(y[i] - y[max(i - 1, 0)]).sum()
        out["sad_next"][i] = diff.sum()
        out["sum_masked"][i] = ((diff * mask[i] + 127) // 255).sum()
    return out, mask.astype(np.uint8)


# ---- the clips -----------------------------------------------------------------------------------------------------------------------------------------------
def _texture(h, w, f, r, level=110.0, a=60.0, b=40.0, px=17.0, py=11.0):
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    return level + a * np.sin(x / px + f) + b * np.cos(y / py - f) + r.normal(0.0, 2.0, (h, w))


def _rgb(v):
    return np.clip(np.rint(v[..., None] + np.array([0.0, 3.0, -5.0])), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def kernel_clip(h, w, n=6, seed=3):
    """six frames of 110 + 60 sin(x / 17 + f) + 40 cos(y / 11 - f) + N(0, 2) (a mask around 70, no pixel at 0 or 255: uniform noise would saturate the
    Kirsch term), frames 1, 3 and 4 with a flat hard-edged rectangle that moves (its inside gives mask 0, its border 255).  On every frame of 64 x 64 and
    above at most half the pixels are at 0 or 255 and both values occur in the clip: checked here, on the numpy mask, with the rectangle in place."""
    r = np.random.default_rng(seed + 1000 * h + w)
    clip = np.empty((n, h, w, 3), np.uint8)
    for f in range(n):
        v = _texture(h, w, 0.9 * f, r)
        if f in (1, 3, 4):
            y0, x0 = h // 4 + f, w // 5 + 2 * f
            v[y0:y0 + max(h // 3, 1), x0:x0 + max(w // 3, 1)] = 235.0 if f != 3 else 20.0
        clip[f] = _rgb(v)
    clip.setflags(write=False)
    if h >= 64 and w >= 64:
        for sigma in (SE.DEF_CANNY_SIGMA, 0.6):
            m = np.stack([edge_mask(p, sigma) for p in gray(clip)])
            extreme = ((m == 0) | (m == 255)).reshape(n, -1).mean(1)
            assert extreme.max() <= 0.5 and (m == 0).any() and (m == 255).any(), (h, w, sigma, extreme)
    return clip


@functools.lru_cache(maxsize=None)
def reference_stats(h, w, offset, limited, sigma):
    """the numpy statistics of kernel_clip(h, w), computed once and shared"""
    st, mask = edge_stats_np(kernel_clip(h, w), offset, SD.LUMA_LIMITED if limited else SD.LUMA_FULL, sigma)
    mask.setflags(write=False)
    return st, mask


@functools.lru_cache(maxsize=None)
def detect_clip(n=24, h=96, w=160, seed=6):
    """24 frames of 160 x 96: scene A (frames 0-7), a cut at 8 to scene B (8-13), a cross-fade from B to C over frames 14-17, C (18-20), a cut at 21 to
    scene D.  The scenes differ in level and pattern by tens of gray levels, so the misc.SCDetect stand-in (mean difference above 0.10) fires at both cuts.  The seed is one with which none of the
    filter's scores lies within 1e-6 of a rounding boundary or threshold (float64 sums in another order may differ that far): the GPU test asserts that."""
    r = np.random.default_rng(seed)
    scenes = [dict(level=75.0, a=35.0, b=25.0, px=17.0, py=11.0), dict(level=150.0, a=-45.0, b=30.0, px=9.0, py=23.0),
              dict(level=95.0, a=30.0, b=-40.0, px=29.0, py=7.0), dict(level=60.0, a=40.0, b=20.0, px=6.0, py=15.0)]
    clip = np.empty((n, h, w, 3), np.uint8)
    for i in range(n):
        f = 0.05 * i
        if i < 8:
            v = _texture(h, w, f, r, **scenes[0])
        elif i < 14:
            v = _texture(h, w, f, r, **scenes[1])
        elif i < 18:
            t = (i - 13) / 5.0
            v = (1 - t) * _texture(h, w, f, r, **scenes[1]) + t * _texture(h, w, f, r, **scenes[2])
        elif i < 21:
            v = _texture(h, w, f, r, **scenes[2])
        else:
            v = _texture(h, w, f, r, **scenes[3])
        clip[i] = _rgb(v)
    clip.setflags(write=False)
    return clip


def detect_edges_np(clip, threshold=0.035, ssim_threshold=0.80, sc_diff_offset=2, sc_min_int=20, sc_mult_tht=15, tht_white=0.70, tht_black=0.10,
                    coeffs=SD.LUMA_LIMITED):
    """scdetect_edge.scene_detect_edges without the GPU, for a clip that needs no resize: the statistics from edge_stats_np, the filter's scores from the
    numpy restatements of tests/scfilter_util.py -> (EdgeSceneInfo, debug); debug["raw"][t_n] = the unrounded (ssim, 1 - hellinger distance), "asked" the pairs"""
    from tests import scfilter_util as FU
    n, h, w, _ = clip.shape
    assert SD.resize_min_hw(w, h) == (w, h)
    st, _ = edge_stats_np(clip, SE.edges_offset(sc_diff_offset, n), coeffs)
    g = FU.gray(clip)
    debug = {"raw": {}, "asked": [], "stats": st}

    def scores(t_n, last):
        s, d = FU.ssim_np(g[t_n], g[last]), SD.hellinger_distance(FU.hist(g[last]), FU.hist(g[t_n]))
        debug["raw"][t_n] = (float(s), 1.0 - d)
        debug["asked"].append((t_n, last))
        return s, d

    info = SE.scene_flags_edges(st["sum_y"], st["sad_prev"], st["sad_next"], st["sum_masked"], h * w, threshold=threshold, ssim_threshold=ssim_threshold,
                                sc_min_int=sc_min_int, sc_mult_tht=sc_mult_tht, tht_white=tht_white, tht_black=tht_black, scores=scores, debug=debug)
    return info, debug
