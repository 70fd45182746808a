"""numpy restatement of havc_equalize_clip (csrc/equalize.hip) and the clips the equalisation tests share.

The selectors (`selector_yuv`, `selector_rgb`, `autowhite`) follow the reference's frame_autolevels_CLAHE_yuv / frame_autolevels_CLAHE_rgb /
frame_autowhite (vsdeoldify/havc_utils.py:869-953, 1103-1122) statement by statement, with vsdeoldify_amd.equalize's scalar functions; they are pinned by
tests/golden/equalize.npz (made by executing the reference, tools/gen_golden_equalize.py) in tests/test_equalize_host.py.

UNPINNED (cv2 is not installed where the fixtures are made): `clahe` and `equalize_hist` are written from OpenCV's documented algorithm
(modules/imgproc/src/clahe.cpp, histogram.cpp); RGB2YUV / YUV2RGB are oracle/cvcolor.py's.  The stand-ins of VapourSynth's native filters are
vsdeoldify_amd.equalize's (its docstring lists them)."""
import functools
import json
import os

import numpy as np

from oracle import cvcolor
from oracle.imaging import pil_blend
from vsdeoldify_amd import equalize as EQ

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "equalize.npz")
F32 = np.float32


@functools.lru_cache(maxsize=None)
def fixture():
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files}


def params(g, key):
    return json.loads(str(g[key]))


# ---- OpenCV (unpinned) ------------------------------------------------------------------------------------------------------------------------------------
def tile_size(w, h):
    ragged = w % 8 != 0 or h % 8 != 0
    pw = w + (8 - w % 8) if ragged else w
    ph = h + (8 - h % 8) if ragged else h
    return pw // 8, ph // 8


def clahe_luts(plane, clip_limit, stats=None):
    """CLAHE_CalcLut_Body -> uint8 [8, 8, 256].  stats (a list) receives (clipped, residual) of every tile."""
    h, w = plane.shape
    tw, th = tile_size(w, h)
    ext = np.pad(plane, ((0, th * 8 - h), (0, tw * 8 - w)), mode="reflect")          # numpy's "reflect" is BORDER_REFLECT_101
    area = tw * th
    limit = max(int(clip_limit * area / 256), 1) if clip_limit > 0 else 0
    scale = F32(255) / F32(area)
    luts = np.empty((8, 8, 256), np.uint8)
    for ty in range(8):
        for tx in range(8):
            hist = np.bincount(ext[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw].ravel(), minlength=256).astype(np.int64)
            if limit > 0:
                clipped = int(np.maximum(hist - limit, 0).sum())
                hist = np.minimum(hist, limit)
                batch = clipped // 256
                residual = clipped - batch * 256
                hist = hist + batch
                if stats is not None:
                    stats.append((clipped, residual))
                if residual != 0:
                    step = max(256 // residual, 1)
                    i = 0
                    while i < 256 and residual > 0:
                        hist[i] += 1
                        i += step
                        residual -= 1
            sums = np.cumsum(hist).astype(np.int32)
            luts[ty, tx] = np.clip(np.rint(sums.astype(F32) * scale), 0, 255).astype(np.uint8)
    return luts


_MEMO = {}


def _memo(kind, plane, clip_limit, stats, make):
    """clahe / equalize_hist of a plane are computed once per (plane, clip_limit): the tests run many parameter sets over the same frames.  The statistics of
    the first computation are handed to every later caller too."""
    key = (kind, plane.shape, plane.tobytes(), clip_limit)
    if key not in _MEMO:
        own = []
        _MEMO[key] = (make(own), own)
    out, own = _MEMO[key]
    if stats is not None:
        stats.extend(own)
    return out


def clahe(plane, clip_limit, stats=None):
    """cv2.createCLAHE(clipLimit=clip_limit, tileGridSize=(8, 8)).apply(plane)"""
    return _memo("clahe", plane, clip_limit, stats, lambda own: _clahe(plane, clip_limit, own))


def _clahe(plane, clip_limit, stats):
    h, w = plane.shape
    tw, th = tile_size(w, h)
    luts = clahe_luts(plane, clip_limit, stats)

    def coord(n, tile):
        f = np.arange(n).astype(F32) * (F32(1.0) / F32(tile)) - F32(0.5)
        t1 = np.floor(f).astype(np.int32)
        a = f - t1.astype(F32)
        return np.maximum(t1, 0), np.minimum(t1 + 1, 7), a, F32(1.0) - a
    tx1, tx2, xa, xa1 = coord(w, tw)
    ty1, ty2, ya, ya1 = coord(h, th)
    v = plane.astype(np.intp)
    Y1, Y2, X1, X2 = ty1[:, None], ty2[:, None], tx1[None, :], tx2[None, :]
    l11, l12, l21, l22 = (luts[a, b, v].astype(F32) for a, b in ((Y1, X1), (Y1, X2), (Y2, X1), (Y2, X2)))
    xa, xa1, ya, ya1 = xa[None, :], xa1[None, :], ya[:, None], ya1[:, None]
    res = (l11 * xa1 + l12 * xa) * ya1 + (l21 * xa1 + l22 * xa) * ya                 # float32 arrays: numpy rounds after every operation
    assert res.dtype == F32
    return np.clip(np.rint(res), 0, 255).astype(np.uint8)


def equalize_hist(plane, stats=None):
    """cv2.equalizeHist(plane).  stats (a list) receives the first occupied bin."""
    return _memo("hist", plane, None, stats, lambda own: _equalize_hist(plane, own))


def _equalize_hist(plane, stats):
    hist = np.bincount(plane.ravel(), minlength=256).astype(np.int64)
    i0 = int(np.nonzero(hist)[0][0])
    if stats is not None:
        stats.append(i0)
    total = plane.size
    if hist[i0] == total:
        return np.full_like(plane, i0)
    scale = F32(255.0) / F32(total - int(hist[i0]))
    lut = np.zeros(256, np.uint8)
    sums = np.cumsum(hist[i0 + 1:]).astype(np.int32)
    lut[i0 + 1:] = np.clip(np.rint(sums.astype(F32) * scale), 0, 255).astype(np.uint8)
    return lut[plane]


# ---- the reference's selectors, restated (pinned) -------------------------------------------------------------------------------------------------------------
def _luma_blend(img, img_new, luma, consts):
    w = EQ.blend_weight(luma, *consts)                                               # image_luma_blend, imfilters.py:612-624
    return img_new if w is None else pil_blend(img, img_new, w)


def selector_yuv(img, equalise, range_tv, blend):
    """frame_autolevels_CLAHE_yuv (havc_utils.py:869-909) on one RGB frame; equalise(y_plane) stands for clahe.apply"""
    yuv = cvcolor.rgb2yuv_u8(img)
    y_image = yuv[:, :, 0]
    luma = EQ.f_luma(int(y_image.sum(dtype=np.int64)), y_image.size, range_tv)
    if not EQ.luma_gate(luma):
        return img.copy()
    minrange, maxrange = (16, 235) if range_tv else (0, 255)
    yuv = yuv.copy()
    yuv[:, :, 0] = equalise(y_image).clip(min=minrange, max=maxrange).astype(int)
    img_new = cvcolor.yuv2rgb_u8(yuv)
    return _luma_blend(img, img_new, luma, EQ.BLEND_YUV) if blend else img_new


def selector_rgb(img, equalise, range_tv, blend):
    """frame_autolevels_CLAHE_rgb (havc_utils.py:912-953); equalise(plane) stands for clahe.apply (algo 0) or cv2.equalizeHist (algo 1)"""
    y_image = cvcolor.rgb2yuv_u8(img)[:, :, 0]
    luma = EQ.f_luma(int(y_image.sum(dtype=np.int64)), y_image.size, range_tv)       # get_image_luma, imfilters.py:597-601
    if not EQ.luma_gate(luma):
        return img.copy()
    img_new = np.stack([equalise(img[:, :, c]) for c in range(3)], -1)
    return _luma_blend(img, img_new, luma, EQ.BLEND_RGB) if blend else img_new


def autowhite(img, rgb_fact):
    """frame_autowhite (havc_utils.py:1103-1122) + the std.Expr stand-in"""
    n = img.shape[0] * img.shape[1]
    avg = [EQ.plane_average(img[:, :, c].sum(dtype=np.int64), n) for c in range(3)]
    gains = EQ.balance_gains(avg[0], avg[1], avg[2], rgb_fact)
    return np.stack([EQ.expr_mul(img[:, :, c], gains[c]) for c in range(3)], -1)


def rgb_balance(clip, strength, rgb_factor):
    """rgb_balance (havc_utils.py:1087-1145) on a clip"""
    weight = min(max(1.0 - strength, 0.0), 1.0)
    if not 0 <= weight < 1:
        return clip
    return np.stack([EQ.merge15(autowhite(f, rgb_factor), f, weight) for f in clip])


def rgb_equalizer(clip, method=0, clip_limit=1.0, strength=0.5, weight3=0.3, luma_blend=True, range_tv=True, stats=None):
    """rgb_equalizer (havc_utils.py:836-1075), methods 0-3, on a clip uint8 [n, h, w, 3].  stats: dict of lists "clahe" / "hist" (see clahe_luts / equalize_hist)"""
    weight = min(max(1.0 - strength, 0.0), 1.0)
    cs = None if stats is None else stats.setdefault("clahe", [])
    hs = None if stats is None else stats.setdefault("hist", [])
    cl = lambda p: clahe(p, clip_limit, cs)
    eh = lambda p: equalize_hist(p, hs)
    out = []
    for f in clip:
        if method == 0:
            a = selector_yuv(f, cl, range_tv, luma_blend)
        elif method == 1:
            a = selector_rgb(f, eh, range_tv, luma_blend)
        elif method == 2:
            a = selector_rgb(f, cl, range_tv, luma_blend)
        else:
            a = EQ.merge15(selector_yuv(f, cl, range_tv, luma_blend), selector_rgb(f, eh, range_tv, luma_blend), weight3)
        out.append(EQ.merge15(a, f, weight) if 0 <= weight < 1 else f)
    return np.stack(out)


def auto_levels(clip, mode="Light", method=0, luma_blend=False, range_tv=True):
    """HAVC_auto_levels -> vs_auto_levels (havc_utils.py:785-833), composed"""
    strength = [0.0, 0.98, 0.99, 1.0][["none", "light", "medium", "strong"].index(mode.lower())]
    if range_tv:
        clip = EQ.tv_in_table()[clip]
    clip = rgb_equalizer(clip, method=method, strength=strength, luma_blend=luma_blend, range_tv=range_tv)
    return EQ.tv_out_table()[clip] if range_tv else clip


def bw_tune(clip, tune="Light", method=0, luma_blend=True, range_tv=True):
    """HAVC_bw_tune (vsdeoldify/__init__.py:1266-1339), composed"""
    i = ["none", "light", "medium", "strong"].index(tune.lower())
    if i == 0:
        return clip
    s = [0.0, 0.30, 0.40, 0.50][i]
    if range_tv:
        clip = EQ.tv_in_table()[clip]
    clip = rgb_balance(clip, s, [[1.0, 0.96, 0.94, 0.92][i], [1.0, 1.03, 1.05, 1.08][i], 1.0])
    clip = rgb_equalizer(clip, method=method, strength=s, weight3=s, luma_blend=luma_blend, range_tv=range_tv)
    return EQ.tv_out_table()[clip] if range_tv else clip


# ---- clips ----------------------------------------------------------------------------------------------------------------------------------------------------
FRAME_KINDS = ("below", "above", "blend", "plain", "constant", "tinted")


@functools.lru_cache(maxsize=None)
def make_clip(h, w, seed=0):
    """6 frames: below the gate (f_luma < 0.15), above it (> 0.70), in the blend zone (0.15 <= f_luma < 0.40), at or above 0.40, one constant frame (inside the
    gate), and a tinted frame whose channels start at different, nonzero values.  Noise over a ramp plus flat patches: whole tiles in one bin (clipped, with
    a residual), bins that stay empty.  Frame 3 also has a gray patch over tiles (3..4, 4..5) whose values are spread as evenly as a tile allows: all
    different while a tile has at most 256 pixels (clipped == 0 at clip limit 1), at most ceil(area / 256) per bin beyond.  The levels hold for range_tv on
    and off (test_gpu_equalize asserts what each frame is)."""
    r = np.random.default_rng(1000 * h + w + seed)
    yy, xx = np.mgrid[0:h, 0:w]

    def textured(level, spread):
        base = level + spread * (xx / max(w - 1, 1) - 0.5) + spread * 0.5 * (yy / max(h - 1, 1) - 0.5)
        f = base[:, :, None] + r.integers(-spread // 3, spread // 3 + 1, (h, w, 3))
        f = np.clip(f, 0, 255).astype(np.uint8)
        f[: max(h // 3, 1), : max(w // 4, 1)] = int(level)                         # a flat patch: whole tiles in one bin
        f[h - max(h // 5, 1):, w - max(w // 3, 1):] = (int(level) // 2, int(level), min(int(level) + 40, 255))
        return f
    clip = np.empty((6, h, w, 3), np.uint8)
    clip[0] = textured(22, 18)
    clip[1] = textured(228, 30)
    clip[2] = textured(78, 60)
    clip[3] = textured(135, 90)
    tw, th = tile_size(w, h)
    area = tw * th
    k = (xx % tw) + tw * (yy % th)
    spread = (k + max(135 - area // 2, 0)) % 256 if area <= 256 else (k * 256) // area
    patch = (slice(3 * th, min(5 * th, h)), slice(4 * tw, min(6 * tw, w)))
    clip[3][patch] = spread[patch][:, :, None]
    clip[4] = 120
    clip[5] = np.clip(textured(120, 70).astype(np.int32) * np.array([0.7, 0.9, 0.6]) + np.array([40, 25, 60]), 0, 255).astype(np.uint8)
    clip.setflags(write=False)
    return clip
