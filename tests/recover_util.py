"""Shared by tests/test_recover_host.py and tests/test_gpu_recover.py: the cases of tests/golden/recover.npz, and the CPU reference of
HAVC_recover_clip_color = ChromaRetentionMerge (vsdeoldify/vsslib/mcomb.py:450-516) on a clip.

`recover_clip_color_ref` is assembled from the oracle: oracle.tweaks.restore_color_gradient (the gradient selector's frame body), oracle.cvcolor (cv2's HSV /
YUV), oracle.pipeline.get_image_luma and chroma_post_process, oracle/resample.py's Spline64, oracle.imaging.pil_blend (std.Merge's stand-in).  `restore_color`
(vsslib/restcolor.py:38-83 with tht_scen = 1.0, hue_adjust 'none') and the clip-level steps are restated here in plain numpy.  The `rules` argument switches
single rules OFF (or round): tests/test_recover_host.py uses it to show that the fixture can tell."""
import json
import math
import os

import numpy as np

from oracle import cvcolor, imaging, pipeline, resample, tweaks
from tests.conftest import GOLDEN

DEF_STANDARD_DARK, DEF_STANDARD_BRIGHT = 0.22, 0.78                          # vsslib/constants.py:28-29
BINARY_FIRST = 15                                                            # vsfilters.py:339

_FIXTURE = None


def fixture():
    global _FIXTURE
    if _FIXTURE is None:
        with np.load(os.path.join(GOLDEN, "recover.npz")) as z:
            _FIXTURE = {k: z[k] for k in z.files}
    return _FIXTURE


def cases():
    """[(index, parameter dict, clip, clip_color, expected output, recorded Spline64 sizes)]"""
    g = fixture()
    out = []
    for i, c in enumerate(g["cases"]):
        c = json.loads(str(c))
        name = c.pop("clip")
        out.append((i, c, g["clip_" + name], g["color_" + name], g[f"out_{i}"], [tuple(s) for s in g[f"sizes_{i}"].tolist()]))
    return out


def recover_size(width):
    """mcomb.py:482-484 -> the square size, or None when the clip is not resized"""
    rf = min(max(math.trunc(0.4 * width / 16), 16), 48)
    fs = min(rf * 16, width)
    return fs if fs < width else None


def restore_color(np_color, np_gray, sat=1.0, tht=15, weight=0.0, return_mask=False, swap_sign=False):
    """restcolor.py:38-83 with tht_scen = 1.0 (its early return needs 0 < tht_scen < 1) and hue_adjust 'none'"""
    hsv_color = cvcolor.rgb2hsv_u8(np_color)
    hsv_gray = cvcolor.rgb2hsv_u8(np_gray)
    hsv_color[:, :, 1] = hsv_color[:, :, 1] * min(max(sat, 0), 10)              # for every sat; float -> uint8 cast
    np_color_sat = cvcolor.hsv2rgb_u8(hsv_color)
    hsv_mask = np.where(hsv_gray[:, :, 1] < tht, 255, 0)
    mask_rgb = np_gray.copy()
    for i in range(3):
        mask_rgb[:, :, i] = hsv_mask
    if return_mask:
        return mask_rgb
    white = (mask_rgb / 255).astype(float)                                     # np_image_mask_merge(normalize=True)
    res = (np_gray * (1 - white) + np_color_sat * white).clip(0, 255).astype(np.uint8)
    to_gray, to_color = (np_color_sat, np_gray) if swap_sign else (np_gray, np_color_sat)
    if weight > 0:                                                             # np_weighted_merge
        res = (np.multiply(res, 1 - weight) + np.multiply(to_gray, weight)).clip(0, 255).astype(np.uint8)
    if weight < 0:
        res = (np.multiply(res, 1 + weight) + np.multiply(to_color, -weight)).clip(0, 255).astype(np.uint8)
    return res


def frame_is_standard(frame, rules=()):
    f_luma = pipeline.get_image_luma(frame, 255)
    standard = DEF_STANDARD_DARK <= f_luma <= DEF_STANDARD_BRIGHT
    return (not standard) if "flip_gate" in rules else standard


def gradient_frame(gray, color, sat, tht, weight, alpha, return_mask=False, algo=0, rules=()):
    """color_grad_frame, vsfilters.py:391-412"""
    if not frame_is_standard(gray, rules):
        weight = min(weight, -0.5)
        alpha = max(alpha, 4.0)
    return tweaks.restore_color_gradient(color, gray, sat, tht, weight, alpha, return_mask, algo)


def binary_frame(n, gray, color, sat, tht, weight, return_mask=False, rules=()):
    """color_frame, vsfilters.py:327-351"""
    if n < BINARY_FIRST and "no_n15" not in rules:
        return gray.copy()
    if not frame_is_standard(gray, rules):
        weight = min(weight, -0.8)
    return restore_color(color, gray, sat, tht, weight, return_mask, swap_sign="swap_sign" in rules)


def selector_clip(clip, clip_color, sat, tht, weight, alpha, return_mask=False, binary_mask=False, algo=0, first_frame=0, rules=()):
    """what havc_recover_color_clip computes: the selector on every frame (alpha as given)"""
    if binary_mask:
        return np.stack([binary_frame(first_frame + i, g, c, sat, tht, weight, return_mask, rules) for i, (g, c) in enumerate(zip(clip, clip_color))])
    return np.stack([gradient_frame(g, c, sat, tht, weight, alpha, return_mask, algo, rules) for g, c in zip(clip, clip_color)])


def recover_clip_color_ref(clip, clip_color, sat=0.8, tht=30, strength=1.0, alpha=2.0, mask_weight=1.0, chroma_resize=True, return_mask=False,
                           binary_mask=False, algo=0, first_frame=0, rules=(), sizes=None):
    """HAVC_recover_clip_color (vsdeoldify/__init__.py:2956-2992) -> ChromaRetentionMerge (mcomb.py:479-516) on uint8 clips [n, h, w, 3], on the CPU.
    sizes: a list that receives the (width, height) of every Spline64 call."""
    clip, clip_color = np.asarray(clip), np.asarray(clip_color)
    h, w = clip.shape[1:3]
    alpha = max(min(alpha, 10.0), 1.0)
    fs = recover_size(w) if chroma_resize and not return_mask else None

    def spline64(x, dw, dh):
        if sizes is not None:
            sizes.append((dw, dh))
        return np.stack([resample.resize_rgb8(f, dw, dh) for f in x])
    a, b = (clip, clip_color) if fs is None else (spline64(clip, fs, fs), spline64(clip_color, fs, fs))
    restored = selector_clip(a, b, sat, tht, mask_weight, alpha, return_mask, binary_mask, algo, first_frame, rules)
    if return_mask:
        return restored
    if fs is not None:
        restored = spline64(restored, w, h)
        restored = np.stack([pipeline.chroma_post_process(r, o) for r, o in zip(restored, clip)])    # vs_sc_recover_clip_luma
    if strength == 0:                                                          # vs_simple_merge
        return clip
    if strength == 1:
        return restored
    return imaging.pil_blend(clip, restored, strength)


def make_frame(rng, level, shape, gray_share=0.5):
    """a frame around `level` with a share of (almost) gray pixels"""
    h, w = shape
    base = level + 18.0 * rng.standard_normal((h, w, 1))
    tint = rng.integers(-60, 61, (h, w, 3)) * (rng.random((h, w, 1)) > gray_share) + rng.integers(-4, 5, (h, w, 3))
    return np.clip(base + tint, 0, 255).astype(np.uint8)


def make_donor(rng, shape):
    h, w = shape
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    c = np.stack([128 + 110 * np.sin(xx / 3.0 + yy / 5.0), 128 + 110 * np.cos(yy / 2.0 - xx / 7.0), 128 + 110 * np.sin((xx + yy) / 4.0 + 1.0)], -1)
    return np.clip(c + 10 * rng.standard_normal((h, w, 3)), 0, 255).astype(np.uint8)


def make_clips(levels, shape, seed=7):
    rng = np.random.default_rng(seed)
    return np.stack([make_frame(rng, v, shape) for v in levels]), np.stack([make_donor(rng, shape) for _ in levels])
