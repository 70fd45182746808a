"""Histogram equalisation of clips without VapourSynth and without cv2: rgb_equalizer (vsdeoldify/havc_utils.py:836-1075, methods 0-3) and rgb_balance
(:1087-1145), the two filters HAVC_bw_tune (vsdeoldify/__init__.py:1266-1339) and HAVC_auto_levels (:3150-3179 -> havc_utils.py:785-833) are made of.

`rgb_equalizer_np` runs them on a clip uint8 [n, h, w, 3] (ndarray or DeviceImage) through `havc_equalize_clip` (csrc/equalize.hip): tile histograms in LDS,
CLAHE's clip / redistribute / prefix sum, the bilinear blend of four tables per pixel, colour conversion, the per-frame gate and blend weight and every
merge in two launches (three with rgb_balance), nothing in between on the host.  A DeviceImage in gives a DeviceImage out and the call only enqueues.

The per-frame scalars are restated here in the reference's own Python (`f_luma`, `luma_gate`, `blend_weight`, `balance_gains`) and pinned by
tests/golden/equalize.npz, which tools/gen_golden_equalize.py makes by executing the reference's selector bodies (frame_autolevels_CLAHE_yuv,
frame_autolevels_CLAHE_rgb, frame_autowhite) and image_luma_blend with real Pillow.  `frame_params` returns what the library computes for the same inputs
(the C++ the kernels run, compiled for the host).

UNPINNED -- neither cv2 nor VapourSynth can be executed where the fixtures are made:
  * cv2.createCLAHE().apply, cv2.equalizeHist: OpenCV's published algorithm (modules/imgproc/src/clahe.cpp, histogram.cpp) -- 8 x 8 tiles of the plane padded
    with BORDER_REFLECT_101 to a multiple of 8 (by 8 - size % 8 on BOTH axes once one is ragged), clip limit max(int(clip_limit * tile_area / 256), 1), the
    excess spread as clipped / 256 per bin plus one for every max(256 / residual, 1)-th bin, lut = saturate(cvRound(float(sum) * (255.0f / tile_area)));
    per pixel txf = x * (1.0f / tile_w) - 0.5f, floor, clamped tile indices, (l11 * xa1 + l12 * xa) * ya1 + (l21 * xa1 + l22 * xa) * ya in float32
    without FMA, cvRound.  equalizeHist: first occupied bin i0, scale = 255.f / (total - hist[i0]), lut[i] = saturate(cvRound(sum * scale)); a constant
    plane keeps its value.  tests/equalize_util.py restates all of it in numpy.  cv2 RGB2YUV / YUV2RGB: oracle/cvcolor.py, as everywhere.
  * std.Levels (8 bit, gamma 1) -> the table int(clamp((v - min_in) / (max_in - min_in), 0, 1) * (max_out - min_out) + min_out + 0.5) (`levels_table`).
  * resize.Bicubic(format=RGB24, range_in_s=.., range_s=..) at unchanged size -> a per-sample range scale rounded to nearest: v * 219 / 255 + 16, and
    (v - 16) * 255 / 219 clamped to 0..255 (`range_table`).  The reference applies Levels AND the range conversion on the way in and on the way out; so
    do `tv_in_table` / `tv_out_table`, one composed table each, folded into the kernels' first load and last store.
  * std.Merge(a, b, w) -> a + (((b - a) * w15 + 16384) >> 15), w15 = int(w * 32768 + 0.5) (`merge15`): w == 0 gives a, w == 1 gives b exactly.
  * std.PlaneStats' PlaneStatsAverage -> sum / (n_pixels * 255) in float64.
  * std.Expr "x g *" on 8-bit samples -> float32(g), a float32 product, round half to even, clamp to 0..255.
Methods 4 (the timecube plugin with LUT files) and 5 (the Retinex MSRCP plugin) are refused, as is a grid other than 8 x 8.
"""
import ctypes as C
import math

import numpy as np

DEF_THT_DARK_BLACK, DEF_THT_BRIGHT_WHITE = 0.15, 0.70          # vsslib/constants.py:45-46
BLEND_YUV = (0.40, 0.90, 0.35, 2.0)                            # havc_utils.py:907: luma_limit, alpha, min_w, decay of image_luma_blend
BLEND_RGB = (0.40, 0.90, 0.15, 4.0)                            # havc_utils.py:951
GRID = 8


# ---- the per-frame scalars, in the reference's Python -----------------------------------------------------------------------------------------------------
def f_luma(sum_y, n_pixels, range_tv):
    """havc_utils.py:878-885 / imfilters.py:597-601 from the integer sum of cv2's Y: np.mean(y) is sum / n in float64; round() is numpy's on a float64"""
    mean = np.float64(int(sum_y)) / np.float64(int(n_pixels))
    if range_tv:
        return max(round(mean / 235, 6) - 0.07, 0)
    return round(mean / 255, 6)


def luma_gate(luma):
    return bool(DEF_THT_DARK_BLACK <= luma <= DEF_THT_BRIGHT_WHITE)


def blend_weight(luma, luma_limit, alpha, min_w, decay):
    """image_luma_blend (imfilters.py:612-624) -> the weight Image.blend gets, or None when img_new is returned as it is"""
    if luma < luma_limit:
        bright_scale = min(max(pow(luma / luma_limit, decay), 0), 1)
        return round(max(alpha * bright_scale, min_w), 6)
    return None


def balance_gains(red, green, blue, rgb_fact):
    """frame_autowhite (havc_utils.py:1103-1120) from the three PlaneStatsAverage values -> (r_gain, g_gain, b_gain)"""
    small_number = 0.000000001
    r, g, b = rgb_fact[0], rgb_fact[1], rgb_fact[2]
    max_rgb = max(red, green, blue)
    red_corr = max_rgb / max(red, small_number)
    green_corr = max_rgb / max(green, small_number)
    blue_corr = max_rgb / max(blue, small_number)
    norm = max(blue, math.sqrt(red_corr * red_corr + green_corr * green_corr + blue_corr * blue_corr) / math.sqrt(3), small_number)
    return round(r * red_corr / norm, 8), round(g * green_corr / norm, 8), round(b * blue_corr / norm, 8)


def plane_average(total, n_pixels):
    """std.PlaneStats' PlaneStatsAverage of an 8-bit plane (stand-in)"""
    return float(int(total)) / (float(int(n_pixels)) * 255.0)


def frame_params(sum_y, n_pixels, range_tv, chan_sums=None, rgb_factor=None):
    """what the library makes of the same numbers (havc_equalize_frame_params: the kernels' C++ on the host, no GPU) ->
    dict(f_luma, gate, w_yuv, w_rgb, gains); a weight of None = no blend"""
    from . import _native as nat
    out = (C.c_double * 7)()
    ch = (C.c_int64 * 3)(*[int(v) for v in chan_sums]) if chan_sums is not None else None
    fa = (C.c_double * 3)(*[float(v) for v in rgb_factor]) if rgb_factor is not None else None
    if nat.load().havc_equalize_frame_params(int(sum_y), ch, int(n_pixels), 1 if range_tv else 0, fa, out) != 0:
        raise ValueError("havc_equalize_frame_params: bad arguments")
    return dict(f_luma=out[0], gate=bool(out[1]), w_yuv=None if out[2] < 0 else np.float32(out[2]), w_rgb=None if out[3] < 0 else np.float32(out[3]),
                gains=tuple(np.float32(v) for v in out[4:7]))


# ---- the stand-ins of VapourSynth's native filters (module docstring) ------------------------------------------------------------------------------------
def levels_table(min_in, max_in, min_out, max_out):
    t = np.empty(256, np.uint8)
    for v in range(256):
        t[v] = int(min(max((v - min_in) / (max_in - min_in), 0), 1) * (max_out - min_out) + min_out + 0.5)
    return t


def range_table(to_limited):
    """full -> limited: round(v * 219 / 255 + 16); limited -> full: round((v - 16) * 255 / 219) clamped.  Integer arithmetic: neither quotient can end in .5"""
    v = np.arange(256, dtype=np.int64)
    if to_limited:
        return ((v * 219 * 2 + 255) // 510 + 16).astype(np.uint8)
    return np.clip(((v - 16) * 255 * 2 + 219) // 438, 0, 255).astype(np.uint8)


def tv_in_table():
    """HAVC_bw_tune / vs_auto_levels on the way in (__init__.py:1325-1326): std.Levels(0, 255 -> 16, 235), then full -> limited"""
    return range_table(True)[levels_table(0, 255, 16, 235)]


def tv_out_table():
    """on the way out (__init__.py:1336-1337): std.Levels(16, 235 -> 0, 255), then limited -> full"""
    return range_table(False)[levels_table(16, 235, 0, 255)]


def w15(w):
    return int(w * 32768 + 0.5)


def merge15(a, b, w):
    """std.Merge(a, b, w) on uint8 arrays (stand-in)"""
    a, b = np.asarray(a).astype(np.int32), np.asarray(b).astype(np.int32)
    return (a + (((b - a) * w15(w) + 16384) >> 15)).astype(np.uint8)


def expr_mul(v, gain):
    """std.Expr "x g *" on uint8 samples (stand-in)"""
    p = np.asarray(v).astype(np.float32) * np.float32(gain)
    return np.clip(np.rint(p), 0, 255).astype(np.uint8)


# ---- the GPU path ------------------------------------------------------------------------------------------------------------------------------------------
def check_args(shape, method, gridsize=GRID):
    """the refusals, before anything touches the GPU.  Imported lazily: havc.py imports this module."""
    from .havc import HAVCError
    if method == 4:
        raise NotImplementedError("rgb_equalizer(method=4): ScaleAbs + LUT is the timecube plugin (vs_timecube) applied with LUT files: not in this harness")
    if method not in (0, 1, 2, 3):
        raise NotImplementedError("rgb_equalizer(method=5): Multi-Scale Retinex is the Retinex.dll MSRCP plugin (vs_retinex): not in this harness")
    if gridsize != GRID:
        raise HAVCError(f"rgb_equalizer: gridsize = {gridsize}: only the reference's own 8 x 8 grid is supported")
    if len(shape) not in (3, 4) or shape[-1] != 3:
        raise HAVCError("HAVC: only RGB24 clips (uint8 [n, h, w, 3]) are supported")
    if shape[-2] < GRID or shape[-3] < GRID:
        raise HAVCError(f"rgb_equalizer: frames of {shape[-3]} x {shape[-2]} are smaller than the 8 x 8 tile grid")


def rgb_equalizer_np(ctx, clip, method=0, clip_limit=1.0, gridsize=8, strength=0.5, weight3=0.3, luma_blend=True, range_tv=True, *, balance=None,
                     lut_in=None, lut_out=None):
    """rgb_equalizer (havc_utils.py:836-1075) on a frame [h, w, 3] or a clip [n, h, w, 3], ndarray or DeviceImage -> the same kind and shape.
    balance = (strength, rgb_factor): rgb_balance (:1087-1145) in front, as HAVC_bw_tune has it.  lut_in / lut_out: 256-entry uint8 tables applied to every
    sample read / written (tv_in_table / tv_out_table for HAVC_bw_tune's range_tv).  ndarray: blocks; DeviceImage: only enqueues."""
    from . import _native as nat
    from .device import DeviceImage, is_device, operand_ptr
    if not is_device(clip):
        clip = np.ascontiguousarray(clip, dtype=np.uint8)
    check_args(clip.shape, method, gridsize)
    shape = tuple(clip.shape)
    n = shape[0] if len(shape) == 4 else 1
    p = nat.EqualizeParams(width=shape[-2], height=shape[-3], n_frames=n, method=int(method), luma_blend=1 if luma_blend else 0,
                           range_tv=1 if range_tv else 0, clip_limit=float(clip_limit), weight=min(max(1.0 - strength, 0.0), 1.0),      # :866
                           weight3=float(weight3))
    if balance is not None:
        p.balance, p.balance_weight = 1, min(max(1.0 - balance[0], 0.0), 1.0)                     # :1100
        for k in range(3):
            p.rgb_factor[k] = float(balance[1][k])
    for name, tab in (("lut_in", lut_in), ("lut_out", lut_out)):
        tab = np.arange(256, dtype=np.uint8) if tab is None else np.ascontiguousarray(tab, dtype=np.uint8)
        if tab.shape != (256,):
            raise ValueError(f"{name}: 256 uint8 entries expected")
        C.memmove(getattr(p, name), tab.ctypes.data, 256)
    out = DeviceImage(ctx, shape) if is_device(clip) else np.empty(shape, np.uint8)
    nat.check(ctx.lib.havc_equalize_clip(ctx.h, operand_ptr(clip), operand_ptr(out), C.byref(p)), ctx.h)
    return out
