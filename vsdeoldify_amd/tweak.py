"""The three hand corrections a user reaches for after colouring, without VapourSynth: HAVC_tweak (vsdeoldify/__init__.py:1377-1408 -> vs_tweak,
vsslib/vsfilters.py:753-850), HAVC_adjust_rgb (:1342-1374 -> vs_rgb_normalize, vsfilters.py:1013-1038, vs_simple_merge, adjust_rgb, havc_utils.py:664-749)
and HAVC_rgb_denoise (:924-944 -> rgb_denoise, havc_utils.py:752-773).

PINNED -- the reference's Python, restated here as PLANS: `tweak_plan`, `adjust_plan`, `normalize_gains`, `denoise_calls` derive every number and every
string the reference hands to VapourSynth's native filters, and the ordered list of those calls.  tests/golden/tweak.npz records the same by EXECUTING the
reference against a recording vapoursynth stand-in (tools/gen_golden_tweak.py); tests/test_tweak_host.py compares them case by case: the gamma handed to
std.Levels, the arguments of both resize.Bicubic, the two expression strings, the 256-entry luma list (with the -1 < bright < 1 scaling and the truncating
int()), the affine expressions and per-plane gammas of adjust_rgb, the un-rounded gains of vs_rgb_normalize, rgb_denoise's calls.

UNPINNED -- the native filters themselves (zimg's resize, std.Levels / Expr / Lut / Merge / PlaneStats) cannot be executed where the fixtures are made.
tests/tweak_util.py restates them in numpy and is THE DEFINITION for this project; its docstring lists every assumption about zimg (Mitchell b = c = 1/3,
vertical pass first, centred vertical and left horizontal chroma siting, mirrored edges, round half to even, Floyd - Steinberg error diffusion); the
kernels (csrc/tweak.hip) equal it byte for byte.

A quirk that is kept: is_limited_range (havc_utils.py:616-629) answers True for a clip WITHOUT a range prop, because convert_format_RGB24 has just flagged
such an RGB24 clip as limited (:78-82).  An array carries no props, so HAVC_adjust_rgb takes a keyword-only color_range: None and "limited" take the limited
branch (a bias is scaled by 256 / 235 and checked against +-235), "full" the other (256 / 255, +-255).

`tweak_np`, `adjust_rgb_np`, `rgb_to_yuv420_np`, `yuv420_to_rgb_np` run on a frame [h, w, 3] or a clip [n, h, w, 3], ndarray or DeviceImage; a DeviceImage in
gives a DeviceImage out and the call only enqueues.  The vs_tweak refusals inside the other entry points (HAVC_colorizer's sat / hue, render_vivid, ddtweak) stay as
they are: routing them here is a separate decision.  HAVC_stabilizer(stab=True) is built on the two conversions (chroma_stab.py).
"""
import ctypes as C
import math

import numpy as np

MAX_SIDE = 4096                                                # csrc/kernels.h TW_MAX_SIDE: the back kernel keeps one error row per channel in LDS
BICUBIC_TO_YUV = dict(format="YUV420P8", matrix_s="709", range_s="full")                                          # vsfilters.py:790
BICUBIC_TO_RGB = dict(format="RGB24", matrix_in_s="709", range_s="full", dither_type="error_diffusion")           # :848


def _err(msg):
    from .havc import HAVCError
    return HAVCError(msg)


# ---- std.Levels(gamma=) (stand-in) ----------------------------------------------------------------------------------------------------------------------------
def gamma_table(gamma):
    """int(pow(v / 255, 1 / gamma) * 255 + 0.5) in float64; gamma 0 (adjust_rgb allows it) is the limit: everything below 255 goes to 0"""
    inv = math.inf if gamma == 0 else 1.0 / gamma
    return np.array([int(math.pow(v / 255, inv) * 255 + 0.5) for v in range(256)], np.uint8)


# ---- vs_tweak's Python -----------------------------------------------------------------------------------------------------------------------------------------
def tweak_plan(hue=0, sat=1, bright=0, cont=1, gamma=1):
    """vsfilters.py:781-848 -> None (the clip comes back as it is) or dict(gamma, hue_sat, exprs, luma_lut, calls): gamma = what std.Levels gets (None: not
    called), hue_sat = (hue_cos * sat, hue_sin * sat) as the float64 the reference formats into its strings, exprs = the two strings, luma_lut = the 256
    entries of std.Lut, calls = the native calls in order"""
    if hue == 0 and sat == 1 and bright == 0 and cont == 1 and gamma == 1:
        return None
    plan = dict(gamma=None, hue_sat=None, exprs=None, luma_lut=None, calls=[])
    if gamma != 1:
        plan["gamma"] = gamma
        plan["calls"].append(["std.Levels", dict(gamma=gamma)])
    plan["calls"].append(["resize.Bicubic", dict(BICUBIC_TO_YUV)])
    if -1.0 < bright < 1.0:
        bright = bright * 255.0
    if hue != 0 or sat != 1:
        rad = hue * math.pi / 180.0
        hue_sin, hue_cos = math.sin(rad), math.cos(rad)
        gray, chroma_min, chroma_max = 128, 0, 255
        expr_u = "x {} - {} * y {} - {} * + {} + {} max {} min".format(gray, hue_cos * sat, gray, hue_sin * sat, gray, chroma_min, chroma_max)
        expr_v = "y {} - {} * x {} - {} * - {} + {} max {} min".format(gray, hue_cos * sat, gray, hue_sin * sat, gray, chroma_min, chroma_max)
        plan["hue_sat"], plan["exprs"] = (hue_cos * sat, hue_sin * sat), [expr_u, expr_v]
        plan["calls"] += [["std.Expr", expr_u], ["std.Expr", expr_v]]
    if bright != 0 or cont != 1:
        luma_min, luma_max = 0, 255
        lut = []
        for i in range(256):
            val = int((i - luma_min) * cont + bright + luma_min + 0.5)
            lut.append(min(max(val, luma_min), luma_max))
        plan["luma_lut"] = lut
        plan["calls"].append(["std.Lut", dict(planes=0, lut=lut)])
    plan["calls"].append(["resize.Bicubic", dict(BICUBIC_TO_RGB)])
    return plan


# ---- HAVC_adjust_rgb's Python ----------------------------------------------------------------------------------------------------------------------------------
def normalize_gains(red, green, blue):
    """auto_white_adjust (vsfilters.py:1019-1033) from the three PlaneStatsAverage values -> the gains, float64, not rounded"""
    small_number = 0.000000001
    max_rgb = max(red, green, blue)
    red_corr = max_rgb / max(red, small_number)
    green_corr = max_rgb / max(green, small_number)
    blue_corr = max_rgb / max(blue, small_number)
    norm = max(blue, math.sqrt(red_corr * red_corr + green_corr * green_corr + blue_corr * blue_corr) / math.sqrt(3), small_number)
    return red_corr / norm, green_corr / norm, blue_corr / norm


def normalize_exprs(gains):
    return ['x ' + repr(g) + ' *' for g in gains]                                                 # :1034-1035


def adjust_plan(factor=(1.0, 1.0, 1.0), bias=(0, 0, 0), gamma=(1.0, 1.0, 1.0), color_range=None):
    """adjust_rgb (havc_utils.py:681-749) -> dict(gain, bias, gamma, exprs): the constants as std.Expr parses them out of the strings, the gamma per plane
    (None: std.Levels is not called), the three strings.  The refusals carry the reference's texts."""
    name = 'HAVC_adjust_rgb'
    if color_range not in (None, "limited", "full"):
        raise _err(name + ': color_range must be None, "limited" or "full"')
    r, g, b = factor[0], factor[1], factor[2]
    rb, gb, bb = bias[0], bias[1], bias[2]
    rg, gg, bg = gamma[0], gamma[1], gamma[2]
    limited = color_range != "full"                                                               # is_limited_range: no prop = limited (module docstring)
    lim, flag = (235, "limited") if limited else (255, "full")
    for n, v in (("rb", rb), ("gb", gb), ("bb", bb)):
        if v > lim or v < -lim:
            raise _err(f'{name}: source is flagged as "{flag}" but {n} is out of range [-{lim},{lim}]!')
    for n, v in (("rg", rg), ("gg", gg), ("bg", bg)):
        if v < 0:
            raise _err(f'{name}: {n} needs to be >= 0!')
    size, max_val = 256, lim
    rb, gb, bb = [size / max_val * v for v in (rb, gb, bb)]                                       # :739: size (256) never equals maxVal
    exprs = [f"x {r} * {rb} +", f"x {g} * {gb} +", f"x {b} * {bb} +"]
    gain, off = [float(e.split()[1]) for e in exprs], [float(e.split()[3]) for e in exprs]
    return dict(gain=gain, bias=off, gamma=[None if v == 1 else v for v in (rg, gg, bg)], exprs=exprs)


def adjust_calls(strength, plan, averages=None):
    """the native calls of HAVC_adjust_rgb in order; averages: the three PlaneStatsAverage values the frame function sees"""
    calls = []
    if strength == 1 or 0 < strength < 1:
        calls.append(["std.Expr", normalize_exprs(normalize_gains(*averages))])
        if strength != 1:
            calls.append(["std.Merge", dict(weight=strength)])
    calls.append(["std.Expr", list(plan["exprs"])])
    calls += [["std.Levels", dict(plane=p, gamma=g)] for p, g in enumerate(plan["gamma"]) if g is not None]
    return calls


def denoise_calls(denoise_levels=(0.4, 0.3), rgb_factors=(0.95, 1.05, 1.01)):
    """rgb_denoise (havc_utils.py:752-773): the calls in order"""
    return [["std.Levels", dict(min_in=0, max_in=255, min_out=16, max_out=235)],
            ["resize.Bicubic", dict(format="RGB24", matrix_in_s="709", range_in_s="full", range_s="limited")],
            ["rgb_balance", dict(strength=denoise_levels[0], rgb_factor=[rgb_factors[0], rgb_factors[1], rgb_factors[2]])],
            ["rgb_equalizer", dict(method=0, strength=denoise_levels[1], luma_blend=False, range_tv=True)],
            ["std.Levels", dict(min_in=16, max_in=235, min_out=0, max_out=255)],
            ["resize.Bicubic", dict(format="RGB24", matrix_in_s="709", range_in_s="limited", range_s="full")]]


def adjust_tables(chan_sums, n_pixels, strength, plan):
    """the three 256-entry tables HAVC_adjust_rgb comes to for a frame with these channel sums -- what adjust_tables_kernel composes on the device:
    normalise, std.Merge by strength, the affine expression, gamma"""
    from . import equalize as EQ
    v = np.arange(256, dtype=np.uint8)
    normalise = strength == 1 or 0 < strength < 1
    gains = normalize_gains(*[EQ.plane_average(s, n_pixels) for s in chan_sums]) if normalise else None
    out = np.empty((3, 256), np.uint8)
    for c in range(3):
        s = v
        if normalise:
            s = EQ.expr_mul(v, gains[c])
            if strength != 1:
                s = EQ.merge15(v, s, strength)
        p = s.astype(np.float32) * np.float32(plan["gain"][c]) + np.float32(plan["bias"][c])
        s = np.clip(np.rint(p), 0, 255).astype(np.uint8)
        out[c] = s if plan["gamma"][c] is None else gamma_table(plan["gamma"][c])[s]
    return out


def adjust_frame_params(chan_sums, n_pixels):
    """what the library makes of a frame's channel sums (havc_adjust_frame_params: the kernels' C++ on the host, no GPU) -> the three gains"""
    from . import _native as nat
    out = (C.c_double * 3)()
    ch = (C.c_int64 * 3)(*[int(v) for v in chan_sums])
    if nat.load().havc_adjust_frame_params(ch, int(n_pixels), out) != 0:
        raise ValueError("havc_adjust_frame_params: bad arguments")
    return tuple(out)


def native_weights():
    """havc_tweak_weights: (down_v[8], down_h[8], up_v[2][4], up_h[2][4]) as float32 arrays"""
    from . import _native as nat
    out = np.empty(32, np.float32)
    if nat.load().havc_tweak_weights(nat.as_ptr(out)) != 0:
        raise ValueError("havc_tweak_weights")
    return out[:8], out[8:16], out[16:24].reshape(2, 4), out[24:].reshape(2, 4)


# ---- the GPU path ------------------------------------------------------------------------------------------------------------------------------------------
def check_clip(shape, dtype, name, even):
    """the refusals every entry shares, before anything touches the GPU"""
    if len(shape) not in (3, 4) or shape[-1] != 3 or np.dtype(dtype) != np.uint8 or min(shape) < 1:
        raise _err("HAVC: only RGB24 clips (uint8 [n, h, w, 3]) are supported")
    if even:
        h, w = shape[-3], shape[-2]
        if h % 2 or w % 2:
            raise _err(f"{name}: a frame of {w} x {h} cannot be YUV420P8: width and height must be even (VapourSynth refuses it too)")
        if h > MAX_SIDE or w > MAX_SIDE:
            raise _err(f"{name}: frames of {w} x {h} are larger than {MAX_SIDE} x {MAX_SIDE}")


def _prepare(clip, name, even):
    from .device import is_device
    if not is_device(clip):
        clip = np.asarray(clip)
    check_clip(tuple(clip.shape), np.uint8 if is_device(clip) else clip.dtype, name, even)
    if not is_device(clip):
        clip = np.ascontiguousarray(clip, dtype=np.uint8)
    shape = tuple(clip.shape)
    return clip, shape, (shape[0] if len(shape) == 4 else 1)


def tweak_np(ctx, clip, plan, chunk_frames=0):
    """vs_tweak with a plan of tweak_plan (None: the clip itself) through havc_tweak_clip: two launches per chunk of frames"""
    from . import _native as nat
    from .device import DeviceImage, is_device, operand_ptr
    clip, shape, n = _prepare(clip, "HAVC_tweak", True)
    if plan is None:
        return clip
    p = nat.TweakParams(width=shape[-2], height=shape[-3], n_frames=n, chunk_frames=int(chunk_frames))
    if plan["gamma"] is not None:
        p.has_gamma = 1
        C.memmove(p.gamma_lut, gamma_table(plan["gamma"]).ctypes.data, 256)
    if plan["hue_sat"] is not None:
        p.has_hue_sat, p.hue_c, p.hue_s = 1, float(plan["hue_sat"][0]), float(plan["hue_sat"][1])
    if plan["luma_lut"] is not None:
        p.has_luma = 1
        C.memmove(p.luma_lut, np.asarray(plan["luma_lut"], np.uint8).ctypes.data, 256)
    out = DeviceImage(ctx, shape) if is_device(clip) else np.empty(shape, np.uint8)
    nat.check(ctx.lib.havc_tweak_clip(ctx.h, operand_ptr(clip), operand_ptr(out), C.byref(p)), ctx.h)
    return out


def rgb_to_yuv420_np(ctx, clip):
    """havc_rgb_to_yuv420: RGB24 (ndarray or DeviceImage) -> (y, u, v) ndarrays, full range BT.709.  (The C entry takes device planes too; a DeviceImage
    is an RGB container, so this wrapper hands the planes out on the host.)"""
    from . import _native as nat
    from .device import operand_ptr
    clip, shape, n = _prepare(clip, "rgb_to_yuv420", True)
    lead, h, w = shape[:-3], shape[-3], shape[-2]
    y, u, v = np.empty(lead + (h, w), np.uint8), np.empty(lead + (h // 2, w // 2), np.uint8), np.empty(lead + (h // 2, w // 2), np.uint8)
    nat.check(ctx.lib.havc_rgb_to_yuv420(ctx.h, operand_ptr(clip), nat.as_ptr(y), nat.as_ptr(u), nat.as_ptr(v), w, h, n), ctx.h)
    return y, u, v


def yuv420_to_rgb_np(ctx, y, u, v, device=False):
    """havc_yuv420_to_rgb: ndarray planes [h, w] / [h / 2, w / 2] (or with a leading n) -> RGB24 with error diffusion, an ndarray or (device=True) a
    DeviceImage"""
    from . import _native as nat
    from .device import DeviceImage, operand_ptr
    y, u, v = (np.ascontiguousarray(p, dtype=np.uint8) for p in (y, u, v))
    ys = tuple(y.shape)
    if len(ys) not in (2, 3) or min(ys) < 1 or ys[-1] % 2 or ys[-2] % 2 or u.shape != ys[:-2] + (ys[-2] // 2, ys[-1] // 2) or v.shape != u.shape:
        raise _err("yuv420_to_rgb: y must be [n, h, w] or [h, w] with even h and w, u and v half its size")
    if max(ys[-2:]) > MAX_SIDE:
        raise _err(f"yuv420_to_rgb: frames larger than {MAX_SIDE} x {MAX_SIDE}")
    shape = ys + (3,)
    out = DeviceImage(ctx, shape) if device else np.empty(shape, np.uint8)
    nat.check(ctx.lib.havc_yuv420_to_rgb(ctx.h, nat.as_ptr(y), nat.as_ptr(u), nat.as_ptr(v), operand_ptr(out), ys[-1], ys[-2], ys[0] if len(ys) == 3 else 1),
              ctx.h)
    return out


def adjust_rgb_np(ctx, clip, strength, plan):
    """HAVC_adjust_rgb with a plan of adjust_plan through havc_adjust_rgb_clip: the channel sums (0 < strength <= 1), the tables, one pass"""
    from . import _native as nat
    from .device import DeviceImage, is_device, operand_ptr
    clip, shape, n = _prepare(clip, "HAVC_adjust_rgb", False)
    p = nat.AdjustParams(width=shape[-2], height=shape[-3], n_frames=n)
    if strength == 1:
        p.normalize = 1
    elif 0 < strength < 1:
        p.normalize, p.strength = 2, float(strength)
    for c in range(3):
        p.gain[c], p.bias[c] = plan["gain"][c], plan["bias"][c]                                  # ctypes rounds to float32: std.Expr's constants
        tab = np.arange(256, dtype=np.uint8) if plan["gamma"][c] is None else gamma_table(plan["gamma"][c])
        C.memmove(p.gamma_lut[c], tab.ctypes.data, 256)
    out = DeviceImage(ctx, shape) if is_device(clip) else np.empty(shape, np.uint8)
    nat.check(ctx.lib.havc_adjust_rgb_clip(ctx.h, operand_ptr(clip), operand_ptr(out), C.byref(p)), ctx.h)
    return out
