"""Multi-scale Retinex of clips without VapourSynth and without the Retinex plugin: HAVC_retinex (vsdeoldify/__init__.py:1073-1101) -> vs_retinex ->
vs_retinex_fast (vsslib/vsretinex.py:25-88).

`retinex_np` runs it on a clip uint8 [n, h, w, 3] (ndarray or DeviceImage) through `havc_retinex_clip` (csrc/retinex.hip): per chunk of frames the sum of
cv2's Y, the recursive Gaussians of every sigma (rows through LDS tiles, then columns), the MSR product and its log, the frame's extremes, a 4096-bin
histogram, the percentile stretch, the hue-preserving gain, the gate and the blend -- seven launches that hand everything on in device memory, nothing in
between on the host.  A DeviceImage in gives a DeviceImage out and the call only enqueues.

PINNED -- the reference's Python around the plugin, restated here (`frame_rule`, `plugin_args`) and pinned by tests/golden/retinex.npz, which
tools/gen_golden_retinex.py makes by executing the reference's HAVC_retinex -> vs_retinex -> vs_retinex_fast with its selector body filter_retinex,
get_image_luma and image_luma_blend with real Pillow: f_luma from the INPUT frame (with range_tv_in max(round(mean(Y) / 235, 6) - 0.07, 0), else
round(mean(Y) / 255, 6)), the gate luma_dark <= f_luma <= luma_bright (a gated-out frame is the input frame, whatever range_tv_out is), with blend
image_luma_blend(img, img_new, f_luma, 0.40, 0.90, 0.25, 3.0), and the arguments the plugin gets: sigma = sigmas, lower_thr = upper_thr = 0.001,
fulls = range_tv_in, fulld = range_tv_out, chroma_protect = 1.2.  (The reference's docstring contradicts itself about which value of range_tv_in means
which range; the code is mirrored, not the docstring.)  `frame_params` returns what the library computes for the same inputs (the C++ the kernels run,
compiled for the host).

UNPINNED -- the plugin itself (core.retinex.MSRCP, Retinex.dll) is not in the reference tree and cannot be executed where the fixtures are made; in the
fixture its output frame is a prescribed INPUT.  Its pixel work is restated from the published algorithm, MSRCP of Petro / Sbert / Morel ("Multiscale
Retinex", IPOL 2014), with the Young - van Vliet recursive Gaussian the plugin uses.  tests/retinex_util.py is that restatement in numpy and THE
DEFINITION for this project (include/havc_mi355.h has it in prose): I = (R + G + B - 3 sF) / (3 sR); per sigma a forward and a backward sweep over every
row, then over every column, each started from the line's first value; P = product of (I / g + 1); O = log(P) / n_sigmas; a 4096-bin histogram between
the frame's extremes, cut where the running count from either end first exceeds int(n_pixels * 0.001 + 0.5); gain = O' / I, capped so that the largest
channel stays inside the source range (MSRCP's colour preservation); the range conversion into the output sample.  chroma_protect does not enter: it belongs
to the plugin's YUV path, and the reference hands the plugin RGB.  Everything is float64 in a stated order without FMA; the only step that is not
bit-defined is `log` (the device's and numpy's may differ in the last place, which can move a byte in a million by one).
A frame with a sample below 16 under fulls = False can make I / g + 1 <= 0 and its logarithm undefined; the restatement and the kernels then disagree on
nothing in particular -- such a frame has no defined result.

Refused: chroma_resize=True (the zimg round trip inside convert_format_RGB24), non-RGB24 shapes, no sigma or more than 8, a sigma outside [0.5, 10000].
rgb_equalizer(method=5), HAVC_bw_tune(bw_method=5) and ddtweak's retinex keep raising: routing them here is a later change.
"""
import ctypes as C
import math

import numpy as np

from . import equalize

DEF_RETINEX_DARK, DEF_RETINEX_BRIGHT = 0.20, 0.80              # vsslib/constants.py:26-27
BLEND = (0.40, 0.90, 0.25, 3.0)                                # vsretinex.py:80: luma_limit, alpha, min_w, decay of image_luma_blend
LOWER_THR = UPPER_THR = 0.001                                  # vsretinex.py:58
CHROMA_PROTECT = 1.200
MAX_SIGMAS, SIGMA_MIN, SIGMA_MAX = 8, 0.5, 10000.0


# ---- the reference's Python around the plugin ------------------------------------------------------------------------------------------------------------
def frame_rule(sum_y, n_pixels, luma_dark=DEF_RETINEX_DARK, luma_bright=DEF_RETINEX_BRIGHT, range_tv=True, blend=False):
    """filter_retinex (vsretinex.py:64-84) from the integer sum of cv2's Y of the input frame -> (f_luma, gate, weight); weight None = the plugin's frame as
    it is"""
    luma = equalize.f_luma(sum_y, n_pixels, range_tv)
    gate = bool(luma_dark <= luma <= luma_bright)
    return luma, gate, (equalize.blend_weight(luma, *BLEND) if blend and gate else None)


def plugin_args(sigmas, range_tv_in, range_tv_out):
    """what vs_retinex_fast hands to core.retinex.MSRCP (vsretinex.py:58-59)"""
    return dict(sigma=sigmas, lower_thr=LOWER_THR, upper_thr=UPPER_THR, fulls=range_tv_in, fulld=range_tv_out, chroma_protect=CHROMA_PROTECT)


def frame_params(sum_y, n_pixels, luma_dark=DEF_RETINEX_DARK, luma_bright=DEF_RETINEX_BRIGHT, range_tv=True, blend=False):
    """what the library makes of the same numbers (havc_retinex_frame_params: the kernels' C++ on the host, no GPU) -> (f_luma, gate, weight)"""
    from . import _native as nat
    out = (C.c_double * 3)()
    if nat.load().havc_retinex_frame_params(int(sum_y), int(n_pixels), 1 if range_tv else 0, float(luma_dark), float(luma_bright), 1 if blend else 0, out) != 0:
        raise ValueError("havc_retinex_frame_params: bad arguments")
    return out[0], bool(out[1]), (None if out[2] < 0 or not out[1] else float(np.float32(out[2])))


# ---- the stand-in's host arithmetic ---------------------------------------------------------------------------------------------------------------------
def coefficients(sigma):
    """Young - van Vliet: (B, B1, B2, B3) of one sigma in float64, every product and sum in the order csrc/retinex_ops.h writes them"""
    sigma = float(sigma)
    if sigma >= 2.5:
        q = 0.98711 * sigma - 0.96330
    else:
        q = 3.97156 - 4.14554 * math.sqrt(1.0 - 0.26891 * sigma)
    q2 = q * q
    q3 = q2 * q
    a1, a2, a3 = 2.44413 * q, 1.4281 * q2, 0.422205 * q3
    b0 = ((1.57825 + a1) + a2) + a3
    c2, c3 = 2.85619 * q2, 1.26661 * q3
    b1 = (a1 + c2) + c3
    b2 = -(a2 + c3)
    b3 = a3
    return 1.0 - ((b1 + b2) + b3) / b0, b1 / b0, b2 / b0, b3 / b0


def native_coefficients(sigma):
    """havc_retinex_coefficients: the same on the library's side"""
    from . import _native as nat
    out = (C.c_double * 4)()
    if nat.load().havc_retinex_coefficients(float(sigma), out) != 0:
        raise ValueError("havc_retinex_coefficients: sigma outside [0.5, 10000]")
    return tuple(out)


# ---- the GPU path ------------------------------------------------------------------------------------------------------------------------------------------
def check_args(shape, sigmas, chroma_resize=False, dtype=np.uint8):
    """the refusals, before anything touches the GPU -> the sigmas as floats.  Imported lazily: havc.py imports this module."""
    from .havc import HAVCError
    if chroma_resize:
        raise NotImplementedError("HAVC_retinex(chroma_resize=True): the downscale is a zimg round trip inside convert_format_RGB24 / restore_format "
                                  "(havc_utils.py:57-140): not in this harness")
    if len(shape) not in (3, 4) or shape[-1] != 3 or np.dtype(dtype) != np.uint8 or min(shape) < 1:
        raise HAVCError("HAVC: only RGB24 clips (uint8 [n, h, w, 3]) are supported")
    try:
        sig = [float(s) for s in sigmas]
    except TypeError:
        raise HAVCError("HAVC_retinex: sigmas must be a sequence of numbers") from None
    if not 1 <= len(sig) <= MAX_SIGMAS:
        raise HAVCError(f"HAVC_retinex: {len(sig)} sigmas: between 1 and {MAX_SIGMAS} are supported")
    for s in sig:
        if not SIGMA_MIN <= s <= SIGMA_MAX:
            raise HAVCError(f"HAVC_retinex: sigma = {s}: outside [{SIGMA_MIN}, {SIGMA_MAX}]")
    return sig


def retinex_np(ctx, clip, sigma=(25, 80, 250), lower_thr=LOWER_THR, upper_thr=UPPER_THR, fulls=True, fulld=True, chroma_protect=CHROMA_PROTECT, *,
               luma_dark=DEF_RETINEX_DARK, luma_bright=DEF_RETINEX_BRIGHT, range_tv=True, blend=False, chunk_frames=0, tap=False):
    """vs_retinex_fast on a frame [h, w, 3] or a clip [n, h, w, 3], ndarray or DeviceImage -> the same kind and shape.  The positional arguments are the
    plugin's, under the plugin's names (plugin_args: `sigma` is HAVC_retinex's `sigmas`); the thresholds and chroma_protect are fixed by the reference's call and other values are refused.  tap=True (tests; host
    clips): -> (out, planes float64 [n, n_sigmas + 1, h, w]: the Gaussian planes, then the MSR product).  ndarray: blocks; DeviceImage: only enqueues."""
    from . import _native as nat
    from .device import DeviceImage, is_device, operand_ptr
    from .havc import HAVCError
    if not is_device(clip):
        clip = np.asarray(clip)
    sig = check_args(tuple(clip.shape), sigma, False, np.uint8 if is_device(clip) else clip.dtype)
    if lower_thr != LOWER_THR or upper_thr != UPPER_THR or chroma_protect != CHROMA_PROTECT:
        raise HAVCError("retinex_np: lower_thr / upper_thr / chroma_protect are fixed at the reference's 0.001 / 0.001 / 1.2")
    if not is_device(clip):
        clip = np.ascontiguousarray(clip, dtype=np.uint8)
    shape = tuple(clip.shape)
    n = shape[0] if len(shape) == 4 else 1
    p = nat.RetinexParams(width=shape[-2], height=shape[-3], n_frames=n, n_sigmas=len(sig), luma_dark=float(luma_dark), luma_bright=float(luma_bright),
                          fulls=1 if fulls else 0, fulld=1 if fulld else 0, range_tv=1 if range_tv else 0, blend=1 if blend else 0,
                          chunk_frames=int(chunk_frames))
    for k, s in enumerate(sig):
        p.sigma[k] = s
    out = DeviceImage(ctx, shape) if is_device(clip) else np.empty(shape, np.uint8)
    planes = np.empty((n, len(sig) + 1, shape[-3], shape[-2]), np.float64) if tap else None
    nat.check(ctx.lib.havc_retinex_clip(ctx.h, operand_ptr(clip), operand_ptr(out), C.byref(p), nat.as_ptr(planes) if tap else None), ctx.h)
    return (out, planes) if tap else out
