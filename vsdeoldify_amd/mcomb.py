"""Per-frame bodies of the HAVC model-combination methods (vsdeoldify/vsslib/mcomb.py `merge_frame` selectors), on
uint8 HWC frames, backed by the HIP filters.  The VapourSynth wrappers (ModifyFrame plumbing, scene-change
passthrough) stay in the reference; these are the functions they would call once per frame.

  method 2  SimpleMerge               mcomb.py:206-223   Image.blend(a, b, w)
  method 3  ConstrainedChromaMerge    mcomb.py:333-367   chroma_stabilizer (+ dark-frame red fix)
  method 4  LumaMaskedMerge           mcomb.py:238-271   (w_)image_luma_merge + weighted merge
  method 5  AdaptiveLumaMerge         mcomb.py:289-314   frame-mean luma -> weight -> blend
  method 7  ChromaBoundAdaptiveMerge  mcomb.py:370-437   chroma_stabilizer_adaptive (+ red fix)
  method 6  ChromaRetentionMerge      mcomb.py:450-516   restore_color_gradient (+ blend); the optional Spline64 round
                                                         trip of chroma_resize stays with the caller (zimg)
`chroma_retention_merge_clip` is the exception: ChromaRetentionMerge as a whole on a CLIP -- both selectors (gradient and binary mask) with their frame-level
decisions made on the device (havc_recover_color_clip: two launches per clip), the chroma_resize round trip through the library's Spline64 and the closing merge.
The dark-frame "red fix" (frame luma <= 0.3, mcomb.py:350-361) = image_tweak (ImageEnhance.Color + hue-range mask) merged
back through w_image_luma_merge.
"""
import numpy as np

from . import imfilters as F
from .device import is_device
from .render import get_context


def _img(x):
    return x if is_device(x) else np.asarray(x)

DEF_STANDARD_DARK, DEF_STANDARD_BRIGHT = 0.22, 0.78        # vsslib/constants.py:28-29


def simple_merge(a, b, weight=0.5, device_index=0):
    if weight == 0.0:
        return _img(a)
    if weight == 1.0:
        return _img(b)
    return F.blend_np(get_context(device_index), a, b, weight)


def _red_fix(ctx, img_stab):
    """mcomb.py:350-361 / 409-420."""
    luma = round(F.image_luma_np(ctx, img_stab) / 255, 6)
    if luma > 0.3:
        return img_stab
    if luma > 0.1:
        dark_luma, white_luma, sat = (0.2, 0.3, 0.9) if luma > 0.2 else (0.1, 0.2, 0.8)        # literals, as the reference writes them
        dark = F.image_tweak_np(ctx, img_stab, sat=sat, hue_range="280:360,0:30")
        max_white = round(white_luma * 255)                                  # w_image_luma_merge (imfilters.py:80-100)
        tresh = min(round(dark_luma * 255), max_white - 10)
        return F.luma_merge_np(ctx, dark, img_stab, 1, tresh, round(1 / (max_white - tresh), 3))
    return F.image_tweak_np(ctx, img_stab, sat=0.7)


def constrained_chroma_merge(a, b, clipb_weight=0.5, chroma_threshold=0.2, red_fix=True, device_index=0):
    ctx = get_context(device_index)
    img_stab = F.chroma_stabilizer_np(ctx, a, b, chroma_threshold, clipb_weight)
    return _red_fix(ctx, img_stab) if red_fix else img_stab


def chroma_bound_adaptive_merge(a, b, red_fix=True, base_tol=14, max_extra=18, clipb_weight=0.5, device_index=0):
    ctx = get_context(device_index)
    img_stab = F.chroma_stabilizer_adaptive_np(ctx, a, b, base_tol, max_extra, clipb_weight)
    return _red_fix(ctx, img_stab) if red_fix else img_stab


def luma_masked_merge(a, b, c=None, luma_mask_limit=0.4, luma_white_limit=0.7, clipm_weight=0.5, device_index=0):
    """a = clipa frame, b = clipb frame, c = de-saturated clipa frame (== a when luma_mask_sat >= 1)."""
    ctx = get_context(device_index)
    c = a if c is None else c
    if luma_mask_limit == luma_white_limit:
        masked = F.image_luma_merge_np(ctx, _img(c), _img(b), luma_mask_limit)
    else:
        masked = F.w_image_luma_merge_np(ctx, _img(c), _img(b), luma_mask_limit, luma_white_limit)
    return simple_merge(a, masked, clipm_weight, device_index) if clipm_weight < 1.0 else masked


def adaptive_luma_merge(a, b, luma_threshold=0.6, alpha=1.0, clipb_weight=0.5, min_weight=0.15, device_index=0):
    ctx = get_context(device_index)
    luma = round(F.image_luma_np(ctx, b) / 255, 6)
    w = max(clipb_weight * pow(luma / luma_threshold, alpha), min_weight) if luma < luma_threshold else clipb_weight
    return F.blend_np(ctx, a, b, w)


def chroma_retention_frame(a, b, sat=0.8, tht=30, mask_weight=0.0, alpha=2.0, return_mask=False, algo=0, device_index=0):
    """The per-frame selector of ChromaRetentionMerge (mcomb.py:450-516 -> vs_sc_recover_gradient_color, vsfilters.py:391-412):
    a = frame to repair (deoldify), b = colour donor (ddcolor).  Frames darker / brighter than the standard luma band get
    weight <= -0.5 and alpha >= 4 (vsfilters.py:403-409).  The clip-level steps around it -- the optional Spline64 round trip
    (chroma_resize) and the closing std.Merge(clip_a, restored, clipb_weight) -- are VapourSynth core filters and stay there."""
    ctx = get_context(device_index)
    alpha = max(min(alpha, 10.0), 1.0)                                       # DEF_MIN/MAX_COLOR_ALPHA, constants.py:80-81
    luma = round(F.image_luma_np(ctx, a) / 255, 6)
    if not (DEF_STANDARD_DARK <= luma <= DEF_STANDARD_BRIGHT):
        mask_weight = min(mask_weight, -0.5)
        alpha = max(alpha, 4.0)
    return F.restore_color_gradient_np(ctx, b, a, sat, tht, mask_weight, alpha, return_mask, algo)


def recover_size(width):
    """mcomb.py:482-484: the square size chroma_resize works at, or None when it would not shrink the clip (`if frame_size < clip_luma.width`).  rf is capped
    at 48 here; HAVC_merge's own rule (__init__.py:2663-2667) caps it at 32."""
    import math
    rf = min(max(math.trunc(0.4 * width / 16), 16), 48)
    fs = min(rf * 16, width)
    return fs if fs < width else None


def recover_color_clip(ctx, gray, color, sat=0.8, tht=30, weight=0.0, alpha=2.0, return_mask=False, binary_mask=False, algo=0, first_frame=0):
    """havc_recover_color_clip on two clips [n, h, w, 3] of one kind (ndarray: blocks; DeviceImage: only enqueues): the selectors of ChromaRetentionMerge,
    vs_sc_recover_gradient_color / vs_sc_recover_clip_color, for every frame in two launches.  alpha is used as given."""
    import ctypes as C
    from . import _native as nat
    from .device import DeviceImage, operand_ptr
    dev = is_device(gray)
    if not dev:
        gray, color = np.ascontiguousarray(gray, dtype=np.uint8), np.ascontiguousarray(color, dtype=np.uint8)
    shape = tuple(gray.shape)
    if len(shape) != 4 or shape[3] != 3 or tuple(color.shape) != shape:
        raise ValueError("recover_color_clip: two clips [n, h, w, 3] of one shape expected")
    p = nat.RecoverParams(width=shape[2], height=shape[1], n_frames=shape[0], first_frame=int(first_frame), sat=float(sat), tht=int(tht), algo=int(algo),
                          weight=float(weight), alpha=float(alpha), binary_mask=1 if binary_mask else 0, return_mask=1 if return_mask else 0)
    out = DeviceImage(ctx, shape) if dev else np.empty(shape, np.uint8)
    nat.check(ctx.lib.havc_recover_color_clip(ctx.h, operand_ptr(gray), operand_ptr(color), operand_ptr(out), C.byref(p)), ctx.h)
    return out


def chroma_retention_merge_clip(a, b, sat=0.8, tht=30, clipb_weight=0.9, alpha=2.0, mask_weight=0.0, chroma_resize=True, return_mask=False,
                                binary_mask=False, algo=0, first_frame=0, device_index=0):
    """ChromaRetentionMerge (mcomb.py:450-516) on clips [n, h, w, 3], ndarray or DeviceImage (one of each: the ndarray is uploaded): a = clip to repair,
    b = colour donor.  The clip-level steps in the reference's order: alpha clamped to [1, 10]; with chroma_resize (and no return_mask) both clips through
    Spline64 to recover_size(W) squared when that is smaller than W; the selector for every frame (ONE havc_recover_color_clip call, frame-level decisions
    on the device); return_mask returns here; Spline64 back to W x H with the luma of a (vs_sc_recover_clip_luma, fused); vs_simple_merge(a, restored,
    clipb_weight).  No step reads a value back to the host: with DeviceImage operands the whole function only enqueues.  first_frame: clip index of frame 0
    (the binary selector hands frames below 15 on unchanged).  algo reaches the gradient selector (the reference's ChromaRetentionMerge drops it on the way)."""
    from .device import DeviceImage
    from .havc import spline64
    if len(a.shape) != 4 or a.shape[3] != 3 or tuple(b.shape) != tuple(a.shape):
        raise ValueError("chroma_retention_merge_clip: two clips [n, h, w, 3] of one shape expected")
    ctx = get_context(device_index)
    if is_device(a) != is_device(b):
        a = a if is_device(a) else DeviceImage.from_numpy(ctx, a)
        b = b if is_device(b) else DeviceImage.from_numpy(ctx, b)
    if not is_device(a):
        a, b = np.ascontiguousarray(a, dtype=np.uint8), np.ascontiguousarray(b, dtype=np.uint8)
    alpha = max(min(alpha, 10.0), 1.0)                                       # DEF_MIN/MAX_COLOR_ALPHA, constants.py:80-81
    h, w = a.shape[1], a.shape[2]
    fs = recover_size(w) if chroma_resize and not return_mask else None
    clip, clip_color = (a, b) if fs is None else (spline64(ctx, a, fs, fs), spline64(ctx, b, fs, fs))
    restored = recover_color_clip(ctx, clip, clip_color, sat, tht, mask_weight, alpha, return_mask, binary_mask, algo, first_frame)
    if return_mask:
        return restored
    if fs is not None:
        restored = spline64(ctx, restored, w, h, luma_from=a)
    if clipb_weight == 0:                                                    # vs_simple_merge, vsfilters.py:730-739
        return a
    if clipb_weight == 1:
        return restored
    rows = (lambda x: x.as_rows()) if is_device(a) else (lambda x: x.reshape((-1,) + x.shape[2:]))
    merged = simple_merge(rows(a), rows(restored), clipb_weight, device_index)
    return merged.reshaped(a.shape) if is_device(merged) else merged.reshape(a.shape)
