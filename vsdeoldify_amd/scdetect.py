"""Scene detection without VapourSynth: vsslib/vsscdect.py:44-350 on per-frame statistics the GPU takes of a clip in one pass.

The reference's detector is Python over two numbers per frame -- the mean of a small gray plane and std.PlaneStats' difference against the frame
`offset` frames before it.  `scene_stats` gets both for a whole clip from `havc_scene_stats` (csrc/scdetect.hip: exact integer sums, one launch, two
with normalisation); `scene_flags` is the sequential rest, a pure function of those numbers that needs no GPU:

    SceneDetect (vsscdect.py:44-87)                the early returns (no flags; the modulo rule of set_scene_change_freq) and the clamps of offset / min_length
    SceneDetection.SceneDetect (:200-238)          custom detector or plugin path, SSIM filter
    SceneDetectCustom.set_SCDetect (:288-342)      adaptive-ratio detector with its roundings, carried state and overrides -- pinned by tests/golden/scdetect.npz,
                                                   which tools/gen_golden_scdetect.py makes by executing the reference's own selector
    filter_black_white (:240-279)                  the luma filter on top of the plugin's flags -- pinned the same way

What stands in for VapourSynth native code here (it cannot be executed where the fixtures are made, so it is UNPINNED, like Spline64 and MaskedMerge in havc.py):
  * zimg's RGB -> GRAY8 (`resize.Bicubic(format=vs.GRAY8, matrix_s='709')`) -> Y = (cr * R + cg * G + cb * B + bias) >> 16 with BT.709 integer coefficients.
    The reference names no range and VapourSynth's default for non-RGB output is limited: LUMA_LIMITED (16..235; the coefficients sum to
    56284 = round(219 / 255 * 65536)) is the default.  LUMA_FULL exists because that assumption cannot be checked here.
  * `resize_min_HW` (vsresize.py:30-99; zimg Spline36 on the gray plane) -> the size arithmetic restated (`resize_min_hw`), the resampling done by the
    library's Spline64 on the RGB clip BEFORE the gray conversion (the reference converts first).
  * `misc.SCDetect` (the default path: threshold >= 0.10, offset 1) -> prev_n = diff(n - 1, n) > threshold with prev_0 = 1; next_n = prev_(n + 1) with
    next_last = 1.  What the plugin does at the first and last frame is not pinned.
  * std.PlaneStats' PlaneStatsDiff -> sad / (n_pixels * 255) in float64.
`SceneDetectFilter` (0 < sc_tht_filter < 1 or min_length > 1) needs skimage.metrics.structural_similarity and cv2.calcHist / compareHist, which do not
exist here: NotImplementedError, before anything is enqueued.
"""
import ctypes as C
import dataclasses

import numpy as np

DEF_THRESHOLD = 0.10                                   # vsslib/constants.py:60
DEF_THT_WHITE, DEF_THT_BLACK = 0.70, 0.10              # :24-25
DEF_THT_BLACK_MIN, DEF_THT_WHITE_MIN = 0.19, 0.70      # :43-44 (sc_clip_normalize's thresholds, and the "bright" band of the custom detector)
DEF_ADAPTIVE_RATIO_LO, DEF_ADAPTIVE_RATIO_MED = 1.02, 1.12     # :47-48
DEF_ADAPTIVE_RATIO_RF, DEF_ADAPTIVE_RATIO_VHI = 2.0, 15.0      # :50-51
DEF_SC_MIN_DISTANCE = 15                               # :63

LUMA_LIMITED = (11966, 40254, 4064, 16 * 65536 + 32768)        # BT.709, 16..235
LUMA_FULL = (13933, 46871, 4732, 32768)                        # BT.709, 0..255


@dataclasses.dataclass
class SceneInfo:
    """the frame props the reference's SceneDetect leaves on a clip (CopySCDetect's list, vsscdect.py:118-120), one array entry per frame"""
    scene_change_prev: np.ndarray      # _SceneChangePrev, int8
    scene_change_next: np.ndarray      # _SceneChangeNext, int8
    sc_luma: np.ndarray                # float64; 0.5 where the reference never sets it (the early returns; :204)
    sc_ratio: np.ndarray               # float64; 0 where the reference never sets it (:205)
    sc_threshold: float
    sc_frequency: int


def resize_min_hw(width, height, min_size=(512, 480)):
    """resize_min_HW's size arithmetic (vsresize.py:30-99) -> (width, height) of the clip the statistics are taken of: the short side at most 480
    (landscape) / 512 (portrait or square), the other side in proportion and even (rounded down for a landscape clip, up for a portrait one, as there)"""
    if height < width:
        if height > min_size[1]:
            tw = round(width * min_size[1] / height)
            if tw % 2 != 0:
                tw -= 1
            return tw, min_size[1]
        return width, height
    if width > min_size[0]:
        th = round(height * min_size[0] / width)
        if th % 2 != 0:
            th += 1
        return min_size[0], th
    return width, height


def norm_value(k, d):
    """frame_normalize on one value (vsutils.py:314-316): uint8(255 * ((y - min) / (max - min))) in float64 -- divide, multiply, truncate; k = y - min,
    d = max - min.  d == 0 is NaN there: 0 here."""
    if d <= 0:
        return 0
    return int(255.0 * (float(k) / float(d)))


def detect_branch(threshold, frequency, sc_tht_filter=0.0, min_length=1, tht_offset=1):
    """which path SceneDetect takes (vsscdect.py:50, 71, 81-82, 213-227): "none", "frequency", "custom" or "plugin"; the SSIM filter is refused"""
    if threshold == 0 and frequency == 0:
        return "none"
    if frequency == 1 or (threshold == 0 and frequency > 1):
        return "frequency"
    t_offset = min(max(tht_offset, 1), 25)
    m_length = min(max(min_length, 1), 25)
    if 0.0 < sc_tht_filter < 1.0 or m_length > 1:
        raise NotImplementedError("SceneDetect: the SSIM post-filter (0 < sc_tht_ssim < 1 or sc_min_int > 1: SceneDetectFilter) needs "
                                  "skimage.metrics.structural_similarity and cv2.calcHist / cv2.compareHist: not in this harness")
    if sc_tht_filter > 0.0 or threshold < 0.10 or t_offset > 1:
        return "custom"
    return "plugin"


def _luma(sum_y, n_pixels):
    """round(np.mean(f_y) / 255.0, 4) -- numpy's round on a float64 scalar, not Python's"""
    return float(round(np.float64(int(sum_y)) / np.float64(int(n_pixels)) / 255.0, 4))


def custom_detector(sum_y, sad, n_pixels, threshold, frequency, min_length, tht_white, tht_black):
    """SceneDetectCustom.set_SCDetect (vsscdect.py:288-342), frame by frame in order -> (prev, next, sc_luma, sc_ratio)"""
    n = len(sum_y)
    adaptive_ratio = DEF_ADAPTIVE_RATIO_MED if frequency > 0 else DEF_ADAPTIVE_RATIO_LO            # :75
    prev, nxt = np.zeros(n, np.int8), np.zeros(n, np.int8)
    luma, ratios = np.zeros(n, np.float64), np.zeros(n, np.float64)
    prev_diff, ref_luma, last_ref = 0, None, None
    for i in range(n):
        f_luma = _luma(sum_y[i], n_pixels)
        bright = DEF_THT_BLACK_MIN <= f_luma <= DEF_THT_WHITE_MIN
        n_diff = round(max(float(int(sad[i])) / (float(int(n_pixels)) * 255.0), 0.0001), 5)
        if i == 0 or last_ref is None:
            sc, prev_diff, ref_luma, last_ref, ratio = True, n_diff, f_luma, i, 0
        elif i - last_ref < min_length:
            ratio, sc = round(n_diff / prev_diff, 4), False
        else:
            ratio = round(n_diff / prev_diff, 4)
            sc = ratio > adaptive_ratio and n_diff > threshold
            prev_diff = n_diff
            if frequency > 1:
                sc = sc or (i % frequency == 0)
            sc = sc or (ratio > DEF_ADAPTIVE_RATIO_RF and bright)
            sc = sc or ratio > DEF_ADAPTIVE_RATIO_VHI
            sc = sc or (ref_luma < DEF_THT_BLACK_MIN and bright)
            sc = sc and tht_black < f_luma < tht_white
        luma[i], ratios[i] = f_luma, ratio
        if sc:
            last_ref, ref_luma, prev[i] = i, f_luma, 1
    return prev, nxt, luma, ratios


def plugin_flags(sad, n_pixels, threshold):
    """the stand-in of misc.SCDetect (module docstring) -> (prev, next)"""
    n = len(sad)
    diff = np.asarray([float(int(s)) / (float(int(n_pixels)) * 255.0) for s in sad], np.float64)
    prev = (diff > threshold).astype(np.int8)
    if n:
        prev[0] = 1
    nxt = np.ones(n, np.int8)
    nxt[:-1] = prev[1:]
    return prev, nxt


def filter_black_white(plugin_prev, plugin_next, sum_y, n_pixels, frequency, tht_white, tht_black):
    """SceneDetection.filter_black_white (vsscdect.py:240-279) on the plugin's flags -> (prev, next, sc_luma)"""
    n = len(sum_y)
    prev, luma = np.zeros(n, np.int8), np.zeros(n, np.float64)
    for i in range(n):
        f_luma = _luma(sum_y[i], n_pixels)
        luma[i] = f_luma
        sc = i == 0 or (plugin_prev[i] == 1 and plugin_next[i] == 0)
        if frequency > 1:
            sc = sc or (i % frequency == 0)
        if sc and (i == 0 or tht_black < f_luma < tht_white):
            prev[i] = 1
    return prev, np.zeros(n, np.int8), luma


def scene_flags(sum_y, sad, n_pixels, threshold=DEF_THRESHOLD, frequency=0, tht_offset=1, min_length=1, tht_white=DEF_THT_WHITE, tht_black=DEF_THT_BLACK,
                sc_tht_filter=0.0):
    """per-frame statistics -> SceneInfo: vsscdect.SceneDetect (:44-87) and SceneDetection.SceneDetect (:200-238) branch for branch.  sum_y / sad: one
    integer per frame (havc_scene_stats, taken with the offset min(max(tht_offset, 1), 25)); n_pixels: pixels per frame of the clip they were taken of."""
    n = len(sum_y)
    branch = detect_branch(threshold, frequency, sc_tht_filter, min_length, tht_offset)
    prev, nxt = np.zeros(n, np.int8), np.zeros(n, np.int8)
    luma, ratio = np.full(n, 0.5, np.float64), np.zeros(n, np.float64)                             # :204-205
    if branch == "frequency":                                                                       # set_scene_change_freq, :53-69
        idx = np.arange(n)
        prev = ((idx % frequency == 0) if frequency > 1 else np.ones(n, bool)).astype(np.int8)
    elif branch == "custom":
        prev, nxt, luma, ratio = custom_detector(sum_y, sad, n_pixels, threshold, frequency, DEF_SC_MIN_DISTANCE, tht_white, tht_black)   # :217-218
    elif branch == "plugin":
        p, q = plugin_flags(sad, n_pixels, threshold)
        prev, nxt, luma = filter_black_white(p, q, sum_y, n_pixels, frequency, tht_white, tht_black)
    return SceneInfo(prev, nxt, luma, ratio, threshold, frequency)


def scene_stats(ctx, clip, offset=1, normalize=False, coeffs=LUMA_LIMITED, tht_black=DEF_THT_BLACK_MIN, tht_white=DEF_THT_WHITE_MIN):
    """havc_scene_stats on a clip u8 [n, h, w, 3] (ndarray, or DeviceImage: read in place) -> structured array (_native.SCENE_REC_DTYPE), one record per frame"""
    from . import _native as nat
    from .device import is_device, operand_ptr
    if not is_device(clip):
        clip = np.ascontiguousarray(clip, dtype=np.uint8)
    n, h, w, _ = clip.shape
    out = np.zeros(n, nat.SCENE_REC_DTYPE)
    p = nat.SceneParams(w, h, n, int(offset), int(coeffs[0]), int(coeffs[1]), int(coeffs[2]), int(coeffs[3]), 1 if normalize else 0, 0,
                        float(tht_black), float(tht_white))
    nat.check(ctx.lib.havc_scene_stats(ctx.h, operand_ptr(clip), C.byref(p), nat.as_ptr(out)), ctx.h)
    return out


def scene_detect(ctx, clip, threshold=DEF_THRESHOLD, frequency=0, sc_tht_filter=0.0, min_length=1, tht_white=DEF_THT_WHITE, tht_black=DEF_THT_BLACK,
                 frame_norm=False, tht_offset=1, coeffs=LUMA_LIMITED):
    """vsscdect.SceneDetect on a 4-D clip (ndarray or DeviceImage) -> SceneInfo.  The refusals come first; the early returns touch no pixel."""
    branch = detect_branch(threshold, frequency, sc_tht_filter, min_length, tht_offset)
    n, h, w, _ = clip.shape
    if branch in ("none", "frequency"):
        z = np.zeros(n, np.int64)
        return scene_flags(z, z, h * w, threshold, frequency, tht_offset, min_length, tht_white, tht_black, sc_tht_filter)
    tw, th = resize_min_hw(w, h)
    if (tw, th) != (w, h):
        from .havc import spline64
        clip = spline64(ctx, clip, tw, th)
    rec = scene_stats(ctx, clip, min(max(tht_offset, 1), 25) if branch == "custom" else 1, frame_norm, coeffs)
    return scene_flags(rec["sum_y"], rec["sad"], tw * th, threshold, frequency, tht_offset, min_length, tht_white, tht_black, sc_tht_filter)
