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
exist here: NotImplementedError, before anything is enqueued.  That refusal of `detect_branch` / `scene_flags` / `scene_detect` (and HAVC_SceneDetect)
STAYS as it is: tests/test_scdetect_host.py pins it.

The filter itself is built next to them, as new functions, and reached through HAVC_extract_reference_frames (havc.py):

    scene_detect_filtered                          SceneDetection.SceneDetect (:200-238) with the filter on: stage 1 = the detector with min_length 1 (:214-215) or
                                                   the plugin path, stage 2 = the filter, on the same small clip
    scene_filter                                   _scene_detect_filter_task.set_scenechange (:380-483) in SceneDetectFilter's 5000-frame chunks (:352-366), frame by
                                                   frame in order -- pinned by tests/golden/scfilter.npz, which tools/gen_golden_scfilter.py makes by executing the
                                                   reference's own selector on recorded scores
    scene_hist / scene_ssim                        havc_scene_hist / havc_scene_ssim (csrc/scfilter.hip): the histogram and the SSIM of listed frames, one launch each
    hellinger_distance                             cv2.compareHist(HISTCMP_HELLINGER) of the two L2-normalised histograms, float64, on the host

What stands in for foreign code in the filter (UNPINNED as well: neither library can be executed where the fixtures are made):
  * skimage's structural_similarity -> its published formula over 7 x 7 window sums, which are exact integers for uint8 planes (csrc/scfilter_ops.h;
    tests/scfilter_util.py restates it in numpy and compares it with the scipy.ndimage.uniform_filter form skimage itself evaluates);
  * cv2.cvtColor(COLOR_RGB2GRAY) and the Y of COLOR_RGB2YUV -> (4899 R + 9617 G + 1868 B + 8192) >> 14 (oracle/cvcolor.py: the same expression for both);
  * cv2.calcHist -> an exact integer histogram; cv2.normalize (L2, float32 there) and compareHist(HELLINGER) -> OpenCV's published definition in float64:
    sqrt(max(1 - sum(sqrt(h1 h2)) / sqrt(sum(h1) sum(h2)), 0)), the 1 / sqrt factor replaced by 1 when |sum(h1) sum(h2)| <= FLT_EPSILON.  float32 there,
    float64 here: a score within ~1e-7 of a 4-decimal rounding boundary or of a threshold may fall on the other side;
  * the RGB clip the filter reads is `resize_min_HW(clip)` (zimg) in the reference -> the library's Spline64 at the same size, the clip the statistics are
    taken of.
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

DEF_THT_BLACK_FREQ = 0.14                              # :42 (the filter's frequency override)
DEF_SSIM_SCORE_EQUAL, DEF_HIST_SCORE_EQUAL, DEF_HIST_SCORE_HIGH = 0.69, 0.70, 0.95     # :52-54
FILTER_CHUNK = 5000                                    # SceneDetectFilter's t_step (vsscdect.py:353)
SSIM_WIN = 7                                           # skimage's default win_size: a plane below 7 x 7 raises there
FLT_EPSILON = float(np.finfo(np.float32).eps)

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


# ---- the SSIM / histogram post-filter (vsscdect.py:352-495): new functions; the refusals above stay as they are ----------------------------------------------
def filter_active(sc_tht_filter, min_length):
    """vsscdect.py:227 with the clamp of :82: does SceneDetect run SceneDetectFilter?"""
    return 0.0 < sc_tht_filter < 1.0 or min(max(min_length, 1), 25) > 1


def hellinger_distance(h1, h2):
    """cv2.compareHist(H1, H2, HISTCMP_HELLINGER) of the two histograms after _calc_histogram's cv2.normalize (L2 norm 1; a zero histogram stays zero), by
    OpenCV's published definition, float64 throughout (cv2 holds the normalised histograms in float32: module docstring)"""
    out = []
    for h in (h1, h2):
        a = np.asarray(h, np.float64)
        norm = float(np.sqrt(np.sum(a * a)))
        out.append(a * (1.0 / norm if norm > np.finfo(np.float64).eps else 0.0))
    a, b = out
    s1 = float(np.sum(a)) * float(np.sum(b))
    s1 = 1.0 / float(np.sqrt(s1)) if abs(s1) > FLT_EPSILON else 1.0
    return float(np.sqrt(max(1.0 - float(np.sum(np.sqrt(a * b))) * s1, 0.0)))


def scene_filter(prev, nxt, luma, ratio, scores, ssim_tht, min_length=1, tht_white=DEF_THT_WHITE, tht_black=DEF_THT_BLACK, frequency=0, chunk=FILTER_CHUNK,
                 debug=None):
    """_scene_detect_filter_task.set_scenechange (vsscdect.py:380-483) over a whole clip, frame by frame in order, in SceneDetectFilter's chunks (:352-366):
    `n` of `n > 0` / `n > 1` is the frame's number inside its chunk, t_n and the carried state (_sc_last_index, _sc_prev_luma; the previous plane and
    histogram = the last accepted frame's number) are global.  prev / nxt / luma / ratio: what stage 1 left on every frame.  scores(t_n, last) ->
    (structural_similarity of the two frames' gray planes, compareHist(HELLINGER) of their histograms), both unrounded; asked only where the reference
    computes them.  -> (prev, next) after the filter.  debug["scores"][t_n] = (ssim_score, hist_score) as rounded there, debug["reasons"][t_n] = sc_reason."""
    n_frames = len(prev)
    out_prev, out_next = np.array(prev, np.int8), np.array(nxt, np.int8)
    rec_scores = {} if debug is None else debug.setdefault("scores", {})
    rec_reasons = {} if debug is None else debug.setdefault("reasons", {})
    last_index, prev_luma = None, None
    for t_n in range(n_frames):
        n = t_n % chunk                                                                             # clip[t_start:t_end]: the selector's n is chunk-local
        f_luma, f_ratio = float(luma[t_n]), float(ratio[t_n])
        if t_n == 0:                                                                                # :391-395
            last_index, prev_luma = None, 0
        is_scenechange = prev[t_n] == 1 or t_n == 0
        if is_scenechange and last_index is None:                                                   # :399-410
            out_prev[t_n], out_next[t_n] = 1, 0
            last_index, prev_luma = t_n, f_luma
            rec_reasons[t_n] = 1
            continue
        if not is_scenechange:
            continue
        sc_reason = 0
        if n > 0 and (t_n - last_index) < min_length:                                               # :417-427
            if min_length > 1 and n > 1 and prev_luma >= DEF_THT_BLACK_MIN > f_luma:
                out_prev[t_n], out_next[t_n] = 0, 0
                rec_reasons[t_n] = -1
                continue
            sc_reason = 4
        if ssim_tht == 1:                                                                           # :431-435
            ssim_score = hist_score = 1
            scene_change = tht_black < f_luma < tht_white
            sc_reason = (sc_reason + 1) if scene_change else 0
        else:                                                                                       # :436-456 (n < clip.num_frames always holds)
            ssim_raw, hist_compare = scores(t_n, last_index)
            ssim_score = float(round(np.float64(ssim_raw), 4))                                      # skimage hands back a numpy float64: numpy's round
            hist_score = round(1 - float(hist_compare), 4)                                          # cv2 hands back a Python float: Python's round
            if ssim_score < ssim_tht and hist_score < DEF_HIST_SCORE_HIGH:
                scene_change = tht_black < f_luma < tht_white
                if scene_change and sc_reason == 0 and frequency > 1:
                    scene_change = scene_change and not (f_luma < DEF_THT_BLACK_FREQ and f_ratio < DEF_ADAPTIVE_RATIO_RF)
                sc_reason = (sc_reason + 1) if scene_change else 0
            elif ssim_score >= DEF_SSIM_SCORE_EQUAL and prev_luma < DEF_THT_BLACK_MIN <= f_luma:
                scene_change = tht_black < f_luma < tht_white
                sc_reason = (sc_reason + 2) if scene_change else 0
            elif ssim_score >= DEF_SSIM_SCORE_EQUAL and hist_score < DEF_HIST_SCORE_EQUAL:
                scene_change = DEF_THT_BLACK_MIN < f_luma < DEF_THT_WHITE_MIN
                sc_reason = (sc_reason + 3) if scene_change else 0
            else:
                scene_change, sc_reason = False, 0
        rec_scores[t_n], rec_reasons[t_n] = (ssim_score, hist_score), sc_reason
        if scene_change:                                                                            # :462-473
            out_prev[t_n], out_next[t_n] = 1, 0
            last_index, prev_luma = t_n, f_luma
        else:
            out_prev[t_n], out_next[t_n] = 0, 0
    return out_prev, out_next


def _frame_list(ctx, what, clip, frames, width):
    from .device import is_device
    if not is_device(clip):
        clip = np.ascontiguousarray(clip, dtype=np.uint8)
    lst = np.ascontiguousarray(np.asarray(frames, np.int32).reshape(-1, width))
    if clip.ndim != 4 or clip.shape[3] != 3 or len(lst) == 0:
        raise ValueError(f"{what}: needs a clip [n, h, w, 3] and a list that is not empty")
    return clip, lst


def scene_hist(ctx, clip, frames):
    """havc_scene_hist: the 256-bin histogram of cv2's gray of the listed frames of a clip u8 [n, h, w, 3] (ndarray, or DeviceImage: read in place), ONE launch
    -> uint32 [len(frames), 256], exact counts"""
    from . import _native as nat
    from .device import operand_ptr
    clip, idx = _frame_list(ctx, "scene_hist", clip, frames, 1)
    n, h, w, _ = clip.shape
    out = np.zeros((len(idx), 256), np.uint32)
    nat.check(ctx.lib.havc_scene_hist(ctx.h, operand_ptr(clip), n, w, h, nat.as_ptr(idx), len(idx), nat.as_ptr(out)), ctx.h)
    return out


def scene_ssim(ctx, clip, pairs):
    """havc_scene_ssim: skimage's structural_similarity(gray_a, gray_b) (win_size 7, data_range 255, sample covariance) of the listed frame pairs of a clip,
    ONE launch -> float64 [len(pairs)]; bit-identical from run to run"""
    from . import _native as nat
    from .device import operand_ptr
    clip, prs = _frame_list(ctx, "scene_ssim", clip, pairs, 2)
    n, h, w, _ = clip.shape
    out = np.zeros(len(prs), np.float64)
    nat.check(ctx.lib.havc_scene_ssim(ctx.h, operand_ptr(clip), n, w, h, nat.as_ptr(prs), len(prs), nat.as_ptr(out)), ctx.h)
    return out


def scene_detect_filtered(ctx, clip, threshold=DEF_THRESHOLD, frequency=0, sc_tht_filter=0.0, min_length=1, tht_white=DEF_THT_WHITE, tht_black=DEF_THT_BLACK,
                          frame_norm=False, tht_offset=1, coeffs=LUMA_LIMITED, debug=None):
    """vsscdect.SceneDetect with the post-filter on (0 < sc_tht_filter < 1 or min_length > 1) on a 4-D clip (ndarray or DeviceImage) -> SceneInfo.
    Stage 1 (SceneDetection.SceneDetect, :213-222): the custom detector with min_length 1 -- or, with sc_tht_filter == 0, threshold >= 0.10 and offset 1, the
    plugin path with its black / white filter -- on the statistics of the small clip.  Stage 2: scene_filter.  Its candidates (frame 0 and the frames stage 1
    flagged) are known before it runs: ONE havc_scene_hist launch takes all their histograms and ONE havc_scene_ssim launch every (candidate, previous
    candidate) pair; the walk needs another pair only behind a rejection and fetches it with a one-pair launch.  An ndarray clip is uploaded once.  The early
    returns (:50, :71) never reach the filter and touch no pixel (ctx may be None).  debug receives "candidates", "hist_launches", "ssim_launches",
    "fallback_launches", "fallback_pairs", and scene_filter's "scores" / "reasons"."""
    from .device import DeviceImage, is_device
    n, h, w, _ = clip.shape
    dbg = debug if debug is not None else {}
    dbg.update(candidates=[], hist_launches=0, ssim_launches=0, fallback_launches=0, fallback_pairs=[])
    if (threshold == 0 and frequency == 0) or frequency == 1 or (threshold == 0 and frequency > 1):
        z = np.zeros(n, np.int64)
        return scene_flags(z, z, h * w, threshold, frequency)
    t_offset, m_length = min(max(tht_offset, 1), 25), min(max(min_length, 1), 25)                   # :81-82
    if not filter_active(sc_tht_filter, m_length):
        raise ValueError("scene_detect_filtered: the post-filter is off (0 < sc_tht_filter < 1 or min_length > 1 switches it on): scene_detect is the function")
    tw, th = resize_min_hw(w, h)
    if sc_tht_filter != 1 and (tw < SSIM_WIN or th < SSIM_WIN):
        raise ValueError(f"scene_detect_filtered: structural_similarity's 7 x 7 window needs frames of at least 7 x 7, not {th} x {tw}")
    if (tw, th) != (w, h):
        from .havc import spline64
        clip = spline64(ctx, clip, tw, th)
    small = clip if is_device(clip) else DeviceImage.from_numpy(ctx, clip)
    custom = sc_tht_filter > 0.0 or threshold < 0.10 or t_offset > 1                                # :213
    rec = scene_stats(ctx, small, t_offset if custom else 1, frame_norm, coeffs)
    if custom:
        prev, nxt, luma, ratio = custom_detector(rec["sum_y"], rec["sad"], tw * th, threshold, frequency, 1, tht_white, tht_black)                 # :215
    else:
        p, q = plugin_flags(rec["sad"], tw * th, threshold)
        prev, nxt, luma = filter_black_white(p, q, rec["sum_y"], tw * th, frequency, tht_white, tht_black)
        ratio = np.zeros(n, np.float64)
    cand = [i for i in range(n) if i == 0 or prev[i] == 1]
    dbg["candidates"] = cand
    hists, ssim = {}, {}
    if sc_tht_filter != 1 and len(cand) > 1:
        hists = dict(zip(cand, scene_hist(ctx, small, cand)))
        pairs = [(cand[i], cand[i - 1]) for i in range(1, len(cand))]
        ssim = dict(zip(pairs, scene_ssim(ctx, small, pairs)))
        dbg["hist_launches"], dbg["ssim_launches"] = 1, 1

    def scores(t_n, last):
        if (t_n, last) not in ssim:                                                                 # behind a rejection: the pair was not foreseen
            ssim[(t_n, last)] = scene_ssim(ctx, small, [(t_n, last)])[0]
            dbg["fallback_launches"] += 1
            dbg["fallback_pairs"].append((t_n, last))
        return ssim[(t_n, last)], hellinger_distance(hists[last], hists[t_n])

    prev, nxt = scene_filter(prev, nxt, luma, ratio, scores, sc_tht_filter, m_length, tht_white, tht_black, frequency, debug=dbg)
    return SceneInfo(prev, nxt, luma, ratio, threshold, frequency)
