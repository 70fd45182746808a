"""Edge-masked scene detection without VapourSynth: vsslib/vsscdetect_edge.py on four integers per frame that the GPU takes of a clip in one launch.

The reference's second detector (HAVC_SceneDetectEdges, the one it recommends for blended and smooth transitions) is Python over, per frame, the mean of a
small gray plane, the flag of misc.SCDetect, and std.PlaneStats' average of |Y_n - Y_(n + offset)| with and without an edge mask on it.  `edge_stats` gets
the sums behind those for a whole clip from `havc_scene_edge_stats` (csrc/scedge.hip: exact integers, one launch); the rest is sequential and needs no GPU:

    SceneDetectEdges (:32-102)                     the early returns, the clamps, which selector runs and -- literally -- which props reach it: scene_flags_edges
    vs_edge_based_scenedetect.set_sc_prop (:184-259)   edge_detector: luma gate, the SCDetect and edge_max overrides with their distance rule, reasons 0-4
    SceneDetectionFiltered.set_scenechange (:372-480)  edge_scene_filter: the edge file's OWN copy of the SSIM / histogram filter (not vsscdect.py's: it has a
                                                   reason override, no ratio term, and carries _sc_prev_reason)
both pinned by tests/golden/scdetect_edges.npz, which tools/gen_golden_scedges.py makes by executing the reference's own functions on prescribed statistics.

The prop routing, as the executed reference does it: SceneDetectEdges hands the detector's props to the filter with
CopyFrameProps(props=['_SceneChangePrev', '_SceneChangeNext', 'sc_luma' 'sc_reason']) (:91-94) -- no comma between the last two, so the list names one prop
that does not exist.  The filter therefore sees the detector's flags but the CONSTANTS of :69-70 (sc_luma = 0.15, sc_reason = 0) on every frame, and those
constants are what the final clip carries when the filter ran (:96-97).  Restated as it is: ROUTED_LUMA / ROUTED_REASON.  With the filter off the detector's
own sc_luma / sc_reason come back.

What stands in for native code (UNPINNED; tests/scedges_util.py is the definition of the pixel work, value for value what csrc/scedge.hip computes):
  * zimg's RGB -> GRAY8 and resize_min_HW -> as in scdetect.py: the library's Spline64 on the RGB clip, then Y = (cr R + cg G + cb B + bias) >> 16;
  * std.Convolution (kirsch), akarin.Expr, TCanny(mode=1), std.MaskedMerge, std.PlaneStats -> the stated integer / float32 sequences;
  * `gray[offset:] + gray[-offset]` with VapourSynth's clamp of a request beyond a clip's end -> j = n + offset for n < N - offset, else N - offset;
  * misc.SCDetect(threshold=0.10) -> scdetect.plugin_flags on sad_prev;
  * the filter's skimage / cv2 calls -> havc_scene_ssim / havc_scene_hist and scdetect.hellinger_distance, as in scdetect.scene_detect_filtered.
"""
import ctypes as C
import dataclasses

import numpy as np

from .scdetect import (DEF_HIST_SCORE_EQUAL, DEF_HIST_SCORE_HIGH, DEF_SSIM_SCORE_EQUAL, DEF_THT_BLACK_FREQ, DEF_THT_BLACK_MIN, DEF_THT_WHITE_MIN, FILTER_CHUNK,
                       LUMA_LIMITED, SSIM_WIN, SceneInfo, hellinger_distance, plugin_flags, resize_min_hw, scene_hist, scene_ssim)

DEF_CANNY_SIGMA = 1.2                                  # vs_edge_based_scenedetect's canny_sigma (vsscdetect_edge.py:149)
DEF_SCDETECT_THRESHOLD = 0.10                          # gray.misc.SCDetect(threshold=0.10) (:171)
ROUTED_LUMA, ROUTED_REASON = 0.15, 0                   # :69-70: what the filter sees and the final clip carries (module docstring)
MAX_OFFSET = 25


@dataclasses.dataclass
class EdgeSceneInfo(SceneInfo):
    """SceneInfo + the sc_reason prop of the edge detector (0: none, 1: thresholds, 2: edge_max, 3: tht_max, 4: both / first frame); sc_ratio is zeros"""
    sc_reason: np.ndarray = None       # int8


def _luma(sum_y, n_pixels):
    """round(np.mean(f_y) / 255.0, 4): numpy's round on a float64 scalar"""
    return float(round(np.float64(int(sum_y)) / np.float64(int(n_pixels)) / 255.0, 4))


def _average(total, n_pixels):
    """std.PlaneStats' PlaneStatsAverage of an 8-bit plane"""
    return float(int(total)) / (float(int(n_pixels)) * 255.0)


def next_index(n, n_frames, offset):
    """the frame `gray[offset:] + gray[-offset]` hands out as frame n (module docstring)"""
    return n + offset if n < n_frames - offset else n_frames - offset


def edge_detector(sum_y, plugin_prev, sad_next, sum_masked, n_pixels, threshold, sc_min_int, sc_mult_tht, tht_white, tht_black, debug=None):
    """vs_edge_based_scenedetect.set_sc_prop (vsscdetect_edge.py:184-259) frame by frame in order, with SceneDetectEdges' argument routing (:63, :72-84)
    -> (prev, next, sc_luma, sc_reason).  plugin_prev: misc.SCDetect's _SceneChangePrev.  debug["status"][n]: the selector's status string."""
    n_frames = len(sum_y)
    sc_mult_tht = 7 if sc_mult_tht == 0 else sc_mult_tht                                            # :63
    edge_diff_threshold, ssim_diff_threshold = threshold, round(1.75 * threshold, 5)                # :72-77
    prev, nxt = np.zeros(n_frames, np.int8), np.zeros(n_frames, np.int8)
    luma, reason = np.zeros(n_frames, np.float64), np.zeros(n_frames, np.int8)
    status_of = {} if debug is None else debug.setdefault("status", {})
    last_sc_frame, last_sc_status = -sc_min_int, ""                                                 # :159-160
    for n in range(n_frames):
        if n == 0:                                                                                  # :191-198
            prev[0], luma[0], reason[0] = 1, 0.10, 4
            last_sc_frame, last_sc_status = 0, "Accepted(First)"
            status_of[0] = last_sc_status
            continue
        f_luma = _luma(sum_y[n], n_pixels)
        edge_diff = round(10 * _average(sum_masked[n], n_pixels), 5)
        ssim_diff = round(4 * _average(sad_next[n], n_pixels), 5)
        in_luma_range = tht_black <= f_luma <= tht_white
        above_threshold = (edge_diff > edge_diff_threshold) and (ssim_diff > ssim_diff_threshold)
        above_distance_max = (n - last_sc_frame) >= sc_min_int
        above_distance_min = (n - last_sc_frame) >= max(int(sc_mult_tht * 0.5), 3)
        mandatory_ref_1 = plugin_prev[n] == 1
        mandatory_ref_2 = edge_diff > (edge_diff_threshold * sc_mult_tht)
        luma[n] = f_luma
        accepted = None
        if in_luma_range:
            if mandatory_ref_1:
                if ("tht_max" not in last_sc_status) or above_distance_min:
                    accepted = ("Accepted(tht_max+edge_max)", 4) if mandatory_ref_2 else ("Accepted(tht_max)", 3)
                else:
                    status = "Skipped"
            elif mandatory_ref_2:
                if ("edge_max" not in last_sc_status) or above_distance_min:
                    accepted = ("Accepted(edge_max)", 2)
                else:
                    status = "Skipped"
            elif above_distance_max and above_threshold:
                accepted = ("Accepted", 1)
            else:
                status = "Skipped"
        else:
            status = "Rejected"
        if accepted is not None:
            status, reason[n] = accepted
            prev[n], last_sc_frame, last_sc_status = 1, n, status
        status_of[n] = status
    return prev, nxt, luma, reason


def edge_scene_filter(prev, nxt, luma, reason, scores, ssim_tht, min_length=1, tht_white=0.70, tht_black=0.10, frequency=0, chunk=FILTER_CHUNK, debug=None):
    """the edge file's SceneDetectionFiltered.set_scenechange (vsscdetect_edge.py:372-480) over a whole clip, frame by frame in order, in SceneDetectFilter's
    chunks (:354-368): `n` is the frame's number inside its chunk, t_n and the carried state are global.  prev / nxt / luma / reason: the props the filter
    SEES on every frame (scene_flags_edges passes the routed constants).  _sc_prev_reason is set where the reference sets it: at frame 0 and where a frame is
    taken without a predecessor -- never where a later frame is accepted.  scores(t_n, last) as in scdetect.scene_filter.  -> (prev, next) after the filter;
    debug["scores"] / debug["reasons"] as there."""
    n_frames = len(prev)
    out_prev, out_next = np.array(prev, np.int8), np.array(nxt, np.int8)
    rec_scores = {} if debug is None else debug.setdefault("scores", {})
    rec_reasons = {} if debug is None else debug.setdefault("reasons", {})
    last_index, prev_luma, prev_reason = None, None, None
    for t_n in range(n_frames):
        n = t_n % chunk
        f_luma, f_reason = float(luma[t_n]), int(reason[t_n])
        if t_n == 0:                                                                                # :384-389
            last_index, prev_luma, prev_reason = None, 0, 0
        is_scenechange = prev[t_n] == 1 or t_n == 0
        if is_scenechange and last_index is None:                                                   # :393-405
            out_prev[t_n], out_next[t_n] = 1, 0
            last_index, prev_luma, prev_reason = t_n, f_luma, f_reason
            rec_reasons[t_n] = 1
            continue
        if not is_scenechange:
            continue
        sc_reason = 0
        if n > 0 and (t_n - last_index) < min_length:                                               # :412-422
            if min_length > 1 and n > 1 and prev_luma >= DEF_THT_BLACK_MIN > f_luma:
                out_prev[t_n], out_next[t_n] = 0, 0
                rec_reasons[t_n] = -1
                continue
            sc_reason = 4
        if ssim_tht == 1:                                                                           # :426-430
            ssim_score = hist_score = 1
            scene_change = tht_black < f_luma < tht_white
            sc_reason = (sc_reason + 1) if scene_change else 0
        else:                                                                                       # :431-453 (n < clip.num_frames always holds)
            ssim_raw, hist_compare = scores(t_n, last_index)
            ssim_score = float(round(np.float64(ssim_raw), 4))
            hist_score = round(1 - float(hist_compare), 4)
            if f_reason > 1 and prev_reason < 2:                                                    # override on reason and luma: sc_reason stays
                scene_change = tht_black < f_luma < tht_white
            elif ssim_score < ssim_tht and hist_score < DEF_HIST_SCORE_HIGH:
                scene_change = tht_black < f_luma < tht_white
                if scene_change and sc_reason == 0 and frequency > 1:
                    scene_change = scene_change and not (f_luma < DEF_THT_BLACK_FREQ)
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
        if scene_change:                                                                            # :459-470
            out_prev[t_n], out_next[t_n] = 1, 0
            last_index, prev_luma = t_n, f_luma
        else:
            out_prev[t_n], out_next[t_n] = 0, 0
    return out_prev, out_next


def edges_branch(threshold, frequency=0):
    """which path SceneDetectEdges takes (:39, :60): "none", "frequency" or "detect" """
    if threshold == 0 and frequency == 0:
        return "none"
    if frequency == 1 or (threshold == 0 and frequency > 1):
        return "frequency"
    return "detect"


def scene_flags_edges(sum_y, sad_prev, sad_next, sum_masked, n_pixels, threshold=0.07, frequency=0, ssim_threshold=0.0, sc_min_int=30, sc_mult_tht=7,
                      tht_white=0.70, tht_black=0.12, scores=None, debug=None):
    """SceneDetectEdges (vsscdetect_edge.py:32-102) on per-frame statistics -> EdgeSceneInfo, with the reference function's own defaults.  The statistics are
    havc_scene_edge_stats' (taken with the offset max(sc_diff_offset, 1)); scores: the filter's score callback, needed with ssim_threshold > 0."""
    n = len(sum_y)
    branch = edges_branch(threshold, frequency)
    zeros = np.zeros(n, np.int8)
    if branch == "none":                                                                            # :39-40: no prop but sc_threshold / sc_frequency
        return EdgeSceneInfo(zeros, zeros.copy(), np.zeros(n), np.zeros(n), threshold, frequency, zeros.copy())
    if branch == "frequency":                                                                       # set_scene_change_freq, :42-61
        idx = np.arange(n)
        prev = ((idx % frequency == 0) if frequency > 1 else np.ones(n, bool)).astype(np.int8)
        return EdgeSceneInfo(prev, zeros, np.zeros(n), np.zeros(n), threshold, frequency, zeros.copy())
    plugin_prev, _ = plugin_flags(sad_prev, n_pixels, DEF_SCDETECT_THRESHOLD)
    prev, nxt, luma, reason = edge_detector(sum_y, plugin_prev, sad_next, sum_masked, n_pixels, threshold, sc_min_int, sc_mult_tht, tht_white, tht_black, debug)
    if ssim_threshold > 0:                                                                          # :86-97
        min_length = max(int(round(sc_min_int / 3.0)), 1)
        luma, reason = np.full(n, ROUTED_LUMA, np.float64), np.full(n, ROUTED_REASON, np.int8)      # the props that reach the filter, and the final clip
        prev, nxt = edge_scene_filter(prev, nxt, luma, reason, scores, ssim_threshold, min_length, tht_white, tht_black, frequency, debug=debug)
    return EdgeSceneInfo(prev, nxt, luma, np.zeros(n, np.float64), threshold, frequency, reason)


def edge_stats(ctx, clip, offset=2, coeffs=LUMA_LIMITED, sigma=DEF_CANNY_SIGMA, mask_tap=False):
    """havc_scene_edge_stats on a clip u8 [n, h, w, 3] (ndarray, or DeviceImage: read in place) -> structured array (_native.EDGE_REC_DTYPE), one record per
    frame; with mask_tap (tests) -> (records, mask u8 [n, h, w])"""
    from . import _native as nat
    from .device import is_device, operand_ptr
    if not is_device(clip):
        clip = np.ascontiguousarray(clip, dtype=np.uint8)
    n, h, w, _ = clip.shape
    out = np.zeros(n, nat.EDGE_REC_DTYPE)
    tap = np.zeros((n, h, w), np.uint8) if mask_tap else None
    p = nat.EdgeParams(w, h, n, int(offset), int(coeffs[0]), int(coeffs[1]), int(coeffs[2]), int(coeffs[3]), float(sigma))
    nat.check(ctx.lib.havc_scene_edge_stats(ctx.h, operand_ptr(clip), C.byref(p), nat.as_ptr(out), nat.as_ptr(tap) if mask_tap else None), ctx.h)
    return (out, tap) if mask_tap else out


def edges_offset(sc_diff_offset, n_frames):
    """max(sc_diff_offset, 1) (:64); an offset the clip is too short for is an error in the reference as well (gray[offset:] of nothing)"""
    offset = max(int(sc_diff_offset), 1)
    if offset > MAX_OFFSET:
        raise ValueError(f"SceneDetectEdges: sc_tht_offset must be in range [1-{MAX_OFFSET}], not {sc_diff_offset}")
    if offset >= n_frames:
        raise ValueError(f"SceneDetectEdges: sc_tht_offset = {offset} needs a clip of more than {offset} frames, not {n_frames}")
    return offset


def scene_detect_edges(ctx, clip, threshold=0.07, frequency=0, ssim_threshold=0.0, sc_diff_offset=2, sc_min_int=30, sc_mult_tht=7, tht_white=0.70,
                       tht_black=0.12, coeffs=LUMA_LIMITED, debug=None):
    """SceneDetectEdges on a 4-D clip (ndarray or DeviceImage) -> EdgeSceneInfo: Spline64 to resize_min_hw's size, ONE havc_scene_edge_stats launch, the
    detector on the host; with ssim_threshold > 0 the filter follows with scene_detect_filtered's candidate scheme -- one havc_scene_hist launch and one
    havc_scene_ssim launch over the detector's candidates, a one-pair launch only behind a rejection.  The early returns touch no pixel (ctx may be None).
    debug receives "records" (the statistics), "candidates", the launch counts, "status" and the filter's "scores" / "reasons"."""
    from .device import DeviceImage, is_device
    n, h, w, _ = clip.shape
    dbg = debug if debug is not None else {}
    dbg.update(candidates=[], hist_launches=0, ssim_launches=0, fallback_launches=0, fallback_pairs=[])
    kw = dict(threshold=threshold, frequency=frequency, ssim_threshold=ssim_threshold, sc_min_int=sc_min_int, sc_mult_tht=sc_mult_tht, tht_white=tht_white,
              tht_black=tht_black)
    if edges_branch(threshold, frequency) != "detect":
        z = np.zeros(n, np.int64)
        return scene_flags_edges(z, z, z, z, h * w, **kw)
    offset = edges_offset(sc_diff_offset, n)
    tw, th = resize_min_hw(w, h)
    if ssim_threshold > 0 and ssim_threshold != 1 and (tw < SSIM_WIN or th < SSIM_WIN):
        raise ValueError(f"scene_detect_edges: structural_similarity's 7 x 7 window needs frames of at least 7 x 7, not {th} x {tw}")
    if (tw, th) != (w, h):
        from .havc import spline64
        clip = spline64(ctx, clip, tw, th)
    small = clip if is_device(clip) else DeviceImage.from_numpy(ctx, clip)
    rec = edge_stats(ctx, small, offset, coeffs)
    dbg["records"] = rec
    hists, ssim = {}, {}

    def scores(t_n, last):
        if (t_n, last) not in ssim:                                                                 # behind a rejection: the pair was not foreseen
            ssim[(t_n, last)] = scene_ssim(ctx, small, [(t_n, last)])[0]
            dbg["fallback_launches"] += 1
            dbg["fallback_pairs"].append((t_n, last))
        return ssim[(t_n, last)], hellinger_distance(hists[last], hists[t_n])

    if ssim_threshold > 0:
        # the filter's candidates are the detector's flags: known before it runs, so the detector is evaluated once for them, once inside scene_flags_edges
        pp, _ = plugin_flags(rec["sad_prev"], tw * th, DEF_SCDETECT_THRESHOLD)
        prev = edge_detector(rec["sum_y"], pp, rec["sad_next"], rec["sum_masked"], tw * th, threshold, sc_min_int, sc_mult_tht, tht_white, tht_black)[0]
        cand = [i for i in range(n) if i == 0 or prev[i] == 1]
        dbg["candidates"] = cand
        if ssim_threshold != 1 and len(cand) > 1:
            hists = dict(zip(cand, scene_hist(ctx, small, cand)))
            pairs = [(cand[i], cand[i - 1]) for i in range(1, len(cand))]
            ssim = dict(zip(pairs, scene_ssim(ctx, small, pairs)))
            dbg["hist_launches"], dbg["ssim_launches"] = 1, 1
    return scene_flags_edges(rec["sum_y"], rec["sad_prev"], rec["sad_next"], rec["sum_masked"], tw * th, scores=scores, debug=dbg, **kw)
