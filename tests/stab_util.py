"""numpy restatement of havc_chroma_stab_clip / havc_reduce_flicker_clip (csrc/chroma_stab.hip) and of the reference's Python around them
(vs_chroma_stabilizer_ex, vsslib/vsfilters.py:38-63, 84-157, 216-356; the stab and flicker stages of HAVC_stabilizer, vsdeoldify/__init__.py:2862-2866): THE
DEFINITION of the stand-ins for this project (include/havc_mi355.h has it in prose).  The kernels equal this file byte for byte.

UNPINNED -- VapourSynth, zimg and the ReduceFlicker plugin cannot be executed where the fixtures are made.  What stands in for them:
  * resize.Bicubic to YUV420P8 and back to RGB24 with error diffusion -> tests/tweak_util.py `rgb_to_yuv420` / `yuv420_to_rgb` (every assumption about zimg
    is listed there).  The forward conversion has no dither, also where the reference asks for one (8 bit in, 8 bit out).
  * std.AverageFrames on 8-bit clips, integer weights, scale = 100, planes = [1, 2] -> `average`: out = clamp((sum w_i s_i + 50) // 100, 0, 255) on U and V;
    Y is copied from the MIDDLE input (the centre frame of the temporal form, the centre clip of the list form).  Temporal form (`temporal_sources`): slot k
    of frame n is frame n + k clamped to [0, last].  With scenechange=True, walk back from the centre: at the first slot whose frame carries
    _SceneChangePrev every earlier slot is replaced by that frame; walk forward likewise with _SceneChangeNext.  Arrays carry no props: they come from a
    SceneInfo (`scenes`), None = no scene changes.
  * vs_get_clip_frame(clip, d): frame n is yuv420_to_rgb(Y_n, U_m, V_m), m = clamp(n + d, 0, last), error diffusion applied (its AverageFrames has the one
    weight 100 at offset d, and Y from the centre).
  * vs_reduce_flicker(strength=2, aggressive=0) -> `reduce_flicker`.  RESTATED FROM MEMORY of the plugin's scalar code and UNPINNED: per sample of each RGB
    plane, frames n < 2 or n > last - 2 pass through; otherwise with p2, p1, c, n1, n2 the sample in frames n - 2 .. n + 2: d = min(|c - p2|, |c - n2|),
    avg = (p1 + 2 c + n1 + 2) >> 2, ul = max(min(p1, n1) - d, c), ll = min(max(p1, n1) + d, c), out = clamp(avg, ll, ul) = min(max(avg, ll), ul).
  * restore_color (vsslib/restcolor.py:38-83) WITH its frame-level gate: scenechange = mean(mask) / 255 with mask = 255 where S_gray < tht else 0, i.e.
    ((255 count) / n_pixels) / 255 in float64 (count / n_pixels up to the last bit; the reference's own two divisions are kept); if 0 < tht_scen < 1 and
    scenechange > tht_scen the frame is img_gray untouched, otherwise the per-pixel binary path of tests/recover_util.py `restore_color` (cv2's integer HSV,
    hue_adjust 'none').
  * vs_sc_recover_clip_color(scenechange=False) (vsfilters.py:327-351): frames n < 15 stay as they are; f_luma = get_image_luma(clip_d[n]) outside
    0.22 .. 0.78 -> weight = min(weight, -0.8).  n is first_frame + the index in the array.

PINNED by tests/golden/chroma_stab.npz (made by executing the reference, tools/gen_golden_stab.py) in tests/test_stab_host.py: what vsdeoldify_amd/chroma_stab.py
derives -- N, both weight lists, the resize and AverageFrames arguments in call order, vs_get_clip_frame's weight lists, the n < 15 rule and the luma-band
override.  This file takes the weight lists from vsdeoldify_amd.chroma_stab, so the pin covers it too.

`book`: a dict that receives what the definition did -- "gate" / "band" {(n, d): bool} of the restored frames, "replaced" (slots the scene walk replaced),
"flicker_changed" (samples the flicker pass changed) -- so that a test can assert that its inputs take every branch."""
import numpy as np

from oracle import cvcolor, pipeline
from tests import recover_util as RU
from tests import tweak_util as TU
from vsdeoldify_amd import chroma_stab as CS
from vsdeoldify_amd import equalize as EQ

BINARY_FIRST = 15                                              # vsfilters.py:337
STANDARD_DARK, STANDARD_BRIGHT = 0.22, 0.78                    # vsslib/constants.py:28-29


# ---- std.AverageFrames (stand-in) -------------------------------------------------------------------------------------------------------------------------------
def temporal_sources(n_frames, n_weights, scenes=None, scenechange=True, book=None):
    """-> int [n_frames, n_weights]: the frame every slot of every output frame reads"""
    nh, last = (n_weights - 1) // 2, n_frames - 1
    prev = np.zeros(n_frames, bool) if scenes is None else np.asarray(scenes.scene_change_prev) != 0
    nxt = np.zeros(n_frames, bool) if scenes is None else np.asarray(scenes.scene_change_next) != 0
    out = np.empty((n_frames, n_weights), np.int64)
    replaced = 0
    for n in range(n_frames):
        slot = [min(max(n + k, 0), last) for k in range(-nh, nh + 1)]
        if scenechange:
            for i in range(nh, 0, -1):                         # back from the centre
                if prev[slot[i]]:
                    replaced += sum(slot[j] != slot[i] for j in range(i))
                    slot[:i] = [slot[i]] * i
                    break
            for i in range(nh, n_weights - 1):                 # forward from the centre
                if nxt[slot[i]]:
                    replaced += sum(slot[j] != slot[i] for j in range(i + 1, n_weights))
                    slot[i + 1:] = [slot[i]] * (n_weights - 1 - i)
                    break
        out[n] = slot
    if book is not None:
        book["replaced"] = book.get("replaced", 0) + replaced
    return out


def average(planes, weights):
    """list form on ONE plane kind: planes = the inputs in list order (uint8, equal shapes) -> clamp((sum w_i s_i + 50) // 100, 0, 255)"""
    acc = np.zeros(np.asarray(planes[0]).shape, np.int64)
    for p, w in zip(planes, weights):
        acc += int(w) * np.asarray(p).astype(np.int64)
    return np.clip((acc + 50) // 100, 0, 255).astype(np.uint8)


def average_temporal(plane, weights, scenes=None, scenechange=True, book=None):
    """temporal form on ONE plane kind [n, ...]"""
    src = temporal_sources(plane.shape[0], len(weights), scenes, scenechange, book)
    return average([plane[src[:, k]] for k in range(len(weights))], weights)


# ---- tht == 0: vs_clip_color_stabilizer (vsfilters.py:38-63) -----------------------------------------------------------------------------------------------
def clip_color_stabilizer(clip, nframes=5, mode="A", scenes=None, book=None):
    _, weights = CS.weight_list(nframes, mode)
    y, u, v = TU.rgb_to_yuv420(clip)
    src = temporal_sources(clip.shape[0], len(weights), scenes, True, book)
    u = average([u[src[:, k]] for k in range(len(weights))], weights)
    v = average([v[src[:, k]] for k in range(len(weights))], weights)
    return TU.yuv420_to_rgb(y, u, v)


# ---- tht > 0: _average_clips_ex (vsfilters.py:216-242) -----------------------------------------------------------------------------------------------------
def gray_fraction(count, n_pixels):
    """np.mean(np.where(S < tht, 255, 0)) / 255: the sum of the mask is the exact integer 255 count"""
    return (float(255 * int(count)) / float(n_pixels)) / 255.0


def frame_decision(sum_y, gray_count, n_pixels, weight, tht_scen):
    """-> (effective weight, gate) of one frame of a shifted clip from its two integer sums: what havc_chroma_stab_frame_params answers"""
    f_luma = EQ.f_luma(sum_y, n_pixels, False)                  # get_image_luma(img, 255) from the integer sum of cv2's Y
    if not (STANDARD_DARK <= f_luma <= STANDARD_BRIGHT):
        weight = min(weight, -0.8)
    gate = 0 < tht_scen < 1 and gray_fraction(gray_count, n_pixels) > tht_scen
    return float(weight), bool(gate)


def restore_frame(n, gray, color, sat, tht, weight, tht_scen, key=None, book=None):
    """color_frame (vsfilters.py:327-351, scenechange=False) -> restore_color with its gate"""
    if n < BINARY_FIRST:
        return gray
    f_luma = pipeline.get_image_luma(gray, 255)
    band = not (STANDARD_DARK <= f_luma <= STANDARD_BRIGHT)
    if band:
        weight = min(weight, -0.8)
    count = int((cvcolor.rgb2hsv_u8(gray)[:, :, 1] < tht).sum())
    gate = 0 < tht_scen < 1 and gray_fraction(count, gray.shape[0] * gray.shape[1]) > tht_scen
    if book is not None:
        book.setdefault("band", {})[key] = bool(band)
        book.setdefault("gate", {})[key] = bool(gate)
    if gate:
        return gray
    return RU.restore_color(color, gray, sat, tht, weight)


def shifted_clips(y, u, v, offsets):
    """vs_get_clip_frame for every offset with ONE walk of the error diffusion -> uint8 [len(offsets), n, h, w, 3]"""
    n = y.shape[0]
    idx = np.array([[min(max(f + d, 0), n - 1) for f in range(n)] for d in offsets])
    yy = np.broadcast_to(y, (len(offsets),) + y.shape)
    return TU.yuv420_to_rgb(yy, u[idx], v[idx])


def average_clips_ex(clip, nframes=5, mode="A", sat=1.0, tht=15, weight=0.2, tht_scen=0.8, first_frame=0, book=None):
    _, weights = CS.weight_list(nframes, mode)
    nh = (len(weights) - 1) // 2
    offsets = [d for d in range(-nh, nh + 1) if d != 0]
    y, u, v = TU.rgb_to_yuv420(clip)
    shifted = shifted_clips(y, u, v, offsets)
    restored = np.stack([np.stack([restore_frame(first_frame + n, shifted[i, n], clip[n], sat, tht, weight, tht_scen, (n, d), book)
                                   for n in range(clip.shape[0])]) for i, d in enumerate(offsets)])
    _, ur, vr = TU.rgb_to_yuv420(restored)
    us = [ur[i] for i in range(nh)] + [u] + [ur[i] for i in range(nh, 2 * nh)]
    vs = [vr[i] for i in range(nh)] + [v] + [vr[i] for i in range(nh, 2 * nh)]
    return TU.yuv420_to_rgb(y, average(us, weights), average(vs, weights))


def chroma_stabilizer_ex(clip, nframes=5, mode="A", sat=1.0, tht=0, weight=0.5, tht_scen=0.8, scenes=None, first_frame=0, book=None):
    """vs_chroma_stabilizer_ex (vsfilters.py:84-115) with hue_adjust 'none' and algo 0 on uint8 [n, h, w, 3]"""
    clip = np.asarray(clip)
    if tht == 0:
        return clip_color_stabilizer(clip, nframes, mode, scenes, book)
    return average_clips_ex(clip, nframes, mode, sat, tht, weight, tht_scen, first_frame, book)


# ---- vs_reduce_flicker(strength=2, aggressive=0) (stand-in, restated from memory, UNPINNED) --------------------------------------------------------------------
def reduce_flicker(clip, book=None):
    clip = np.asarray(clip)
    n = clip.shape[0]
    out = clip.copy()
    if n >= 5:
        x = clip.astype(np.int32)
        p2, p1, c, n1, n2 = x[:-4], x[1:-3], x[2:-2], x[3:-1], x[4:]
        d = np.minimum(np.abs(c - p2), np.abs(c - n2))
        avg = (p1 + 2 * c + n1 + 2) >> 2
        ul = np.maximum(np.minimum(p1, n1) - d, c)
        ll = np.minimum(np.maximum(p1, n1) + d, c)
        out[2:-2] = np.minimum(np.maximum(avg, ll), ul).astype(np.uint8)
    if book is not None:
        book["flicker_changed"] = book.get("flicker_changed", 0) + int((out != clip).sum())
    return out


def stab_stage(clip, nframes=5, mode="A", sat=1.0, tht=0, weight=0.5, tht_scen=0.8, scenes=None, first_frame=0, flicker=True, book=None):
    """the stab stage of HAVC_stabilizer without a hue adjustment: vs_chroma_stabilizer_ex, then vs_reduce_flicker"""
    out = chroma_stabilizer_ex(clip, nframes, mode, sat, tht, weight, tht_scen, scenes, first_frame, book)
    return reduce_flicker(out, book) if flicker else out


# ---- clips ----------------------------------------------------------------------------------------------------------------------------------------------------
def make_clip(h, w, n, seed=0):
    """tweak_util.make_clip's tinted noise made temporally coherent (a base frame plus a little noise per frame, so that neighbours resemble each other), plus:
    frames desaturated towards gray (every third from 15 on), one dark and one bright frame in the restored range, and a region that oscillates from frame to
    frame (what the flicker pass acts on)"""
    base = TU.make_clip(h, w, 2, seed)[0].astype(np.int32)
    r = np.random.default_rng(7 * h + w + n + seed)
    clip = np.clip(base[None] + r.integers(-12, 13, (n, h, w, 3)), 0, 255).astype(np.int32)
    gray = clip.mean(-1, keepdims=True)
    for f in range(n):
        if f % 3 == 0:
            clip[f] = (gray[f] + (clip[f] - gray[f]) * 0.03).round()                               # almost gray: the gate's side of tht_scen
        elif f % 3 == 1:
            clip[f] = (gray[f] + (clip[f] - gray[f]) * 0.25).round()                               # partly gray
    if n > 16:
        clip[16] = clip[16] // 8                                                                   # dark: f_luma < 0.22
    if n > 17:
        clip[17] = 255 - (255 - clip[17]) // 8                                                     # bright: f_luma > 0.78
    hh, ww = max(h // 2, 1), max(w // 2, 1)
    for f in range(n):
        clip[f, :hh, :ww] = np.clip(clip[f, :hh, :ww] + (40 if f % 2 else -40), 0, 255)
    return clip.astype(np.uint8)
