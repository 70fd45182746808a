"""The temporal half of HAVC_stabilizer (vsdeoldify/__init__.py:2862-2866), without VapourSynth: vs_chroma_stabilizer_ex (vsslib/vsfilters.py:84-115 ->
vs_clip_color_stabilizer, :38-63, or _average_clips_ex, :216-242, with vs_get_clip_frame, :255-287, and vs_sc_recover_clip_color, :306-356 ->
restcolor.restore_color, vsslib/restcolor.py:38-83) and vs_reduce_flicker (vsslib/vsplugins.py:263).

PINNED -- the reference's Python, restated here as a PLAN: `weight_list` (N and both weight builders, the asymmetric weighted list included), `stab_plan`
(every native call in order with its arguments, vs_get_clip_frame's one-hot weight lists) and `recover_rule` (color_frame's `n < 15` and its luma-band
override).  tests/golden/chroma_stab.npz records the same by EXECUTING the reference against a recording vapoursynth stand-in (tools/gen_golden_stab.py);
tests/test_stab_host.py compares them for nframes 2..16 and both modes.

UNPINNED -- the native filters (zimg's resize, std.AverageFrames, the ReduceFlicker plugin) cannot be executed where the fixtures are made.
tests/stab_util.py restates them in numpy and is THE DEFINITION for this project; the ReduceFlicker stand-in is restated from memory of the plugin's scalar
code.  The kernels (csrc/chroma_stab.hip, csrc/tweak.hip) equal that file byte for byte.

`chroma_stab_np` / `reduce_flicker_np` run on a clip [n, h, w, 3], ndarray or DeviceImage; a DeviceImage in gives a DeviceImage out and the call only enqueues.
Arrays carry no frame props: the scene changes AverageFrames reads come from a SceneInfo (`scenes=`), None = no scene changes.
"""
import ctypes as C
import math

import numpy as np

from .tweak import BICUBIC_TO_RGB, BICUBIC_TO_YUV

BICUBIC_TO_YUV_DITHER = dict(BICUBIC_TO_YUV, dither_type="error_diffusion")                       # vsfilters.py:220, 228
BINARY_FIRST = 15                                                                                 # vsfilters.py:337
STANDARD_DARK, STANDARD_BRIGHT = 0.22, 0.78                                                       # vsslib/constants.py:28-29
MODES_ARITHMETIC = ("A", "arithmetic", "center")
MODES_WEIGHTED = ("W", "weighted", "left", "right")


def _err(msg):
    from .havc import HAVCError
    return HAVCError(msg)


# ---- the reference's Python ------------------------------------------------------------------------------------------------------------------------------------
def build_avg_arithmetic(n):
    """vsfilters.py:118-133"""
    nh = round((n - 1) / 2)
    wi = math.trunc(100.0 / n)
    return [wi] * nh + [100 - (n - 1) * wi] + [wi] * nh


def build_avg_weighted(n):
    """vsfilters.py:136-157, as written: the left half is NOT mirrored (N = 5 -> [6, 13, 62, 6, 13])"""
    nh = round((n - 1) / 2)
    base = n * (n + 1) * 0.5
    side = [math.trunc(1 * 100 * (i + 1) / base) for i in range(nh)]
    return side + [100 - 2 * sum(side)] + side


def weight_list(nframes, mode):
    """vsfilters.py:40-51 / 90-101 -> (N, weights)"""
    if nframes % 2 == 0:
        nframes += 1
    n = max(3, min(nframes, 15))
    if mode in MODES_ARITHMETIC:
        return n, build_avg_arithmetic(n)
    if mode in MODES_WEIGHTED:
        return n, build_avg_weighted(n)
    raise _err("HybridAVC: unknown average method: " + str(mode))


def get_clip_frame_weights(d):
    """vs_get_clip_frame (vsfilters.py:255-270): 100 at offset d of -|d| .. |d|"""
    n = abs(d)
    return [100 if i == d else 0 for i in range(-n, n + 1)]


def stab_plan(nframes=5, mode="A", sat=1.0, tht=0, weight=0.5, tht_scen=0.8):
    """vs_chroma_stabilizer_ex(hue_adjust='none', algo=0) -> dict(N, weights, offsets, calls): the native calls in order"""
    n, weights = weight_list(nframes, mode)
    avg = lambda clips, w, sc: ["std.AverageFrames", dict(clips=clips, weights=list(w), scale=100, scenechange=sc, planes=[1, 2])]
    if tht == 0:
        return dict(N=n, weights=weights, offsets=[],
                    calls=[["resize.Bicubic", dict(BICUBIC_TO_YUV)], avg(1, weights, True), ["resize.Bicubic", dict(BICUBIC_TO_RGB)]])
    nh = round((n - 1) / 2)
    offsets = [-(nh - i) for i in range(nh)] + [i + 1 for i in range(nh)]
    calls = [["resize.Bicubic", dict(BICUBIC_TO_YUV_DITHER)]]
    for d in offsets:
        calls += [["resize.Bicubic", dict(BICUBIC_TO_YUV)], avg(1, get_clip_frame_weights(d), False), ["resize.Bicubic", dict(BICUBIC_TO_RGB)],
                  ["std.ModifyFrame", dict(selector="color_frame", sat=sat, tht=tht, weight=weight, tht_scen=tht_scen, hue_adjust="none", return_mask=False,
                                           scenechange=False)],
                  ["resize.Bicubic", dict(BICUBIC_TO_YUV_DITHER)]]
    calls += [avg(n, weights, None), ["resize.Bicubic", dict(BICUBIC_TO_RGB)]]
    return dict(N=n, weights=weights, offsets=offsets, calls=calls)


def recover_rule(n, f_luma, weight):
    """color_frame (vsfilters.py:327-351, scenechange=False) -> None (the frame stays as it is) or the weight restore_color gets"""
    if n < BINARY_FIRST:
        return None
    if not (STANDARD_DARK <= f_luma <= STANDARD_BRIGHT):
        weight = min(weight, -0.8)
    return weight


def frame_params(sum_y, gray_count, n_pixels, weight, tht_scen):
    """what the library makes of a shifted frame's two sums (havc_chroma_stab_frame_params: the kernels' C++ on the host, no GPU) -> (weight, gate)"""
    from . import _native as nat
    out = (C.c_double * 2)()
    if nat.load().havc_chroma_stab_frame_params(int(sum_y), int(gray_count), int(n_pixels), float(weight), float(tht_scen), out) != 0:
        raise ValueError("havc_chroma_stab_frame_params: bad arguments")
    return out[0], bool(out[1])


# ---- the GPU path ------------------------------------------------------------------------------------------------------------------------------------------
def _prepare(clip, name):
    from .device import is_device
    from .tweak import MAX_SIDE
    if not is_device(clip):
        clip = np.asarray(clip)
    shape = tuple(clip.shape)
    if len(shape) != 4 or shape[-1] != 3 or (not is_device(clip) and clip.dtype != np.uint8) or min(shape) < 1:
        raise _err(f"{name}: only RGB24 clips (uint8 [n, h, w, 3]) are supported")
    if not is_device(clip):
        clip = np.ascontiguousarray(clip)
    return clip, shape, MAX_SIDE


def chroma_stab_np(ctx, clip, nframes=5, mode="A", sat=1.0, tht=0, weight=0.5, tht_scen=0.8, *, scenes=None, first_frame=0, flicker=False, chunk_frames=0):
    """vs_chroma_stabilizer_ex(hue_adjust='none', algo=0) [+ vs_reduce_flicker] through havc_chroma_stab_clip"""
    from . import _native as nat
    from .device import DeviceImage, is_device, operand_ptr
    name = "HAVC_stabilizer(stab=True)"
    n_w, weights = weight_list(nframes, mode)
    clip, shape, max_side = _prepare(clip, name)
    n, h, w, _ = shape
    if h % 2 or w % 2:
        raise _err(f"{name}: a frame of {w} x {h} cannot make the YUV420 round trip: width and height must be even (VapourSynth refuses it too)")
    if h > max_side or w > max_side:
        raise _err(f"{name}: frames of {w} x {h} are larger than {max_side} x {max_side}")
    if tht < 0 or tht > 255:
        raise _err(f"{name}: tht = {tht} must be in 0..255")
    p = nat.ChromaStabParams(width=w, height=h, n_frames=n, first_frame=int(first_frame), n_weights=n_w, sat=float(sat), tht=int(math.ceil(tht)),
                             flicker=int(bool(flicker)), weight=float(weight), tht_scen=float(tht_scen), chunk_frames=int(chunk_frames))
    for k, v in enumerate(weights):
        p.weights[k] = int(v)
    keep = []
    if scenes is not None:
        if len(scenes.scene_change_prev) != n or len(scenes.scene_change_next) != n:
            raise _err(f"{name}: scenes= must be the SceneInfo of this clip (AverageFrames reads _SceneChangePrev / _SceneChangeNext off every frame)")
        keep = [np.ascontiguousarray(np.asarray(a) != 0, dtype=np.uint8) for a in (scenes.scene_change_prev, scenes.scene_change_next)]
        p.scene_prev, p.scene_next = keep[0].ctypes.data, keep[1].ctypes.data
    out = DeviceImage(ctx, shape) if is_device(clip) else np.empty(shape, np.uint8)
    nat.check(ctx.lib.havc_chroma_stab_clip(ctx.h, operand_ptr(clip), operand_ptr(out), C.byref(p)), ctx.h)
    return out


def reduce_flicker_np(ctx, clip):
    """vs_reduce_flicker(strength=2, aggressive=0) (stand-in) through havc_reduce_flicker_clip"""
    from . import _native as nat
    from .device import DeviceImage, is_device, operand_ptr
    clip, shape, _ = _prepare(clip, "reduce_flicker")
    out = DeviceImage(ctx, shape) if is_device(clip) else np.empty(shape, np.uint8)
    nat.check(ctx.lib.havc_reduce_flicker_clip(ctx.h, operand_ptr(clip), operand_ptr(out), shape[2], shape[1], shape[0]), ctx.h)
    return out


def stab_stage_np(ctx, clip, stab_p, *, scenes=None, first_frame=0, chunk_frames=0):
    """the stab stage of HAVC_stabilizer (vsdeoldify/__init__.py:2834-2846, 2862-2866): stab_p unpacked as there; with a hue adjustment (stab_p[6]) the
    flicker pass runs behind it, as in the reference, otherwise inside the same call"""
    from . import imfilters as F
    nframes, mode, sat, tht, weight, tht_scen = stab_p[0], stab_p[1], stab_p[2], stab_p[3], stab_p[4], stab_p[5]
    hue_adjust = (stab_p[6] if len(stab_p) > 6 else "none").lower()
    if tht == 0 or hue_adjust in ("none", ""):                                                    # vs_clip_color_stabilizer's branch never sees hue_adjust
        return chroma_stab_np(ctx, clip, nframes, mode, sat, tht, weight, tht_scen, scenes=scenes, first_frame=first_frame, flicker=True,
                              chunk_frames=chunk_frames)
    out = chroma_stab_np(ctx, clip, nframes, mode, sat, tht, weight, tht_scen, scenes=scenes, first_frame=first_frame, flicker=False, chunk_frames=chunk_frames)
    from .device import is_device
    if is_device(out):                                                                            # vs_adjust_clip_hue(scenechange=False): every frame
        out = F.adjust_hue_range_np(ctx, out, hue_adjust)
    else:                                                                                         # per pixel: the clip as one tall image
        out = F.adjust_hue_range_np(ctx, out.reshape(-1, out.shape[2], 3), hue_adjust).reshape(out.shape)
    return reduce_flicker_np(ctx, out)
