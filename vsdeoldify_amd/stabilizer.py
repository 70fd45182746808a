"""Per-frame bodies of the HAVC_stabilizer colour filters (`vs_dark_tweak`, `vs_chroma_bright_tweak`,
`vs_colormap`; vsdeoldify/vsslib/vsfilters.py:525-641) on uint8 HWC frames, backed by the HIP filters.  The VapourSynth wrappers
(ModifyFrame plumbing, scene-change passthrough) stay in the reference; these are the functions their selectors call per frame."""
import numpy as np

from . import _native as nat
from . import imfilters as F
from .device import DeviceImage, is_device, operand_ptr
from .render import get_context


def _luma_merge_mode(lo, hi):
    """(mode, tresh, grad) of havc_image_luma_merge for the merge the filters end in -- image_luma_merge when the limits are equal (imfilters.py:66-77),
    else w_image_luma_merge (imfilters.py:80-100 with w_np_rgb_to_gray's threshold / gradient arithmetic, nputils.py:141-183); mode -1: no merge, the
    tweaked frame is the result (w_image_luma_merge returns img_dark, imfilters.py:84-85)"""
    if lo == hi:
        return (0, round(lo * 255), 0.0) if lo > 0 else (3, 0.0, 0.0)
    if lo >= hi:
        return -1, 0.0, 0.0
    if lo > 0:
        max_white = round(hi * 255)
        tresh = min(round(lo * 255), max_white - 10)
        return 1, tresh, round(1 / (max_white - tresh), 3)
    return 2, 0.0, 0.0


def _luma_merge(ctx, img2, img1, lo, hi):
    mode, tresh, grad = _luma_merge_mode(lo, hi)
    return np.asarray(img2) if mode < 0 else F.luma_merge_np(ctx, img2, img1, mode, tresh, grad)


def dark_tweak_frame(img, dark_threshold=0.3, dark_amount=0.8, dark_hue_adjust="none", device_index=0):
    """vs_sc_dark_tweak (vsfilters.py:600-632): darker, less saturated copy merged in where the luma is low."""
    ctx = get_context(device_index)
    white = min(max(dark_threshold, 0.1), 0.50)
    d_sat = min(max(1.1 - dark_amount, 0.10), 0.80)
    d_bright = -min(max(dark_amount, 0.20), 0.90)
    img = np.asarray(img)
    return _luma_merge(ctx, F.image_tweak_np(ctx, img, sat=d_sat, bright=d_bright, hue_range=dark_hue_adjust), img, 0.1, white)


def chroma_bright_tweak_frame(img, black_threshold=0.3, white_threshold=0.6, dark_sat=0.8, dark_bright=-0.10, chroma_adjust="none",
                              device_index=0):
    """vs_sc_chroma_bright_tweak (vsfilters.py:525-547)."""
    ctx = get_context(device_index)
    img = np.asarray(img)
    return _luma_merge(ctx, F.image_chroma_tweak_np(ctx, img, sat=dark_sat, bright=dark_bright, hue_adjust=chroma_adjust), img,
                       black_threshold, white_threshold)


def colormap_frame(img, colormap="none", device_index=0):
    """_vs_sc_colormap (vsfilters.py:575-590): direct colour mapping through the "chroma adjustment" string."""
    return F.image_chroma_tweak_np(get_context(device_index), np.asarray(img), hue_adjust=colormap)


# ---- the three filters above as ONE launch over a clip (csrc/stabilizer.hip) -------------------------------------------------------------------
def _dark_stage(threshold, amount, hue_range="none"):
    """vs_sc_dark_tweak (vsfilters.py:609-636) as a stage record: the clamps of dark_tweak_frame, the argument conversion of imfilters.image_tweak_np"""
    white = min(max(threshold, 0.1), 0.50)
    d_sat = min(max(1.1 - amount, 0.10), 0.80)
    d_bright = -min(max(amount, 0.20), 0.90)
    st = nat.StabStage(kind=0, brightness=float(1 + d_bright / 255), color=float(d_sat))
    rng = [] if hue_range in ("none", "") else F.parse_hue_ranges(hue_range)
    _set_ranges(st, rng)
    st.merge_mode, st.tresh, st.grad = _luma_merge_mode(0.1, white)
    return st


def _chroma_stage(sat=1, bright=0, hue_adjust="none", limits=None):
    """image_chroma_tweak (imfilters.py:540-548) [+ the luma merge of vs_sc_chroma_bright_tweak, vsfilters.py:537-541] as a stage record: the
    argument conversion of imfilters.image_chroma_tweak_np"""
    st = nat.StabStage(kind=1, sat=float(sat), bright=float(bright), adj_sat=1.0)
    st.identity = int(sat == 1 and bright == 0 and hue_adjust == "none")                     # restcolor.py:290-291
    param = None if hue_adjust in ("none", "") else F.parse_hue_adjust(hue_adjust)
    if param:
        _set_ranges(st, F.parse_hue_ranges(param[0]))
        st.has_adjust, st.adj_sat, st.adj_hue, st.adj_weight = 1, float(param[1]), int(param[2]), float(param[3])
    st.merge_mode, st.tresh, st.grad = _luma_merge_mode(*limits) if limits else (-1, 0.0, 0.0)
    return st


def _set_ranges(st, rng):
    if len(rng) > 16:
        raise ValueError("at most 8 hue ranges")
    st.n_ranges = len(rng) // 2
    for i, v in enumerate(rng):
        st.hue_ranges[i] = v


def stabilize_np(ctx, clip, dark=None, smooth=None, colormap=None, order=("dark", "smooth", "colormap")):
    """HAVC_stabilizer's filters (vsdeoldify/__init__.py:2850-2860) on a frame [h, w, 3] or a clip [n, h, w, 3], ndarray or DeviceImage, in one launch:
         dark     = (dark_threshold, dark_amount[, hue range])                       -> dark_tweak_frame
         smooth   = (black, white, dark_sat, dark_bright[, chroma adjust])           -> chroma_bright_tweak_frame (dark_bright as the filter takes it: <= 0)
         colormap = "chroma adjustment" string                                        -> colormap_frame
    in that order (`order`: HAVC_deepex runs colormap first, __init__.py:1679-1689), None = off; the bytes are those of the three functions called one after the other.  ndarray -> ndarray (blocks), DeviceImage ->
    DeviceImage (only enqueues)."""
    made = {}
    if dark is not None:
        made["dark"] = _dark_stage(*dark)
    if smooth is not None:
        made["smooth"] = _chroma_stage(smooth[2], smooth[3], smooth[4] if len(smooth) > 4 else "none", (smooth[0], smooth[1]))
    if colormap is not None and colormap != "none":
        made["colormap"] = _chroma_stage(hue_adjust=colormap)
    stages = [made[k] for k in order if k in made]
    if is_device(clip):
        a, out = clip, DeviceImage(ctx, clip.shape)
    else:
        a = np.ascontiguousarray(clip, dtype=np.uint8)
        if a.ndim not in (3, 4) or a.shape[-1] != 3:
            raise ValueError("not an RGB frame or clip")
        out = np.empty_like(a)
    arr = (nat.StabStage * max(len(stages), 1))(*stages)
    nat.check(ctx.lib.havc_stabilizer_chain(ctx.h, operand_ptr(a), operand_ptr(out), a.shape[-2], int(np.prod(a.shape[:-2])), arr, len(stages)), ctx.h)
    return out
