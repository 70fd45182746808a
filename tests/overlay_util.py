"""THE DEFINITION of the native filters under HAVC_clip_overlay (vsdeoldify/__init__.py:3029-3148), in numpy: csrc/overlay.hip equals `clip_overlay` byte for
byte.

UNPINNED: std.Crop, std.AddBorders, std.Expr and std.MaskedMerge are native VapourSynth and cannot be executed where the fixtures are made.  This file does
what the reference's calls say, in their order, on RGB24 clips: the overlay and the mask are cropped and padded to the base's size (the mask's borders are 0, so
the base comes through there); with opacity < 1 the mask becomes expr8(m * float32(opacity)); the blend expression is evaluated in float32 in the RPN order of
the reference's string, one rounding per operation, IEEE division, peak 255 and neutral 128, and stored through expr8; std.MaskedMerge is the project's
stand-in, out = (base * (255 - m) + o * m + 127) // 255 (tests/tiles_util.masked_merge).  Assumptions, all of them this file's: std.Expr stores to 8 bit as
(int)(min(max(v, 0), 255) + 0.5), and its float is float32."""
import numpy as np

from tests.tiles_util import masked_merge

f32 = np.float32
MODES = ["normal", "addition", "average", "difference", "divide", "exclusion", "multiply", "overlay", "subtract"]


def expr8(v):
    return (np.minimum(np.maximum(v.astype(f32), f32(0)), f32(255)) + f32(0.5)).astype(f32).astype(np.int64).astype(np.uint8)


def blend(mode, x, y):
    """x = overlay, y = base, uint8 arrays -> uint8"""
    if mode == "normal":
        return x
    x, y, peak = x.astype(f32), y.astype(f32), f32(255)
    with np.errstate(divide="ignore", invalid="ignore"):
        if mode == "addition":
            v = x + y
        elif mode == "average":
            v = (x + y) / f32(2)
        elif mode == "difference":
            v = np.abs(x - y)
        elif mode == "divide":
            v = np.where(y <= 0, peak, (peak * x) / np.where(y <= 0, f32(1), y))
        elif mode == "exclusion":
            v = (x + y) - ((f32(2) * x) * y) / peak
        elif mode == "multiply":
            v = (x * y) / peak
        elif mode == "overlay":
            v = np.where(x < f32(128), f32(2) * ((x * y) / peak), peak - f32(2) * (((peak - x) * (peak - y)) / peak))
        elif mode == "subtract":
            v = x - y
        else:
            raise ValueError("mask_overlay: invalid mode specified")
    return expr8(v)


def clip_overlay(base, overlay, x=0, y=0, mask=None, opacity=1.0, mode="normal", planes=None, mask_first_plane=True):
    """base [n, H, W, 3]; overlay [n, h, w, 3] or [h, w, 3]; mask None, [n, h, w], [n, h, w, 3] (or one frame of either with a one-frame overlay)"""
    base = np.asarray(base, np.uint8)
    n, H, W, _ = base.shape
    overlay = np.asarray(overlay, np.uint8)
    if overlay.ndim == 3:
        overlay = overlay[None]
    h, w = overlay.shape[1:3]
    if mask is None:
        mask = np.full((1, h, w, 1), 255, np.uint8)
    else:
        mask = np.asarray(mask, np.uint8)
        gray = mask.shape[-2:] == (h, w) and not (mask.ndim >= 3 and mask.shape[-1] == 3 and mask.shape[-3:-1] == (h, w))
        if gray:
            mask = mask[..., None]
        if mask.ndim == 3:
            mask = mask[None]
        if mask_first_plane:
            mask = mask[..., :1]
    overlay = np.broadcast_to(overlay, (n,) + overlay.shape[1:])
    mask = np.broadcast_to(mask, (n, h, w, 3))
    opacity = min(max(opacity, 0.0), 1.0)
    mode = mode.lower()
    planes = [0, 1, 2] if planes is None else ([planes] if isinstance(planes, int) else list(planes))
    # std.Crop + std.AddBorders of :3102-3115: the rectangle of the base the overlay covers, and the part of the overlay that lands there
    x0, y0, x1, y1 = max(x, 0), max(y, 0), min(x + w, W), min(y + h, H)
    ov_full = np.zeros_like(base)
    m_full = np.zeros(base.shape, np.uint8)
    if x1 > x0 and y1 > y0:
        ov_full[:, y0:y1, x0:x1] = overlay[:, y0 - y:y1 - y, x0 - x:x1 - x]
        m_full[:, y0:y1, x0:x1] = mask[:, y0 - y:y1 - y, x0 - x:x1 - x]
    if opacity < 1:
        m_full = expr8(m_full.astype(f32) * f32(opacity))
    blended = blend(mode, ov_full, base)
    merged = masked_merge(base, blended, m_full.astype(np.int64))
    out = base.copy()
    for k in planes:
        out[..., k] = merged[..., k]
    return out


def make_clip(n, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def pair_sweep():
    """every (overlay sample, base sample) pair as frames of 256 x 256: overlay[i][j] = i, base[i][j] = j, on all three planes"""
    i, j = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    return np.stack([j] * 3, -1)[None].copy(), np.stack([i] * 3, -1)[None].copy()                 # base, overlay
