"""HAVC_clip_overlay without VapourSynth (vsdeoldify/__init__.py:3029-3148) on RGB24 clips: an overlay placed at (x, y) of a base, one of nine blend modes, an
optional mask, an opacity, a set of planes.

The reference's Python -- the opacity clamp, the lower-cased mode, `planes`, the l / r / t / b crop and pad arithmetic (:3098-3109), the refusal texts -- is
restated in `overlay_plan`.  Everything that touches a sample there is native VapourSynth (std.Crop, std.AddBorders, std.Expr, std.MaskedMerge) and cannot be
executed where the fixtures are made: UNPINNED, tests/overlay_util.py is THE DEFINITION for this project and csrc/overlay.hip equals it byte for byte.  The
crop and pad values become the rectangle the kernel works in; no cropped or padded copy is made.  Where the reference would ask std.Crop for an empty clip -- the
overlay lies entirely outside the base -- a copy of the base comes back."""
import ctypes as C

import numpy as np

MODES = ["normal", "addition", "average", "difference", "divide", "exclusion", "multiply", "overlay", "subtract"]      # csrc/overlay_ops.h OverlayMode


def _err(msg):
    from .havc import HAVCError
    return HAVCError(msg)


def placement(base_w, base_h, ov_w, ov_h, x, y):
    """:3102-3109 -> dict(crop=(cl, cr, ct, cb), pad=(pl, pr, pt, pb), rect): what std.Crop takes off the overlay, what std.AddBorders puts around it, and the
    rectangle (x0, y0, x1, y1) of the base the cropped overlay covers, None when nothing of it is left"""
    l, r = x, base_w - ov_w - x
    t, b = y, base_h - ov_h - y
    cl, pl = min(l, 0) * -1, max(l, 0)
    cr, pr = min(r, 0) * -1, max(r, 0)
    ct, pt = min(t, 0) * -1, max(t, 0)
    cb, pb = min(b, 0) * -1, max(b, 0)
    inside = cl + cr < ov_w and ct + cb < ov_h
    return dict(crop=(cl, cr, ct, cb), pad=(pl, pr, pt, pb), rect=(pl, pt, base_w - pr, base_h - pb) if inside else None)


def overlay_plan(base_shape, overlay_shape, mask_shape=None, x=0, y=0, opacity=1.0, mode='normal', planes=None, mask_first_plane=True):
    """the arguments of HAVC_clip_overlay checked and normalised -> dict(n, base (w, h), overlay (w, h), overlay_frames, x, y, opacity, mode (index into MODES),
    plane_mask (bit k: plane k), mask_planes (0, 1, 3), mask_first_plane, placement)"""
    base_shape, overlay_shape = tuple(base_shape), tuple(overlay_shape)
    if len(base_shape) != 4 or base_shape[3] != 3 or min(base_shape) < 1:
        raise _err("mask_overlay: base must be an RGB24 clip [n, h, w, 3]")
    if len(overlay_shape) == 3:
        overlay_shape = (1,) + overlay_shape
    if len(overlay_shape) != 4 or overlay_shape[3] != 3 or min(overlay_shape) < 1 or overlay_shape[0] not in (1, base_shape[0]):
        raise _err("mask_overlay: overlay must be an RGB24 clip [n, h, w, 3] with the base's number of frames, or one frame [h, w, 3]")
    n, (oh, ow) = base_shape[0], overlay_shape[1:3]
    mask_planes = 0
    if mask_shape is not None:
        mask_shape = tuple(mask_shape)
        lead = mask_shape[:-3] if len(mask_shape) >= 3 and mask_shape[-1] == 3 and mask_shape[-3:-1] == (oh, ow) else mask_shape[:-2]
        body = mask_shape[len(lead):]
        if body not in ((oh, ow), (oh, ow, 3)):
            raise _err('mask_overlay: mask must have the same dimensions and bit depth as overlay')
        if (lead[0] if len(lead) == 1 else 1 if not lead else -1) != overlay_shape[0]:
            raise _err("mask_overlay: mask must have as many frames as overlay")
        mask_planes = 1 if len(body) == 2 else 3
    if not isinstance(mode, str) or mode.lower() not in MODES:
        raise _err('mask_overlay: invalid mode specified')
    if planes is None:
        planes = [0, 1, 2]
    elif isinstance(planes, (int, np.integer)):
        planes = [int(planes)]
    plane_mask = 0
    for k in planes:
        if k not in (0, 1, 2):
            raise _err(f"mask_overlay: plane {k!r}: an RGB24 clip has planes 0, 1 and 2")
        plane_mask |= 1 << int(k)
    x, y = int(x), int(y)
    if max(abs(x), abs(y)) >= 1 << 30:
        raise _err("mask_overlay: x and y must lie within +-2^30")
    return dict(n=n, base=(base_shape[2], base_shape[1]), overlay=(ow, oh), overlay_frames=overlay_shape[0], x=x, y=y,
                opacity=min(max(float(opacity), 0.0), 1.0), mode=MODES.index(mode.lower()), plane_mask=plane_mask, mask_planes=mask_planes,
                mask_first_plane=bool(mask_first_plane), placement=placement(base_shape[2], base_shape[1], ow, oh, x, y))


def overlay_np(ctx, base, overlay, mask, plan):
    """havc_overlay_clip with a plan of overlay_plan: one launch.  base decides the kind of the result: ndarray -> ndarray (the call blocks), DeviceImage ->
    DeviceImage (the call only enqueues); overlay and mask may be of either kind on their own"""
    from . import _native as nat
    from .device import DeviceImage, is_device, operand_ptr
    ops = [o if o is None or is_device(o) else np.ascontiguousarray(o, dtype=np.uint8) for o in (base, overlay, mask)]
    shape = tuple(base.shape)
    out = DeviceImage(ctx, shape) if is_device(base) else np.empty(shape, np.uint8)
    if plan["placement"]["rect"] is None:                                                         # nothing of the overlay is on the base
        if is_device(base):
            return out.copy_from(base)
        out[...] = ops[0]
        return out
    p = nat.OverlayParams(base_w=plan["base"][0], base_h=plan["base"][1], ov_w=plan["overlay"][0], ov_h=plan["overlay"][1], n_frames=plan["n"], x=plan["x"],
                          y=plan["y"], mode=plan["mode"], plane_mask=plan["plane_mask"], mask_planes=plan["mask_planes"],
                          mask_first_plane=1 if plan["mask_first_plane"] else 0, overlay_frames=plan["overlay_frames"], opacity=plan["opacity"])
    nat.check(ctx.lib.havc_overlay_clip(ctx.h, operand_ptr(ops[0]), operand_ptr(ops[1]), None if ops[2] is None else operand_ptr(ops[2]), operand_ptr(out),
                                        C.byref(p)), ctx.h)
    return out
