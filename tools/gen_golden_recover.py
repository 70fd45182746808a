#!/usr/bin/env python3
"""Golden vectors for HAVC_recover_clip_color by EXECUTING the reference (build container only).  Writes tests/golden/recover.npz (data only): the input
clips, the parameter sets and the outputs of the reference's own ChromaRetentionMerge (vsdeoldify/vsslib/mcomb.py:450-516, what HAVC_recover_clip_color,
vsdeoldify/__init__.py:2956-2992, calls with strength -> clipb_weight and scenechange=False), imported through tools/refshim.py and run on stand-in clip and
frame classes:

  * std.ModifyFrame drives the reference's own selectors frame by frame with the frame number n: color_grad_frame (vsslib/vsfilters.py:391-412), color_frame
    (:327-351) and copy_luma_frame (:863-893), which call the reference's restore_color_gradient / restore_color (vsslib/restcolor.py), get_image_luma and
    chroma_post_process (vsslib/imfilters.py) and nputils' merges -- all executed, with real numpy and Pillow;
  * resize.Spline64 is oracle/resample.py's Spline64, and every call's target size is recorded;
  * std.Merge is the restatement the project already uses for it (oracle/imaging.py pil_blend: Image.blend's float32 truncating blend);
  * cv2.cvtColor is oracle/cvcolor.py's.

What the fixture pins: the selector logic of both paths, the routing of ChromaRetentionMerge's arguments into them (mask_weight -> weight, the clamp of alpha,
tht_scen = 1.0, hue_adjust 'none'), the luma gate DEF_STANDARD_DARK <= f_luma <= DEF_STANDARD_BRIGHT, the weight and alpha overrides outside it, the binary
selector's `n < 15` rule, the resize-size rule (rf capped at 48; `size_table`: the sizes the reference asks Spline64 for at widths up to 3840, recorded by
running it on clips WITHOUT frames), and the fact that return_mask skips both the resize and the merge.  ChromaRetentionMerge does not hand `algo` on to
its selector (mcomb.py:503-504): the reference runs algorithm 0 whatever is asked, so every case here has algo = 0.
What it does not pin: cv2's colour conversion and zimg's resize (both stand-ins, as elsewhere here), and std.Merge.

Frames are at most 272 x 16 (the resize case: 272 is the smallest width the size rule shrinks, to 256 x 256) and 16 x 8 for the 17-frame binary clips.
"""
import importlib
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import refshim  # noqa: E402

refshim.install()
vs = sys.modules["vapoursynth"]
for i, n in enumerate(("DEBUG", "INFORMATION", "WARNING", "CRITICAL", "FATAL")):
    setattr(vs, "MESSAGE_TYPE_" + n, i)
from oracle import imaging, resample  # noqa: E402

SIZES = []                                             # (width, height) of every resize.Spline64 call, in call order


class Frame:
    """three writable u8 planes + props: the part of vs.VideoFrame the selectors touch"""
    format = types.SimpleNamespace(num_planes=3)

    def __init__(self, rgb):
        self.planes, self.props = [np.array(rgb[:, :, k]) for k in range(3)], {}

    def __getitem__(self, i):
        return self.planes[i]

    def copy(self):
        return Frame(self.rgb())

    def rgb(self):
        return np.dstack(self.planes)


class Clip:
    def __init__(self, frames, width, height):
        self.frames, self.num_frames, self.width, self.height = list(frames), len(frames), width, height
        self.std = types.SimpleNamespace(ModifyFrame=self._modify)
        self.resize = types.SimpleNamespace(Spline64=self._spline64)

    @classmethod
    def of(cls, arr):
        return cls([Frame(f) for f in arr], arr.shape[2], arr.shape[1])

    def array(self):
        return np.stack([f.rgb() for f in self.frames])

    def _modify(self, clips, selector):
        clips = clips if isinstance(clips, (list, tuple)) else [clips]
        return Clip([selector(n, [c.frames[n] for c in clips]) for n in range(self.num_frames)], self.width, self.height)

    def _spline64(self, width, height):
        SIZES.append((int(width), int(height)))
        return Clip([Frame(resample.resize_rgb8(f.rgb(), width, height)) for f in self.frames], width, height)


def _merge(clipa, clipb, weight):
    return Clip([Frame(imaging.pil_blend(a.rgb(), b.rgb(), weight)) for a, b in zip(clipa.frames, clipb.frames)], clipa.width, clipa.height)


vs.core.std = types.SimpleNamespace(Merge=_merge)
mc = importlib.import_module("vsdeoldify.vsslib.mcomb")

rng = np.random.default_rng(20261020)


def frame_at(level, shape, gray_share=0.5):
    """a frame around `level`: a share of (almost) gray pixels, the rest coloured"""
    h, w = shape
    base = level + 18.0 * rng.standard_normal((h, w, 1))
    tint = rng.integers(-60, 61, (h, w, 3)) * (rng.random((h, w, 1)) > gray_share) + rng.integers(-4, 5, (h, w, 3))
    return np.clip(base + tint, 0, 255).astype(np.uint8)


def donor(shape):
    h, w = shape
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    c = np.stack([128 + 110 * np.sin(xx / 3.0 + yy / 5.0), 128 + 110 * np.cos(yy / 2.0 - xx / 7.0), 128 + 110 * np.sin((xx + yy) / 4.0 + 1.0)], -1)
    return np.clip(c + 10 * rng.standard_normal((h, w, 3)), 0, 255).astype(np.uint8)


def run(a, b, **kw):
    del SIZES[:]
    out = mc.ChromaRetentionMerge(clip_a=Clip.of(a), clip_b=Clip.of(b), scenechange=False, **kw)
    return out.array(), list(SIZES)


fx = {"provenance": np.array("generated by tools/gen_golden_recover.py executing the reference: vsdeoldify/vsslib/mcomb.py ChromaRetentionMerge with "
                             "vsslib/vsfilters.py vs_sc_recover_gradient_color / vs_sc_recover_clip_color / vs_sc_recover_clip_luma / vs_simple_merge "
                             "(selector bodies included), vsslib/restcolor.py restore_color_gradient / restore_color; cv2 = oracle.cvcolor, "
                             "resize.Spline64 = oracle.resample, std.Merge = oracle.imaging.pil_blend stand-ins")}

# ---- the clips ----
LEVELS_G = [120, 90, 30, 225]                                                # two frames inside the luma band, one dark, one bright
fx["clip_g"] = np.stack([frame_at(v, (16, 24)) for v in LEVELS_G])
fx["color_g"] = np.stack([donor((16, 24)) for _ in LEVELS_G])
fx["clip_r"] = np.stack([frame_at(v, (8, 272)) for v in (110, 35)])        # 272 wide: resized to 256 x 256
fx["color_r"] = np.stack([donor((8, 272)) for _ in range(2)])
levels_b = [40 + 10 * k for k in range(15)] + [130, 232]                     # frames 15 (inside the band) and 16 (bright) are the processed ones
fx["clip_b"] = np.stack([frame_at(v, (8, 16)) for v in levels_b])
fx["color_b"] = np.stack([donor((8, 16)) for _ in levels_b])
levels_b2 = [200 - 10 * k for k in range(15)] + [25, 128]                    # frame 15 dark
fx["clip_b2"] = np.stack([frame_at(v, (8, 16)) for v in levels_b2])
fx["color_b2"] = np.stack([donor((8, 16)) for _ in levels_b2])

cases = []
for mw in (1.0, 0.0, -0.3):
    for sat in (0.8, 1.0):
        for alpha in (2.0, 6.0):
            cases.append(dict(clip="g", sat=sat, tht=30, clipb_weight=1.0, alpha=alpha, mask_weight=mw, chroma_resize=False))
cases += [
    dict(clip="g", sat=0.8, tht=30, clipb_weight=0.9, alpha=2.0, mask_weight=0.0, chroma_resize=True),          # ChromaRetentionMerge's own defaults; 24 wide: no resize
    dict(clip="g", sat=0.6, tht=50, clipb_weight=0.5, alpha=0.25, mask_weight=0.4, chroma_resize=False),        # alpha clamped to 1
    dict(clip="g", sat=1.3, tht=12, clipb_weight=0.3, alpha=14.0, mask_weight=-0.7, chroma_resize=False),       # alpha clamped to 10
    dict(clip="g", sat=0.8, tht=30, clipb_weight=0.9, alpha=2.0, mask_weight=0.0, chroma_resize=False, return_mask=True),
    dict(clip="g", sat=0.8, tht=30, clipb_weight=0.9, alpha=3.0, mask_weight=1.0, chroma_resize=True, return_mask=True, binary_mask=True),
    dict(clip="r", sat=0.8, tht=30, clipb_weight=1.0, alpha=2.0, mask_weight=1.0, chroma_resize=True),          # HAVC_recover_clip_color's defaults
    dict(clip="r", sat=0.8, tht=30, clipb_weight=0.5, alpha=2.0, mask_weight=0.0, chroma_resize=True),
    dict(clip="r", sat=0.8, tht=30, clipb_weight=1.0, alpha=2.0, mask_weight=1.0, chroma_resize=True, return_mask=True),     # no resize, no merge
    dict(clip="r", sat=0.9, tht=40, clipb_weight=0.7, alpha=2.0, mask_weight=-0.2, chroma_resize=False),
]
for name in ("b", "b2"):
    for mw in (1.0, 0.0, -0.4):
        cases.append(dict(clip=name, sat=0.8, tht=30, clipb_weight=1.0, alpha=2.0, mask_weight=mw, chroma_resize=False, binary_mask=True))
cases += [
    dict(clip="b", sat=1.0, tht=60, clipb_weight=0.6, alpha=2.0, mask_weight=0.3, chroma_resize=True, binary_mask=True),    # 16 wide: no resize
    dict(clip="b2", sat=0.8, tht=30, clipb_weight=1.0, alpha=2.0, mask_weight=1.0, chroma_resize=False, binary_mask=True, return_mask=True),
]
for i, c in enumerate(cases):
    kw = {k: v for k, v in c.items() if k != "clip"}
    out, sizes = run(fx["clip_" + c["clip"]], fx["color_" + c["clip"]], **kw)
    fx[f"out_{i}"] = out
    fx[f"sizes_{i}"] = np.array(sizes, dtype=np.int32).reshape(-1, 2)
fx["cases"] = np.array([json.dumps(c) for c in cases])

# ---- the size rule: the reference on clips of a given width and NO frames; what it asks Spline64 for, or nothing ----
table = []
for width in (256, 272, 640, 704, 1280, 1920, 3840):
    del SIZES[:]
    empty = Clip([], width, width * 9 // 16)
    mc.ChromaRetentionMerge(clip_a=empty, clip_b=Clip([], width, width * 9 // 16), chroma_resize=True)
    down = [s for s in SIZES if s != (width, width * 9 // 16)]
    assert len(SIZES) in (0, 3) and len(set(down)) <= 1, SIZES
    table.append((width, down[0][0] if down else 0))
fx["size_table"] = np.array(table, dtype=np.int32)                           # (W, fs); fs = 0: no resize

path = os.path.join(ROOT, "tests", "golden", "recover.npz")
np.savez_compressed(path, **fx)
print("wrote recover.npz", os.path.getsize(path), "bytes;", len(cases), "cases; size table", table)
