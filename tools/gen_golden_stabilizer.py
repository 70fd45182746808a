#!/usr/bin/env python3
"""Golden vectors for HAVC_stabilizer's colour filters (vsdeoldify/__init__.py:2748-2873) by EXECUTING the reference (build container only; cv2 = the
stand-in of tools/refshim.py, recorded as provenance).  Writes tests/golden/stabilizer.npz (data only):

  * colormap_in / colormap_out: havc_utils._get_colormap(name) (havc_utils.py:552-581, ColorTune = "light") for its twelve names and two strings it
    hands on unchanged.  havc_utils imports under the shim once the vapoursynth stand-in carries the MESSAGE_TYPE_* constants vsutils.MessageType reads
    (set below; they are never used on this path).
  * chain cases: vs_dark_tweak -> vs_chroma_bright_tweak -> vs_colormap (vsslib/vsfilters.py:525-641), called with the parameters unpacked as
    HAVC_stabilizer unpacks them (__init__.py:2806-2832) and in its order (:2850-2860).  The three functions are the reference's own, selector bodies
    included: they run on a stand-in clip whose std.ModifyFrame applies the selector to one frame of three numpy planes (what frame_to_image /
    image_to_frame of vsslib/vsutils.py read and write).  The Spline64 squash and _clip_chroma_resize around them are zimg: not executed here.
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
for i, n in enumerate(("DEBUG", "INFORMATION", "WARNING", "CRITICAL", "FATAL")):
    setattr(sys.modules["vapoursynth"], "MESSAGE_TYPE_" + n, i)
hu = importlib.import_module("vsdeoldify.havc_utils")
vf = importlib.import_module("vsdeoldify.vsslib.vsfilters")


class Frame:
    """three writable u8 planes + props: the part of vs.VideoFrame the selectors touch"""
    format = types.SimpleNamespace(num_planes=3)

    def __init__(self, planes):
        self.planes, self.props = [np.array(p) for p in planes], {}

    def __getitem__(self, i):
        return self.planes[i]

    def copy(self):
        return Frame(self.planes)


class Clip:
    """one-frame clip; std.ModifyFrame(clips, selector) -> the clip of selector(0, frame)"""
    def __init__(self, frame):
        self.frame = frame
        self.std = types.SimpleNamespace(ModifyFrame=lambda clips, selector: Clip(selector(0, clips.frame)))


def chain(img, dark=False, dark_p=(0.2, 0.8), smooth=False, smooth_p=(0.3, 0.7, 0.9, 0.0, "none"), colormap="none"):
    clip = Clip(Frame([img[:, :, c] for c in range(3)]))
    dark_hue_adjust = dark_p[2] if len(dark_p) > 2 else "none"                                  # __init__.py:2806-2813
    chroma_adjust = smooth_p[4] if len(smooth_p) > 4 else "none"                                # :2815-2824
    colormap = colormap.lower()                                                                 # :2827-2832
    colormap_enabled = colormap != "none" and colormap != ""
    colormap_adjust = hu._get_colormap(colormap) if colormap_enabled else "none"
    if dark:                                                                                    # :2850-2860
        clip = vf.vs_dark_tweak(clip, dark_threshold=dark_p[0], dark_amount=dark_p[1], dark_hue_adjust=dark_hue_adjust.lower())
    if smooth:
        clip = vf.vs_chroma_bright_tweak(clip, black_threshold=smooth_p[0], white_threshold=smooth_p[1], dark_sat=smooth_p[2],
                                         dark_bright=-smooth_p[3], chroma_adjust=chroma_adjust.lower())
    if colormap_enabled:
        clip = vf.vs_colormap(clip, colormap=colormap_adjust)
    return np.dstack(clip.frame.planes)


names = ['none', 'blue->brown', 'blue->red', 'blue->green', 'green->brown', 'green->red', 'green->blue', 'redrose->brown', 'redrose->blue',
         'red->brown', 'red->blue', 'yellow->rose', '30:90|+300,0.5', 'cyan,blue|0.6,0.2']
r = np.random.default_rng(2024)
h, w = 54, 96
yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
colour = np.stack([128 + 110 * np.sin(xx / 7.0 + yy / 23.0), 128 + 110 * np.cos(yy / 5.0 - xx / 31.0), 128 + 110 * np.sin((xx + yy) / 9.0 + 1.0)], -1)
level = (0.04 + 0.96 * xx / (w - 1))[..., None] ** 1.5                                          # dark on the left: every luma mask has both sides
img = np.clip(colour * level + 6 * r.standard_normal((h, w, 3)), 0, 255).astype(np.uint8)
cases = [
    dict(dark=True, dark_p=[0.2, 0.8], smooth=True, smooth_p=[0.3, 0.7, 0.9, 0.0, "none"], colormap="red->brown"),    # preset medium
    dict(dark=True, dark_p=[0.35, 0.6, "280:360,0:30"]),                                                                # dark with a hue range
    dict(smooth=True, smooth_p=[0.4, 0.4, 0.6, 0.25, "red|0.5,0.0"]),                                                   # black == white: hard mask
    dict(smooth=True, smooth_p=[0.7, 0.3, 0.8, 0.1, "none"], colormap="blue->brown"),                                   # black > white: no merge
    dict(colormap="blue->brown"),                                                                                       # presets fast .. veryfast
    dict(dark=True, dark_p=[0.05, 1.0], smooth=True, smooth_p=[0.0, 0.6, 0.8, 0.2, "green|0.2,-0.4"], colormap="30:90|+300,0.5"),
    dict(smooth=True, smooth_p=[0.0, 0.0, 0.7, 0.15]),                                                                  # both limits 0: mask = luma
    dict(dark=True, dark_p=[0.5, 0.3, "Orange,Yellow"], smooth=True, smooth_p=[0.3, 0.7, 1.0, 0.0, "none"], colormap="Yellow->Rose"),
    dict(),                                                                                                             # everything off
]
fx = {"provenance": np.array("generated by tools/gen_golden_stabilizer.py executing the reference: vsdeoldify/havc_utils.py _get_colormap and "
                             "vsslib/vsfilters.py vs_dark_tweak / vs_chroma_bright_tweak / vs_colormap; cv2 = oracle.cvcolor stand-in"),
      "colormap_in": np.array(names), "colormap_out": np.array([hu._get_colormap(n) for n in names]),
      "img": img, "cases": np.array([json.dumps(c) for c in cases])}
for i, c in enumerate(cases):
    fx[f"out_{i}"] = chain(img, **c)
np.savez_compressed(os.path.join(ROOT, "tests", "golden", "stabilizer.npz"), **fx)
print("wrote stabilizer.npz", [int((fx[f"out_{i}"] != img).any(-1).sum()) for i in range(len(cases))], dict(zip(names, fx["colormap_out"])))
