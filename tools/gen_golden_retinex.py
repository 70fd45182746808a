#!/usr/bin/env python3
"""Golden vectors for HAVC_retinex by EXECUTING the reference (build container only).  Writes tests/golden/retinex.npz (data only).

What runs: the reference's own HAVC_retinex (vsdeoldify/__init__.py:1073-1101; the package's __init__ needs VapourSynth and every model, so the function is
taken out of that file's syntax tree at run time and compiled in a namespace that holds the reference's constants, convert_format_RGB24 and restore_format
of vsdeoldify/havc_utils.py) -> vs_retinex -> vs_retinex_fast (vsslib/vsretinex.py:25-88) with its selector body filter_retinex, get_image_luma and
image_luma_blend (vsslib/imfilters.py) with real Pillow, frame_to_image / image_to_frame (vsslib/vsutils.py).  cv2.cvtColor is oracle/cvcolor.py's.

Stand-ins (tools/refshim.py plus the classes below):
  * core.retinex.MSRCP -- the Retinex plugin, which is not in the reference tree -- records its keyword arguments and hands out a PRESCRIBED frame: the
    plugin's output is an INPUT of the fixture (case_<i>_rtx), exactly as tools/gen_golden_equalize.py prescribes the CLAHE plane;
  * std.ModifyFrame drives filter_retinex frame by frame; the clip is RGB24 with the frame props convert_format_RGB24 looks at.
Recorded per case: the input frame, the prescribed frame, the output, the arguments, the keyword arguments the plugin got, whether the selector looked at the
plugin's frame (= the gate), and the weight Image.blend was called with (-1: not called).

What this pins: the gate on both sides of each bound and at equality, the f_luma roundings for range_tv_in on / off, the blend weight below 0.40 (the min_w
floor included) and its absence at / above 0.40 or with blend off, Pillow's blend, that a gated-out frame is the input whatever range_tv_out is, and the
forwarding of sigmas / thresholds / fulls / fulld / chroma_protect.  Frames are at most 24 x 40.
"""
import ast
import enum
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
vs.RGB24, vs.YUV, vs.GRAY, vs.RGB = 1, 3, 1000, 2000


class MatrixCoefficients(enum.IntEnum):
    MATRIX_RGB, MATRIX_BT709, MATRIX_UNSPECIFIED, MATRIX_BT470_BG = 0, 1, 2, 5


class Range(enum.IntEnum):
    RANGE_FULL, RANGE_LIMITED = 0, 1


vs.MatrixCoefficients, vs.Range, vs.ColorRange = MatrixCoefficients, Range, Range
vs.MATRIX_BT709, vs.RANGE_FULL, vs.RANGE_LIMITED = MatrixCoefficients.MATRIX_BT709, Range.RANGE_FULL, Range.RANGE_LIMITED
vs.core.core_version = types.SimpleNamespace(release_major=74)
vs.core.log_message = lambda *a: None

PLUGIN_CALLS, PRESCRIBED = [], []


def _msrcp(**kw):
    clip = kw.pop("input")
    PLUGIN_CALLS.append(kw)
    assert len(PRESCRIBED) == clip.num_frames
    return Clip([Frame(p) for p in PRESCRIBED])


vs.core.retinex = types.SimpleNamespace(MSRCP=_msrcp)


class Frame:
    """three writable u8 planes + props: the part of vs.VideoFrame the selector touches"""
    format = types.SimpleNamespace(num_planes=3)

    def __init__(self, rgb):
        self.planes = [np.array(rgb[:, :, k]) for k in range(3)]
        self.props = {"_Matrix": int(vs.MATRIX_BT709), "_Range": int(vs.RANGE_FULL)}

    def __getitem__(self, i):
        return self.planes[i]

    def copy(self):
        return Frame(self.rgb())

    def rgb(self):
        return np.dstack(self.planes)


class Clip:
    format = types.SimpleNamespace(id=vs.RGB24, color_family=vs.RGB, bits_per_sample=8)

    def __init__(self, frames):
        self.frames, self.num_frames = list(frames), len(frames)
        self.height, self.width = frames[0].planes[0].shape
        self.std = types.SimpleNamespace(ModifyFrame=self._modify, SetFrameProps=lambda **kw: self)

    def get_frame(self, n):
        return self.frames[n]

    def _modify(self, clips, selector):
        return Clip([selector(n, [c.frames[n] for c in clips]) for n in range(self.num_frames)])


hu = importlib.import_module("vsdeoldify.havc_utils")
rx = importlib.import_module("vsdeoldify.vsslib.vsretinex")
constants = importlib.import_module("vsdeoldify.vsslib.constants")
from PIL import Image  # noqa: E402

# HAVC_retinex itself, out of the reference's __init__.py (module docstring)
init_path = os.path.join(refshim.REF_ROOT, "vsdeoldify", "__init__.py")
tree = ast.parse(open(init_path).read(), init_path)
fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "HAVC_retinex"]
assert len(fn) == 1
future = ast.ImportFrom(module="__future__", names=[ast.alias(name="annotations")], level=0)
ns = dict(vs=vs, constants=constants, convert_format_RGB24=hu.convert_format_RGB24, restore_format=hu.restore_format, vs_retinex=rx.vs_retinex)
exec(compile(ast.fix_missing_locations(ast.Module(body=[future, fn[0]], type_ignores=[])), init_path, "exec"), ns)
HAVC_retinex = ns["HAVC_retinex"]

# instrumentation: how often the selector turns a frame into an image (2 = it looked at the plugin's frame), and what Image.blend is called with
LOOKS, WEIGHTS = [], []
_f2i, _blend = rx.frame_to_image, Image.blend
rx.frame_to_image = lambda f: (LOOKS.append(1), _f2i(f))[1]
Image.blend = lambda a, b, w: (WEIGHTS.append(float(w)), _blend(a, b, w))[1]

rng = np.random.default_rng(20261021)


def frame_at(level, shape):
    f = level + 14.0 * rng.standard_normal(shape + (3,)) + rng.integers(-20, 21, 3)
    return np.clip(f, 0, 255).astype(np.uint8)


def prescribe(img):
    """a 'plugin output': the input stretched and shaken so that no blend or copy can be mistaken for it"""
    m = img.astype(np.float64).mean()
    p = (img.astype(np.float64) - m) * 3.0 + m + 25.0 + rng.integers(-12, 13, img.shape)
    return np.clip(p, 0, 255).astype(np.uint8)


def luma_of(img, range_tv):
    """the reference's own f_luma of a frame (vsretinex.py:68-73)"""
    pil = Image.fromarray(img, "RGB")
    return max(rx.get_image_luma(pil, 235) - 0.07, 0) if range_tv else rx.get_image_luma(pil, 255)


SHAPES = [(24, 40), (16, 24), (9, 11), (5, 7)]
cases = []
# levels from far below the default gate to far above it, range_tv_in and blend alternating; range_tv_out moves on its own
for k, level in enumerate([10, 40, 52, 60, 66, 75, 90, 100, 108, 116, 130, 160, 190, 205, 214, 222, 240]):
    for tv in (bool(k % 2), not bool(k % 2)):
        cases.append(dict(level=level, shape=SHAPES[len(cases) % len(SHAPES)], range_tv_in=tv, range_tv_out=bool(len(cases) % 3), blend=len(cases) % 4 != 3,
                          luma_dark=0.20, luma_bright=0.80, sigmas=[25, 80, 250]))
# the bounds: below, at and above a frame's own f_luma, as luma_dark and as luma_bright; other sigmas go through untouched
for k, (level, tv) in enumerate([(70, True), (70, False), (150, True), (150, False)]):
    for side, delta in (("dark", -1e-6), ("dark", 0.0), ("dark", 1e-6), ("bright", -1e-6), ("bright", 0.0), ("bright", 1e-6)):
        cases.append(dict(level=level, shape=SHAPES[(k + len(cases)) % len(SHAPES)], range_tv_in=tv, range_tv_out=not tv, blend=True, bound=(side, delta),
                          luma_dark=0.20, luma_bright=0.80, sigmas=[15.5, 300] if side == "dark" else [2, 4, 8, 16, 32, 64, 128, 256]))
# the min_w floor (0.90 * (f / 0.40) ** 3 < 0.25 below f = 0.261) with a gate that lets such frames in, and a weight above the floor
for level, tv in [(20, False), (45, False), (60, True), (80, True), (85, False), (98, False)]:
    cases.append(dict(level=level, shape=SHAPES[len(cases) % len(SHAPES)], range_tv_in=tv, range_tv_out=True, blend=True, luma_dark=0.02, luma_bright=0.95,
                      sigmas=[25, 80, 250]))

fx = {"provenance": np.array("generated by tools/gen_golden_retinex.py executing the reference: vsdeoldify/__init__.py HAVC_retinex, vsslib/vsretinex.py "
                             "vs_retinex / vs_retinex_fast (selector body filter_retinex included), havc_utils.py convert_format_RGB24 / restore_format, "
                             "vsslib/imfilters.py get_image_luma / image_luma_blend with real Pillow; the plugin's frames are prescribed inputs")}
stats = dict(gated=0, blended=0, floor=0, taken=0)
for i, c in enumerate(cases):
    img = frame_at(c["level"], tuple(c["shape"]))
    rtx = prescribe(img)
    fl = luma_of(img, c["range_tv_in"])
    if "bound" in c:
        side, delta = c["bound"]
        c["luma_" + side] = fl + delta
    del PLUGIN_CALLS[:], PRESCRIBED[:], LOOKS[:], WEIGHTS[:]
    PRESCRIBED.append(rtx)
    out = HAVC_retinex(Clip([Frame(img)]), c["luma_dark"], c["luma_bright"], c["sigmas"], c["range_tv_in"], c["range_tv_out"], c["blend"])
    out = out.frames[0].rgb()
    assert len(PLUGIN_CALLS) == 1 and len(LOOKS) in (1, 2) and len(WEIGHTS) <= 1
    gate, weight = len(LOOKS) == 2, WEIGHTS[0] if WEIGHTS else -1.0
    y = sys.modules["cv2"].cvtColor(img, sys.modules["cv2"].COLOR_RGB2YUV)[:, :, 0]
    rec = dict(luma_dark=c["luma_dark"], luma_bright=c["luma_bright"], sigmas=c["sigmas"], range_tv_in=c["range_tv_in"], range_tv_out=c["range_tv_out"],
               blend=c["blend"], f_luma=float(fl), gate=gate, weight=weight, sum_y=int(y.astype(np.int64).sum()), n_pixels=int(y.size),
               plugin={k: (list(v) if isinstance(v, (list, tuple)) else v) for k, v in PLUGIN_CALLS[0].items()})
    fx[f"case_{i}_params"] = np.array(json.dumps(rec))
    fx[f"case_{i}_in"], fx[f"case_{i}_rtx"], fx[f"case_{i}_out"] = img, rtx, out
    stats["gated"] += not gate
    stats["blended"] += weight >= 0
    stats["floor"] += weight == 0.25
    stats["taken"] += gate and weight < 0
fx["n_cases"] = np.array(len(cases))
path = os.path.join(ROOT, "tests", "golden", "retinex.npz")
np.savez_compressed(path, **fx)
print("wrote retinex.npz", os.path.getsize(path), "bytes;", len(cases), "cases;", stats)
