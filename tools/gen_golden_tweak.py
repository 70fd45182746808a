#!/usr/bin/env python3
"""Golden vectors for HAVC_tweak / HAVC_adjust_rgb / HAVC_rgb_denoise by EXECUTING the reference (build container only).  Writes tests/golden/tweak.npz
(data only).

What runs: the reference's own HAVC_tweak, HAVC_adjust_rgb and HAVC_rgb_denoise (vsdeoldify/__init__.py:1377-1408, 1342-1374, 924-944; the package's __init__
needs VapourSynth and every model, so the three functions are taken out of that file's syntax tree at run time), vs_tweak, vs_rgb_normalize with its frame
function auto_white_adjust and vs_simple_merge (vsslib/vsfilters.py:753-850, 1013-1038, 730-739; taken out of the syntax tree as well: the module imports
half the package), and convert_format_RGB24, restore_format, is_limited_range, adjust_rgb and rgb_denoise of vsdeoldify/havc_utils.py, imported as they are.

The stand-in (tools/refshim.py plus the classes below) is a RECORDING vapoursynth: a clip knows its format and frame props and nothing else; every native
filter that changes samples appends [name, arguments] to a trace and hands a clip on.  Recorded: std.Levels, resize.Bicubic (format as its name), std.Expr,
std.Lut, std.Merge; in rgb_denoise also rgb_balance / rgb_equalizer (havc_utils functions that tests/golden/equalize.npz pins on their own).  Not recorded,
because they move no sample: std.ShufflePlanes, std.PlaneStats, std.FrameEval, std.SetFrameProps.  std.FrameEval calls the frame function once, with
frames whose PlaneStatsAverage props are PRESCRIBED by the case.

What this pins: the neutral call (no native call at all), the gamma handed to std.Levels, the arguments of both resize.Bicubic, both expression strings, the
256-entry luma list with the -1 < bright < 1 scaling and the truncating int() on negative values, hue = +-180 and sat = 0; adjust_rgb's three affine
strings with the bias scaled by 256 / 235 (no range prop, or limited) and 256 / 255 (full), the per-plane gammas, every refusal text, the un-rounded gains
of vs_rgb_normalize for prescribed averages (a zero blue mean included), the std.Merge weight, and rgb_denoise's calls.
"""
import ast
import enum
import importlib
import json
import math
import os
import sys
import types
from functools import partial

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import refshim  # noqa: E402

refshim.install()
vs = sys.modules["vapoursynth"]
for i, n in enumerate(("DEBUG", "INFORMATION", "WARNING", "CRITICAL", "FATAL")):
    setattr(vs, "MESSAGE_TYPE_" + n, i)
vs.RGB24, vs.YUV420P8, vs.GRAY8 = "RGB24", "YUV420P8", "GRAY8"
vs.YUV, vs.GRAY, vs.RGB = 3, 1000, 2000
vs.INTEGER, vs.FLOAT = 0, 1


class MatrixCoefficients(enum.IntEnum):
    MATRIX_RGB, MATRIX_BT709, MATRIX_UNSPECIFIED, MATRIX_BT470_BG = 0, 1, 2, 5


class Range(enum.IntEnum):
    RANGE_FULL, RANGE_LIMITED = 0, 1


vs.MatrixCoefficients, vs.Range, vs.ColorRange = MatrixCoefficients, Range, Range
vs.MATRIX_BT709, vs.RANGE_FULL, vs.RANGE_LIMITED = MatrixCoefficients.MATRIX_BT709, Range.RANGE_FULL, Range.RANGE_LIMITED
vs.core.core_version = types.SimpleNamespace(release_major=74)
vs.core.log_message = lambda *a: None

TRACE, AVERAGES = [], []
FAMILY = {"RGB24": vs.RGB, "YUV420P8": vs.YUV, "GRAY8": vs.GRAY}


def _plain(v):
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    return v.name if isinstance(v, enum.Enum) else v


def record(name, args):
    TRACE.append([name, _plain(args) if not isinstance(args, dict) else {k: _plain(v) for k, v in args.items()}])


class Clip:
    """a format, frame props, and (for a plane taken out by ShufflePlanes) the plane's number"""

    def __init__(self, fmt, props, plane=None, stats=None):
        self.format = types.SimpleNamespace(id=fmt, color_family=FAMILY[fmt], bits_per_sample=8, sample_type=vs.INTEGER)
        self.props, self.plane, self.stats = dict(props), plane, stats
        self.num_frames, self.width, self.height = 1, 64, 48
        self.std = types.SimpleNamespace(Levels=self._levels, Lut=self._lut, ShufflePlanes=self._shuffle, SetFrameProps=self._set_props,
                                         Expr=lambda expr: core_expr(self, expr))
        self.resize = types.SimpleNamespace(Bicubic=self._bicubic)

    def get_frame(self, n):
        return types.SimpleNamespace(props=self.props)

    def _same(self):
        return Clip(self.format.id, self.props)

    def _levels(self, **kw):
        if self.plane is not None:
            kw = dict(plane=self.plane, **kw)
        record("std.Levels", kw)
        return Clip(self.format.id, self.props, self.plane)

    def _lut(self, **kw):
        record("std.Lut", kw)
        return self._same()

    def _bicubic(self, **kw):
        record("resize.Bicubic", kw)
        return Clip(kw.get("format", self.format.id), self.props)

    def _shuffle(self, planes, colorfamily):
        return Clip("GRAY8", self.props, plane=planes)

    def _set_props(self, **kw):
        return Clip(self.format.id, {**self.props, **{k: int(v) for k, v in kw.items()}})


def core_expr(clips=None, expr=None):
    record("std.Expr", expr)
    first = clips[0] if isinstance(clips, (list, tuple)) else clips
    return Clip(first.format.id, first.props, first.plane)


def core_shuffle(clips, planes, colorfamily):
    first = clips[0] if isinstance(clips, (list, tuple)) else clips
    if colorfamily == vs.GRAY:
        return Clip("GRAY8", first.props, plane=planes)
    return Clip("RGB24" if colorfamily == vs.RGB else "YUV420P8", first.props)


def core_merge(clipa, clipb, weight):
    record("std.Merge", dict(weight=weight))
    return clipa._same()


def core_frame_eval(clip, fn, prop_src):
    frames = [types.SimpleNamespace(props={"PlaneStatsAverage": AVERAGES[c.stats]}) for c in prop_src]
    return fn(0, frames)


vs.VideoNode = Clip
vs.core.std = types.SimpleNamespace(Expr=core_expr, ShufflePlanes=core_shuffle, Merge=core_merge, FrameEval=core_frame_eval,
                                    PlaneStats=lambda clip, plane: Clip(clip.format.id, clip.props, stats=plane),
                                    Levels=lambda clip, **kw: clip.std.Levels(**kw))
vs.core.resize = types.SimpleNamespace(Bicubic=lambda clip, **kw: clip.resize.Bicubic(**kw))

hu = importlib.import_module("vsdeoldify.havc_utils")
hu.rgb_balance = lambda clip, strength, rgb_factor: (record("rgb_balance", dict(strength=strength, rgb_factor=list(rgb_factor))), clip)[1]
hu.rgb_equalizer = lambda clip, **kw: (record("rgb_equalizer", kw), clip)[1]


def take(path, names, ns):
    """compile the named functions of a reference file in the namespace ns"""
    tree = ast.parse(open(path).read(), path)
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert sorted(f.name for f in fns) == sorted(names), (path, names)
    future = ast.ImportFrom(module="__future__", names=[ast.alias(name="annotations")], level=0)
    exec(compile(ast.fix_missing_locations(ast.Module(body=[future] + fns, type_ignores=[])), path, "exec"), ns)
    return ns


ref = os.path.join(refshim.REF_ROOT, "vsdeoldify")
flt = take(os.path.join(ref, "vsslib", "vsfilters.py"), ["vs_tweak", "vs_rgb_normalize", "vs_simple_merge"], dict(vs=vs, math=math, partial=partial))
api = take(os.path.join(ref, "__init__.py"), ["HAVC_tweak", "HAVC_adjust_rgb", "HAVC_rgb_denoise"],
           dict(vs=vs, havc_utils=hu, convert_format_RGB24=hu.convert_format_RGB24, restore_format=hu.restore_format, rgb_denoise=hu.rgb_denoise,
                vs_tweak=flt["vs_tweak"], vs_rgb_normalize=flt["vs_rgb_normalize"], vs_simple_merge=flt["vs_simple_merge"]))


def source(color_range):
    """an RGB24 clip as a script hands it over: BT.709, with the range prop or without it"""
    props = {"_Matrix": int(vs.MATRIX_BT709)}
    if color_range is not None:
        props["_Range"] = int(vs.RANGE_FULL if color_range == "full" else vs.RANGE_LIMITED)
    return Clip("RGB24", props)


def run(fn, *args, **kw):
    del TRACE[:]
    try:
        fn(*args, **kw)
    except ValueError as e:
        return dict(calls=list(TRACE), error=str(e))
    return dict(calls=list(TRACE))


tweak_cases = [dict(), dict(gamma=1.5), dict(gamma=0.7), dict(bright=0.5), dict(bright=-0.5), dict(bright=-40), dict(bright=40.0, cont=1.2), dict(cont=0.5),
               dict(cont=0.5, bright=-0.25), dict(cont=2.5), dict(hue=180), dict(hue=-180), dict(hue=30.0), dict(hue=-72.5, sat=1.4), dict(sat=0), dict(sat=10.0),
               dict(hue=12.0, sat=0.8, bright=-12.0, cont=1.1, gamma=1.2), dict(hue=0.0, sat=1.0, bright=0.0, cont=1.0, gamma=1.0), dict(bright=1.0),
               dict(bright=-1.0), dict(bright=0.999)]
adjust_cases = []
AVG = [(0.41, 0.37, 0.52), (0.2, 0.6, 0.1), (0.5, 0.25, 0.0), (0.0, 0.0, 0.0), (0.3333333333333333, 0.7071067811865476, 0.1234567891234567), (0.9, 0.9, 0.9)]
for k, avg in enumerate(AVG):
    for strength in (1, 0.5, 0.25):
        adjust_cases.append(dict(strength=strength, averages=list(avg), color_range=[None, "full", "limited"][k % 3]))
for cr in (None, "limited", "full"):
    adjust_cases += [dict(strength=0.0, color_range=cr), dict(strength=0.0, factor=[1.3, 0.8, 1.05], bias=[16, -32, 5.5], gamma=[1.2, 1.0, 0.8], color_range=cr),
                     dict(strength=0, factor=[2, 1, 0.5], bias=[235, -235, 0], gamma=[1, 2.2, 1.0], color_range=cr),
                     dict(strength=0.0, bias=[236, 0, 0], color_range=cr), dict(strength=0.0, bias=[0, -236, 0], color_range=cr),
                     dict(strength=0.0, bias=[0, 0, 255.5], color_range=cr), dict(strength=0.0, bias=[-256, 0, 0], color_range=cr),
                     dict(strength=0.0, bias=[0, 255, -255], color_range=cr),
                     dict(strength=0.0, gamma=[-0.1, 1, 1], color_range=cr), dict(strength=0.0, gamma=[1, -1, 1], color_range=cr),
                     dict(strength=0.0, gamma=[1, 1, -2.0], color_range=cr), dict(strength=0.0, gamma=[0, 1, 0.5], color_range=cr),
                     dict(strength=1.5, averages=[0.4, 0.4, 0.4], color_range=cr), dict(strength=-0.5, averages=[0.4, 0.4, 0.4], color_range=cr)]
denoise_cases = [dict(), dict(denoise_levels=[0.3, 0.2], rgb_factors=[0.98, 1.02, 1.0]), dict(denoise_levels=[1.0, 0.0], rgb_factors=[1.0, 1.0, 1.0])]

fx = {"provenance": np.array("generated by tools/gen_golden_tweak.py executing the reference against a recording vapoursynth stand-in: "
                             "vsdeoldify/__init__.py HAVC_tweak / HAVC_adjust_rgb / HAVC_rgb_denoise, vsslib/vsfilters.py vs_tweak / vs_rgb_normalize "
                             "(frame function auto_white_adjust included) / vs_simple_merge, havc_utils.py convert_format_RGB24 / restore_format / "
                             "is_limited_range / adjust_rgb / rgb_denoise; PlaneStatsAverage props are prescribed inputs")}
records = dict(tweak=[], adjust=[], denoise=[])
for c in tweak_cases:
    records["tweak"].append(dict(args=c, **run(api["HAVC_tweak"], source(None), **c)))
for c in adjust_cases:
    kw = {k: v for k, v in c.items() if k not in ("averages", "color_range")}
    AVERAGES[:] = c.get("averages", [])
    records["adjust"].append(dict(args=c, **run(api["HAVC_adjust_rgb"], source(c["color_range"]), **kw)))
for c in denoise_cases:
    records["denoise"].append(dict(args=c, **run(api["HAVC_rgb_denoise"], source(None), **c)))
for k, v in records.items():
    fx[k] = np.array(json.dumps(v))
path = os.path.join(ROOT, "tests", "golden", "tweak.npz")
np.savez_compressed(path, **fx)
print("wrote tweak.npz", os.path.getsize(path), "bytes;", {k: len(v) for k, v in records.items()}, "cases;",
      sum("error" in r for r in records["adjust"]), "refusals;", sum(not r["calls"] for r in records["tweak"]), "neutral")
