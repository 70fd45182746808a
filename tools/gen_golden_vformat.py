#!/usr/bin/env python3
"""Golden records for convert_format_RGB24 / restore_format on every supported clip format by EXECUTING the reference (build container only).  Writes
tests/golden/vformat.json (data only: the recorded calls).

What runs: convert_format_RGB24 and restore_format of vsdeoldify/havc_utils.py (:57-237), imported as they are, with _matrixIsInvalid / _rangeIsInvalid.

The stand-in (tools/refshim.py plus the classes below) is a RECORDING vapoursynth, as in tools/gen_golden_tweak.py: a clip knows its format and frame props
and nothing else.  resize.Bicubic appends [arguments, the frame props the call sees] to a trace -- the props, because a call that names no input range or
matrix takes them from there (the depth step of a > 8 bit clip) -- and hands on a clip of the new format.  std.SetFrameProps moves no sample and is not
recorded; what it sets shows in the props of the calls behind it.  Formats appear by VapourSynth's names, enums by their integer values.

What this pins, for every format x matrix prop x range prop (missing props included): the ordered resize.Bicubic calls of both functions with their
arguments, the ClipInfo fields, the pass-through of an RGB24 clip, and the refusal text of restore_format on a clip that is not RGB24.
"""
import enum
import importlib
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import refshim  # noqa: E402

refshim.install()
vs = sys.modules["vapoursynth"]
for i, n in enumerate(("DEBUG", "INFORMATION", "WARNING", "CRITICAL", "FATAL")):
    setattr(vs, "MESSAGE_TYPE_" + n, i)
vs.YUV, vs.GRAY, vs.RGB = "YUV", "GRAY", "RGB"
vs.INTEGER, vs.FLOAT = 0, 1


class MatrixCoefficients(enum.IntEnum):
    MATRIX_RGB, MATRIX_BT709, MATRIX_UNSPECIFIED, MATRIX_FCC, MATRIX_BT470_BG, MATRIX_ST170_M, MATRIX_ST240_M, MATRIX_YCGCO, MATRIX_BT2020_NCL = 0, 1, 2, 4, 5, 6, 7, 8, 9


class Range(enum.IntEnum):
    RANGE_FULL, RANGE_LIMITED = 0, 1


vs.MatrixCoefficients, vs.Range, vs.ColorRange = MatrixCoefficients, Range, Range
vs.MATRIX_BT709, vs.RANGE_FULL, vs.RANGE_LIMITED = MatrixCoefficients.MATRIX_BT709, Range.RANGE_FULL, Range.RANGE_LIMITED
vs.core.core_version = types.SimpleNamespace(release_major=74)
vs.core.log_message = lambda *a: None

SUBS = {"420": (1, 1), "422": (1, 0), "444": (0, 0)}
FORMATS = {"RGB24": ("RGB", 8)}
for sub in SUBS:
    for bits in (8, 10, 12, 16):
        FORMATS[f"YUV{sub}P{bits}"] = ("YUV", bits)
FORMATS.update(GRAY8=("GRAY", 8), GRAY16=("GRAY", 16))
vs.RGB24, vs.YUV420P8 = "RGB24", "YUV420P8"
TRACE = []


def _plain(v):
    if isinstance(v, Format):
        return v.id
    return int(v) if isinstance(v, enum.Enum) else v


class Format:
    def __init__(self, name):
        self.id, (self.color_family, self.bits_per_sample), self.sample_type = name, FORMATS[name], vs.INTEGER

    def replace(self, bits_per_sample):
        head = self.id[:-len(str(self.bits_per_sample))]
        return Format(head + str(bits_per_sample))


class Clip:
    def __init__(self, fmt, props):
        self.format = fmt if isinstance(fmt, Format) else Format(fmt)
        self.props = dict(props)
        self.std = types.SimpleNamespace(SetFrameProps=self._set_props)
        self.resize = types.SimpleNamespace(Bicubic=self._bicubic)

    def get_frame(self, n):
        return types.SimpleNamespace(props=dict(self.props))

    def _bicubic(self, **kw):
        TRACE.append([{k: _plain(v) for k, v in kw.items()}, dict(self.props)])
        return Clip(kw.get("format", self.format), self.props)

    def _set_props(self, **kw):
        return Clip(self.format, {**self.props, **{k: int(v) for k, v in kw.items()}})


vs.VideoNode = Clip
vs.core.resize = types.SimpleNamespace(Bicubic=lambda clip, **kw: clip.resize.Bicubic(**kw))
hu = importlib.import_module("vsdeoldify.havc_utils")

MATRIX_PROPS = {None: None, "709": 1, "470bg": 5, "170m": 6, "2020ncl": 9}
RANGE_PROPS = {None: None, "limited": 1, "full": 0}


def source(fmt, matrix, color_range):
    props = {}
    if MATRIX_PROPS[matrix] is not None:
        props["_Matrix"] = MATRIX_PROPS[matrix]
    if RANGE_PROPS[color_range] is not None:
        props["_Range"] = RANGE_PROPS[color_range]
    return Clip(fmt, props)


def run(fn, *args):
    del TRACE[:]
    try:
        out = fn(*args)
    except (ValueError, vs.Error) as e:
        return None, dict(calls=list(TRACE), error=str(e))
    return out, dict(calls=list(TRACE))


cases = []
for fmt in FORMATS:
    for matrix in MATRIX_PROPS:
        for color_range in RANGE_PROPS:
            src = source(fmt, matrix, color_range)
            out, conv = run(hu.convert_format_RGB24, src)
            rgb, info = out
            conv["passes"] = rgb is src
            conv["out_format"], conv["out_props"] = rgb.format.id, dict(rgb.props)
            conv["info"] = dict(clip_orig=info.clip_orig, format_id=info.format_id, color_family=info.color_family, bits_per_sample=info.bits_per_sample,
                                matrix=_plain(info.matrix), color_range=_plain(info.color_range), chroma_resize=info.chroma_resize)
            colored = Clip("RGB24", rgb.props)                             # what a colouring function hands back
            back, rest = run(hu.restore_format, colored, info)
            rest["passes"] = back is colored
            rest["out_format"] = back.format.id
            cases.append(dict(format=fmt, matrix=matrix, color_range=color_range, convert=conv, restore=rest))
_, info = hu.convert_format_RGB24(source("YUV420P8", "709", "limited"))
_, refusal = run(hu.restore_format, Clip("YUV420P8", {}), info)
fx = dict(provenance="generated by tools/gen_golden_vformat.py executing the reference's convert_format_RGB24 / restore_format (vsdeoldify/havc_utils.py) "
                     "against a recording vapoursynth stand-in; a call is [arguments, frame props it sees]",
          cases=cases, restore_not_rgb24=refusal)
path = os.path.join(ROOT, "tests", "golden", "vformat.json")
with open(path, "w") as f:
    json.dump(fx, f, indent=0, sort_keys=True)
    f.write("\n")
print("wrote vformat.json", os.path.getsize(path), "bytes;", len(cases), "cases; refusal:", refusal.get("error"))
