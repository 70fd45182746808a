#!/usr/bin/env python3
"""Golden vectors for HAVC_TimeCube by EXECUTING the reference (build container only).  Writes tests/golden/timecube.npz (data only).

What runs: the reference's own HAVC_TimeCube (vsdeoldify/__init__.py:2995-3026; the package's __init__ needs VapourSynth and every model, so the function is
taken out of that file's syntax tree at run time), vs_timecube and vs_timecube_load (vsslib/vsplugins.py:283-378; taken out of the syntax tree as well: the
module imports half the package), and convert_format_RGB24 / restore_format of vsdeoldify/havc_utils.py and the constants of vsslib/constants.py, imported
as they are.

The stand-in (tools/refshim.py plus the classes below) is a RECORDING vapoursynth: a clip knows its format and frame props and nothing else.  Recorded, in
call order: timecube.Cube (the directory under TimeCube_dir and the file name it is handed), vs_tweak (its keyword arguments), vs_combine_models (method,
clipb_weight, CMC_p) and std.Merge (weight).  pathlib.Path.is_file answers True inside vs_timecube_load: no .cube file ships with the reference.
TimeCube_dir is the literal "LUTDIR"; load_TimeCube_plugin does nothing.

What this pins: per lut_effect 0..11 the file requested, the factors vs_tweak gets with factors=None and with a list, which merge runs with which
arguments at strength 0.5 (effect 8: method 7 with CMC_p), and the early returns at strength 0 (no call at all) and strength 1 (no merge).
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

TRACE = []
LUTDIR = "LUTDIR"


class Clip:
    """a format, frame props and a tag that says which call made it"""

    def __init__(self, props, tag="source"):
        self.format = types.SimpleNamespace(id="RGB24", color_family=vs.RGB, bits_per_sample=8, sample_type=vs.INTEGER)
        self.props, self.tag = dict(props), tag
        self.num_frames, self.width, self.height = 1, 64, 48
        self.std = types.SimpleNamespace(SetFrameProps=lambda **kw: Clip({**self.props, **{k: int(v) for k, v in kw.items()}}, self.tag))

    def get_frame(self, n):
        return types.SimpleNamespace(props=self.props)


def cube(clip, cube):
    rel = os.path.relpath(cube, LUTDIR).replace(os.sep, "/")
    TRACE.append(["timecube.Cube", dict(clip=clip.tag, dir=os.path.dirname(rel), file=os.path.basename(rel))])
    return Clip(clip.props, "lut")


def tweak(clip, **kw):
    TRACE.append(["vs_tweak", dict(clip=clip.tag, **kw)])
    return Clip(clip.props, "tweaked")


def combine(clip_a, clip_b, method, clipb_weight, CMC_p):
    TRACE.append(["vs_combine_models", dict(clip_a=clip_a.tag, clip_b=clip_b.tag, method=method, clipb_weight=clipb_weight, CMC_p=list(CMC_p))])
    return Clip(clip_a.props, "merged")


def merge(clipa, clipb, weight):
    TRACE.append(["std.Merge", dict(clipa=clipa.tag, clipb=clipb.tag, weight=weight)])
    return Clip(clipa.props, "merged")


class AlwaysThere:
    """pathlib.Path for vs_timecube_load: every file is there"""

    def __init__(self, name):
        self.name = name

    def is_file(self):
        return True


vs.VideoNode = Clip
vs.core.timecube = types.SimpleNamespace(Cube=cube)
vs.core.std = types.SimpleNamespace(Merge=merge)

hu = importlib.import_module("vsdeoldify.havc_utils")
constants = importlib.import_module("vsdeoldify.vsslib.constants")


def take(path, names, ns):
    """compile the named functions of a reference file in the namespace ns"""
    tree = ast.parse(open(path).read(), path)
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert sorted(f.name for f in fns) == sorted(names), (path, names)
    future = ast.ImportFrom(module="__future__", names=[ast.alias(name="annotations")], level=0)
    exec(compile(ast.fix_missing_locations(ast.Module(body=[future] + fns, type_ignores=[])), path, "exec"), ns)
    return ns


ref = os.path.join(refshim.REF_ROOT, "vsdeoldify")
plg = take(os.path.join(ref, "vsslib", "vsplugins.py"), ["vs_timecube", "vs_timecube_load"],
           dict(vs=vs, os=os, Path=AlwaysThere, TimeCube_dir=LUTDIR, load_TimeCube_plugin=lambda: True, DEF_LUT_Exploration=constants.DEF_LUT_Exploration,
                vs_tweak=tweak, vs_combine_models=combine, HAVC_LogMessage=lambda *a: None, MessageType=types.SimpleNamespace(INFORMATION=1)))
api = take(os.path.join(ref, "__init__.py"), ["HAVC_TimeCube"],
           dict(vs=vs, convert_format_RGB24=hu.convert_format_RGB24, restore_format=hu.restore_format, vs_timecube=plg["vs_timecube"]))


def run(**kw):
    del TRACE[:]
    src = Clip({"_Matrix": int(vs.MATRIX_BT709)})
    out = api["HAVC_TimeCube"](src, **kw)
    return dict(args=kw, calls=json.loads(json.dumps(TRACE)), result=out.tag)


FACTORS = [12.0, 0.8, -12.0, 1.1, 1.2]                                   # hue, sat, bright, cont, gamma
records = []
for effect in range(12):
    records.append(run(strength=0.5, lut_effect=effect))
    records.append(run(strength=1.0, lut_effect=effect))
    records.append(run(strength=0.5, lut_effect=effect, factors=list(FACTORS)))
    records.append(run(strength=0, lut_effect=effect))
records.append(run())                                                    # the defaults: strength 1, effect 0
records.append(run(strength=1, lut_effect=8, factors=[0, 1, 0, 1, 1]))
records.append(run(strength=0.25, lut_effect=8, factors=[0, 1, 0, 1, 1]))
fx = {"provenance": np.array("generated by tools/gen_golden_timecube.py executing the reference against a recording vapoursynth stand-in: "
                             "vsdeoldify/__init__.py HAVC_TimeCube, vsslib/vsplugins.py vs_timecube / vs_timecube_load, havc_utils.py convert_format_RGB24 / "
                             "restore_format; Path.is_file answers True, TimeCube_dir is 'LUTDIR'"),
      "records": np.array(json.dumps(records))}
path = os.path.join(ROOT, "tests", "golden", "timecube.npz")
np.savez_compressed(path, **fx)
print("wrote timecube.npz", os.path.getsize(path), "bytes;", len(records), "records;", sum(not r["calls"] for r in records), "without a call")
