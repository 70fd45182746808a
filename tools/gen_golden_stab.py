#!/usr/bin/env python3
"""Golden vectors for HAVC_stabilizer(stab=True) by EXECUTING the reference (build container only).  Writes tests/golden/chroma_stab.npz (data only).

What runs: the reference's own vs_chroma_stabilizer_ex, vs_clip_color_stabilizer, _build_avg_arithmetic, _build_avg_weighted, _average_clips_ex,
vs_get_clip_frame, vs_recover_clip_color, vs_sc_recover_clip_color (with its frame function color_frame), vs_adjust_clip_hue and vs_sc_adjust_clip_hue
(vsslib/vsfilters.py:38-157, 216-356, 435-459; taken out of that file's syntax tree at run time: the module imports half the package), with
DEF_STANDARD_DARK / DEF_STANDARD_BRIGHT of vsslib/constants.py imported as they are.

The stand-in (tools/refshim.py plus the classes below) is a RECORDING vapoursynth: a clip knows its format and nothing else; every native filter appends
[name, arguments] to a trace and hands a clip on.  Recorded: resize.Bicubic, std.AverageFrames (the number of clips, the weights, scale, scenechange, planes),
std.ModifyFrame (the selector's name and the arguments bound to it).  color_frame is then CALLED on synthetic frames whose luma is PRESCRIBED (get_image_luma
is a stand-in that returns it; restore_color is a stand-in that records the weight it gets): that pins the `n < 15` rule and the luma-band override.

What this pins, for nframes 2..16 and both modes (and the mode aliases, and the refusal of an unknown one): N, both weight lists (the asymmetric weighted one
as written), the resize and AverageFrames arguments in call order for tht == 0 and tht > 0, vs_get_clip_frame's one-hot weight lists, the arguments
color_frame is bound to, hue_adjust 'none' adding no call, and color_frame's decisions.
"""
import ast
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
vs.RGB24, vs.YUV420P8 = "RGB24", "YUV420P8"
vs.YUV, vs.RGB = 3, 2000
vs.Error = type("Error", (Exception,), {})
vs.core.log_message = lambda *a: None

TRACE, SELECTORS, RESTORE_CALLS = [], [], []


def record(name, args):
    TRACE.append([name, args])


class Clip:
    def __init__(self, fmt):
        self.format = types.SimpleNamespace(id=fmt, color_family=vs.RGB if fmt == "RGB24" else vs.YUV)
        self.num_frames, self.width, self.height = 100, 64, 48
        self.resize = types.SimpleNamespace(Bicubic=self._bicubic)
        self.std = types.SimpleNamespace(ModifyFrame=self._modify_frame)

    def _bicubic(self, **kw):
        record("resize.Bicubic", dict(kw))
        return Clip(kw.get("format", self.format.id))

    def _modify_frame(self, clips, selector):
        record("std.ModifyFrame", dict(selector=selector.func.__name__, **selector.keywords))
        SELECTORS.append(selector)
        return Clip(self.format.id)


def average_frames(clips, weights, scale=None, scenechange=None, planes=None):
    many = isinstance(clips, (list, tuple))
    record("std.AverageFrames", dict(clips=len(clips) if many else 1, weights=list(weights), scale=scale, scenechange=scenechange, planes=planes))
    return Clip((clips[len(clips) // 2] if many else clips).format.id)


vs.VideoNode = Clip
vs.core.std = types.SimpleNamespace(AverageFrames=average_frames)
constants = importlib.import_module("vsdeoldify.vsslib.constants")


class Frame:
    """a frame with a prescribed luma"""

    def __init__(self, luma, tag):
        self.luma, self.tag, self.props = luma, tag, {}

    def copy(self):
        return Frame(self.luma, self.tag)


def restore_color(img_color, img_gray, sat, tht, weight, tht_scen, hue_adjust, return_mask):
    RESTORE_CALLS.append(dict(color=img_color.tag, gray=img_gray.tag, sat=sat, tht=tht, weight=weight, tht_scen=tht_scen, hue_adjust=hue_adjust,
                              return_mask=return_mask))
    return Frame(None, "restored")


def take(path, names, ns):
    """compile the named functions of a reference file in the namespace ns"""
    tree = ast.parse(open(path).read(), path)
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert sorted(f.name for f in fns) == sorted(names), (path, names)
    future = ast.ImportFrom(module="__future__", names=[ast.alias(name="annotations")], level=0)
    exec(compile(ast.fix_missing_locations(ast.Module(body=[future] + fns, type_ignores=[])), path, "exec"), ns)
    return ns


NAMES = ["vs_chroma_stabilizer_ex", "vs_clip_color_stabilizer", "_build_avg_arithmetic", "_build_avg_weighted", "_average_clips_ex", "vs_get_clip_frame",
         "vs_recover_clip_color", "vs_sc_recover_clip_color", "vs_adjust_clip_hue", "vs_sc_adjust_clip_hue"]
flt = take(os.path.join(refshim.REF_ROOT, "vsdeoldify", "vsslib", "vsfilters.py"), NAMES,
           dict(vs=vs, math=math, partial=partial, frame_to_image=lambda f: f, image_to_frame=lambda img, f_out: img,
                get_image_luma=lambda img, maxrange: img.luma, restore_color=restore_color, DEF_STANDARD_DARK=constants.DEF_STANDARD_DARK,
                DEF_STANDARD_BRIGHT=constants.DEF_STANDARD_BRIGHT))


def run(**kw):
    del TRACE[:], SELECTORS[:]
    try:
        flt["vs_chroma_stabilizer_ex"](Clip("RGB24"), **kw)
    except vs.Error as e:
        return dict(args=kw, calls=list(TRACE), error=str(e))
    return dict(args=kw, calls=list(TRACE))


plans = []
for nframes in range(2, 17):
    for mode in ("A", "W"):
        n = max(3, min(nframes + (nframes % 2 == 0), 15))
        weights = flt["_build_avg_arithmetic" if mode == "A" else "_build_avg_weighted"](n)
        for tht in (0, 15):
            plans.append(dict(run(nframes=nframes, mode=mode, sat=0.9, tht=tht, weight=0.2, tht_scen=0.8, hue_adjust="none", algo=0), N=n, weights=weights))
for mode in ("arithmetic", "center", "weighted", "left", "right", "X", "a"):
    for tht in (0, 15):
        plans.append(run(nframes=5, mode=mode, tht=tht))

# color_frame on synthetic frames: the selector _average_clips_ex bound last
run(nframes=3, mode="A", sat=0.7, tht=15, weight=0.2, tht_scen=0.8)
selector = SELECTORS[-1]
probes = []
for n in (0, 1, 14, 15, 16, 1000):
    for luma in (0.0, 0.1, 0.219999, 0.22, 0.5, 0.78, 0.780001, 0.9, 1.0):
        for weight in (0.2, 0.0, -0.5, -0.8, -0.9):
            del RESTORE_CALLS[:]
            gray, color = Frame(luma, "gray"), Frame(0.5, "color")
            out = partial(selector.func, **dict(selector.keywords, weight=weight))(n, [gray, color])
            assert len(RESTORE_CALLS) <= 1 and (out.tag == "restored") == bool(RESTORE_CALLS)
            probes.append(dict(n=n, luma=luma, weight=weight, result=RESTORE_CALLS[0] if RESTORE_CALLS else None))

fx = {"provenance": np.array("generated by tools/gen_golden_stab.py executing the reference against a recording vapoursynth stand-in: vsslib/vsfilters.py "
                             "vs_chroma_stabilizer_ex / vs_clip_color_stabilizer / _build_avg_arithmetic / _build_avg_weighted / _average_clips_ex / "
                             "vs_get_clip_frame / vs_recover_clip_color / vs_sc_recover_clip_color (color_frame called on frames with a prescribed luma) / "
                             "vs_adjust_clip_hue; vsslib/constants.py DEF_STANDARD_DARK / DEF_STANDARD_BRIGHT"),
      "plans": np.array(json.dumps(plans)), "probes": np.array(json.dumps(probes))}
path = os.path.join(ROOT, "tests", "golden", "chroma_stab.npz")
np.savez_compressed(path, **fx)
print("wrote chroma_stab.npz", os.path.getsize(path), "bytes;", len(plans), "plans,", sum("error" in p for p in plans), "refusals,", len(probes), "probes")
