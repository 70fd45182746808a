"""HAVC_TimeCube without VapourSynth (vsdeoldify/__init__.py:2995-3026 -> vs_timecube / vs_timecube_load, vsslib/vsplugins.py:283-378): a 3D LUT from a
.cube file, vs_tweak with the effect's factors, and a merge with the input by strength.

PINNED -- the reference's Python, restated here as a PLAN: `timecube_plan` derives the file the reference asks for, the arguments vs_tweak gets and which merge
runs with which arguments.  tests/golden/timecube.npz records the same by EXECUTING the reference against a recording vapoursynth stand-in
(tools/gen_golden_timecube.py); tests/test_timecube_host.py compares them record by record.

UNPINNED -- the timecube.Cube plugin is not in the reference tree and cannot be executed where the fixtures are made.  tests/timecube_util.py restates it in
numpy (trilinear interpolation, float32, red then green then blue) and is THE DEFINITION for this project; csrc/lut3d.hip equals it byte for byte.  `parse_cube`
reads the Adobe / Resolve text format; `axis_tables` turns the file's domain into the cell and fraction of each of the 256 sample values, in float32 on the host,
so the kernel only reads them.

DEVIATION -- a LUT file that is not there raises HAVCError naming the path.  The reference logs "not found" and goes on to tweak and merge the un-graded clip;
no .cube file ships with either tree, so a missing file is the normal state here, and a silently wrong picture is worse than an error.  For the same reason a
lut_effect outside 0..11 without `cube=` is refused (the reference falls through with an empty file name), and a strength outside [0, 1] (std.Merge refuses it).
"""
import collections
import ctypes as C
import math
import os

import numpy as np

MIN_SIZE, MAX_SIZE = 2, 256                                    # csrc/lut3d_ops.h LUT3D_MIN_SIZE / LUT3D_MAX_SIZE

# vs_timecube_load, vsplugins.py:288-312: the file under <lut_dir>/color/ per lut_effect
LUT_FILES = ["Stockpresets - Forest Film.cube", "Presetpro - City Skyline.cube", "Presetpro - Exploration.cube", "Presetpro - FUJ Film.cube",
             "Presetpro - Hollywood.cube", "Presetpro - Classic Film.cube", "Presetpro - Warm Haze.cube", "Presetpro - HDR Color.cube",
             "Presetpro - Amber Light.cube", "Presetpro - Blue Mist.cube", "Presetpro - Vintage Fox.cube", "Presetpro - Flat Pop.cube"]
# vs_timecube, vsplugins.py:335-359: what differs from hue 0, sat 1, bright 0, cont 1, gamma 1 per lut_effect
LUT_FACTORS = [dict(sat=0.70, hue=10), dict(cont=0.90, sat=0.65, hue=-3, bright=1, gamma=1.05), dict(sat=1.05, cont=1.05, gamma=0.95, hue=10, bright=-1),
               dict(sat=0.80, hue=10), dict(sat=0.75, hue=10), dict(sat=0.80), dict(sat=0.75), dict(sat=0.95), dict(sat=0.40, hue=10, bright=5),
               dict(sat=0.80, hue=3, bright=-1), dict(sat=0.80, hue=3, bright=1), dict(sat=0.80, hue=-2, bright=0)]
AMBER_LIGHT = 8                                                # the effect that merges through ChromaBoundAdaptiveMerge
AMBER_CMC_P = [0.15, True, 25, 25]                             # vsplugins.py:374

Cube = collections.namedtuple("Cube", "size domain_min domain_max table title")


def _err(msg):
    from .havc import HAVCError
    return HAVCError(msg)


# ---- the .cube reader ------------------------------------------------------------------------------------------------------------------------------------------
def parse_cube(path_or_text):
    """A .cube file (a path) or its text (anything with a line break in it) -> Cube(size, domain_min[3], domain_max[3], table float32 [N][N][N][3] indexed
    [blue][green][red][channel], title).  Adobe / Resolve: `#` comments, blank lines, TITLE "..", LUT_3D_SIZE N (2..256), DOMAIN_MIN / DOMAIN_MAX a b c,
    LUT_3D_INPUT_RANGE a b (the domain of all three channels), then N^3 rows of three floats, red fastest.  Everything else is refused, with file and line."""
    if isinstance(path_or_text, (bytes, os.PathLike)) or "\n" not in str(path_or_text):
        name = os.fspath(path_or_text)
        if not os.path.isfile(name):
            raise _err(f"HAVC_TimeCube: LUT cube file: {name} not found!")
        with open(name, "r", encoding="utf-8", errors="replace", newline=None) as f:
            text = f.read()
    else:
        name, text = "<text>", str(path_or_text)

    def bad(no, why):
        return _err(f"HAVC_TimeCube: {name}, line {no}: {why}")

    def floats(no, words, n, what):
        try:
            v = [float(w) for w in words]
        except ValueError:
            raise bad(no, f"{what} needs {n} numbers") from None
        if len(v) != n:
            raise bad(no, f"{what} needs {n} numbers")
        if not all(math.isfinite(x) for x in v):
            raise bad(no, "a value is not finite")
        return v

    size, title, dmin, dmax, rows, last = None, "", [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [], 0
    for no, line in enumerate(text.splitlines(), 1):
        line = line.strip()
        if not line or line.startswith("#"):
            continue
        last = no
        words = line.split()
        key = words[0]
        if key[0].isalpha() or key[0] == "_":
            if key == "TITLE":
                title = line[len(key):].strip().strip('"')
            elif key == "LUT_1D_SIZE":
                raise bad(no, "LUT_1D_SIZE: 1D and shaper LUTs are not built")
            elif key == "LUT_3D_SIZE":
                if size is not None:
                    raise bad(no, "a second LUT_3D_SIZE")
                if len(words) != 2 or not words[1].isdigit() or not MIN_SIZE <= int(words[1]) <= MAX_SIZE:
                    raise bad(no, f"LUT_3D_SIZE must be one integer in {MIN_SIZE}..{MAX_SIZE}")
                size = int(words[1])
            elif key == "DOMAIN_MIN":
                dmin = floats(no, words[1:], 3, key)
            elif key == "DOMAIN_MAX":
                dmax = floats(no, words[1:], 3, key)
            elif key == "LUT_3D_INPUT_RANGE":
                lo, hi = floats(no, words[1:], 2, key)
                dmin, dmax = [lo] * 3, [hi] * 3
            elif key.lower() in ("nan", "inf", "infinity"):
                raise bad(no, "a value is not finite")
            else:
                raise bad(no, f"unknown keyword {key}")
            continue
        if size is None:
            raise bad(no, "a table row in front of LUT_3D_SIZE")
        if len(rows) == size ** 3:
            raise bad(no, f"more than {size ** 3} rows for LUT_3D_SIZE {size}")
        rows.append(floats(no, words, 3, "a table row"))
    if size is None:
        raise bad(last, "no LUT_3D_SIZE")
    if len(rows) != size ** 3:
        raise bad(last, f"{len(rows)} rows, LUT_3D_SIZE {size} needs {size ** 3}")
    if any(not np.float32(hi) > np.float32(lo) for lo, hi in zip(dmin, dmax)):
        raise bad(last, "DOMAIN_MAX must be larger than DOMAIN_MIN on every channel (as float32)")
    with np.errstate(over="ignore"):
        table = np.asarray(rows, np.float64).astype(np.float32)
    if not np.isfinite(table).all():
        raise bad(last, "a value is not finite in float32")
    return Cube(size, tuple(dmin), tuple(dmax), np.ascontiguousarray(table.reshape(size, size, size, 3)), title)


def axis_tables(cube):
    """-> (idx int32 [3][256], frac float32 [3][256]): for sample s of channel c, in float32 with one operation per step, x = s / 255,
    t = (x - dmin_c) / (dmax_c - dmin_c) * (N - 1) clamped to [0, N - 1], idx = min(floor(t), N - 2), frac = t - idx"""
    f32 = np.float32
    n1 = f32(cube.size - 1)
    idx, frac = np.empty((3, 256), np.int32), np.empty((3, 256), np.float32)
    x = np.arange(256, dtype=np.float32) / f32(255)
    for c in range(3):
        lo, hi = f32(cube.domain_min[c]), f32(cube.domain_max[c])
        t = (x - lo) / (hi - lo)
        t = np.minimum(np.maximum(t * n1, f32(0)), n1)
        i = np.minimum(np.floor(t), f32(cube.size - 2))
        idx[c], frac[c] = i.astype(np.int32), t - i
    return idx, frac


# ---- vs_timecube's Python --------------------------------------------------------------------------------------------------------------------------------------
def timecube_plan(strength=1.0, lut_effect=0, factors=None, lut_dir=None, cube=None):
    """vs_timecube / vs_timecube_load (vsplugins.py:283-378) -> dict(identity, file, tweak, merge):
      identity  strength == 0: the clip itself comes back, nothing else is looked at (:327-328)
      file      the path the reference hands to timecube.Cube, <lut_dir>/color/<name> normalised; None with cube=
      tweak     the five keyword arguments of vs_tweak: the effect's defaults, or `factors` = [hue, sat, bright, cont, gamma]
      merge     None (strength == 1), ["combine_models", dict(method=7, w=strength, cmc_p=[0.15, True, 25, 25])] for effect 8, else ["simple_merge", strength]"""
    if strength == 0:
        return dict(identity=True, file=None, tweak=None, merge=None)
    if not 0 <= strength <= 1:
        raise _err(f"HAVC_TimeCube: strength = {strength}: std.Merge needs a weight in [0, 1]")
    path = None
    if cube is None:
        if isinstance(lut_effect, bool) or not isinstance(lut_effect, (int, np.integer)) or not 0 <= lut_effect < len(LUT_FILES):
            raise _err(f"HAVC_TimeCube: lut_effect = {lut_effect!r}: 0..{len(LUT_FILES) - 1} name a LUT file")
        if lut_dir is None:
            raise _err("HAVC_TimeCube: no LUT directory: pass lut_dir=, set the environment variable HAVC_LUT_DIR, or pass cube=")
        path = os.path.normpath(os.path.join(lut_dir, "color", LUT_FILES[lut_effect]))
    tweak = dict(hue=0, sat=1, bright=0, cont=1, gamma=1)
    if factors is None:
        if isinstance(lut_effect, (int, np.integer)) and 0 <= lut_effect < len(LUT_FACTORS):
            tweak.update(LUT_FACTORS[lut_effect])
    else:
        tweak = dict(hue=factors[0], sat=factors[1], bright=factors[2], cont=factors[3], gamma=factors[4])
    if strength == 1:
        merge = None
    elif lut_effect == AMBER_LIGHT:
        merge = ["combine_models", dict(method=7, w=strength, cmc_p=list(AMBER_CMC_P))]
    else:
        merge = ["simple_merge", strength]
    return dict(identity=False, file=path, tweak=tweak, merge=merge)


def load_cube(plan, cube=None):
    """the Cube of a plan: cube= (a Cube, or a path / text for parse_cube), else the plan's file, which must be there (module docstring: DEVIATION)"""
    if isinstance(cube, Cube):
        return cube
    return parse_cube(plan["file"] if cube is None else cube)


# ---- the GPU path ----------------------------------------------------------------------------------------------------------------------------------------------
def lut3d_np(ctx, clip, cube, table_ptr=None):
    """the LUT alone through havc_lut3d_clip (two launches): a frame [h, w, 3] or a clip [n, h, w, 3] of any width and height, ndarray or DeviceImage; a
    DeviceImage in gives a DeviceImage out and the call only enqueues.  table_ptr: the cube's table already in device memory (a ctypes pointer; tests and
    callers that apply one cube many times)"""
    from . import _native as nat
    from .device import DeviceImage, is_device, operand_ptr
    from .tweak import _prepare
    clip, shape, n = _prepare(clip, "HAVC_TimeCube", False)
    if not MIN_SIZE <= cube.size <= MAX_SIZE:
        raise _err(f"HAVC_TimeCube: a cube of {cube.size} points per axis: {MIN_SIZE}..{MAX_SIZE} are supported")
    table = np.ascontiguousarray(cube.table, dtype=np.float32)
    if table.shape != (cube.size,) * 3 + (3,):
        raise _err("HAVC_TimeCube: the cube's table must be [size][size][size][3]")
    idx, frac = axis_tables(cube)
    p = nat.Lut3dParams(width=shape[-2], height=shape[-3], n_frames=n, size=cube.size)
    out = DeviceImage(ctx, shape) if is_device(clip) else np.empty(shape, np.uint8)
    nat.check(ctx.lib.havc_lut3d_clip(ctx.h, operand_ptr(clip), operand_ptr(out), nat.as_ptr(table) if table_ptr is None else table_ptr, nat.as_ptr(idx),
                                      nat.as_ptr(frac), C.byref(p)), ctx.h)
    return out
