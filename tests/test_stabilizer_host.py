"""CPU (-m "not gpu"): HAVC_stabilizer (vsdeoldify/__init__.py:2748-2873) -- the expected values the GPU tests use are pinned to the executed reference
(tests/golden/stabilizer.npz), the argument rules run before any GPU context exists, and the C struct, its ctypes mirror and the signature agree."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import stabilizer_util as U
from tests.conftest import ROOT
from vsdeoldify_amd import _native as nat
from vsdeoldify_amd import havc
from vsdeoldify_amd.stabilizer import stabilize_np  # noqa: F401  (the entry point the GPU tests drive)

HEADER = os.path.join(ROOT, "include", "havc_mi355.h")


def test_oracle_chain_reproduces_the_executed_reference():
    """oracle.tweaks dark_tweak_frame -> chroma_bright_tweak_frame -> colormap_frame == vs_dark_tweak -> vs_chroma_bright_tweak -> vs_colormap of the
    reference on every chain case of the fixture, byte for byte"""
    g, cases, table = U.fixture()
    assert len(cases) >= 4 and g["img"].shape[0] <= 54 and g["img"].shape[1] <= 96
    changed = 0
    for i, c in enumerate(cases):
        got = U.oracle_chain(g["img"], *U.parsed(table, **c))
        assert np.array_equal(got, g[f"out_{i}"]), (i, c, int((got != g[f"out_{i}"]).sum()))
        changed += bool((g[f"out_{i}"] != g["img"]).any())
    assert changed >= len(cases) - 1                                            # (only the everything-off case hands the frame on)
    # the four configurations the fixture must hold
    assert any(c.get("dark") and c.get("smooth") and c.get("colormap", "none") != "none" for c in cases)
    assert any(c.get("dark") and len(c["dark_p"]) > 2 for c in cases)
    assert any(c.get("smooth") and c["smooth_p"][0] == c["smooth_p"][1] for c in cases)
    assert any(c.get("smooth") and c["smooth_p"][0] > c["smooth_p"][1] and c.get("colormap") == "blue->brown" for c in cases)


def test_colormap_translation_equals_the_reference_table():
    g, _, table = U.fixture()
    assert len(table) == 14
    for name, want in table.items():
        assert havc._get_colormap(name) == want, name
        assert havc._get_colormap(name.upper()) == want.lower(), name           # havc_utils.py:562: lower-cased first
    assert table["red->brown"] == "320:360|+50,0.90" and table["30:90|+300,0.5"] == "30:90|+300,0.5"
    for bad in ("red|a,b", "a|b|c", "red|0.5"):                                 # what restcolor._parse_hue_adjust rejects (havc_utils.py:573-575)
        with pytest.raises(havc.HAVCError, match="ColorMap choice is invalid"):
            havc._get_colormap(bad)
    assert havc._get_colormap("Purple->Green") == "purple->green"               # ... and what it lets through: refused by HAVC_stabilizer itself


def test_argument_rules_run_before_any_context():
    f = np.zeros((8, 8, 3), np.uint8)
    for rf in (15, 65, -1, 8):
        with pytest.raises(havc.HAVCError, match="HAVC_stabilizer: render_factor must be between: 16-64"):
            havc.HAVC_stabilizer(f, render_factor=rf)
    with pytest.raises(NotImplementedError, match="vs_chroma_stabilizer_ex"):
        havc.HAVC_stabilizer(f, stab=True)
    for bad in ("not a clip", None, [[1, 2, 3]]):
        with pytest.raises(havc.HAVCError, match="HAVC_stabilizer: this is not a clip"):
            havc.HAVC_stabilizer(bad)
    for bad in ("purple->green", "red|a,b", "Sepia"):                           # an unknown name: no colour map, no hue range
        with pytest.raises(havc.HAVCError, match="ColorMap choice is invalid"):
            havc.HAVC_stabilizer(f, colormap=bad)
    with pytest.raises(havc.HAVCError):
        havc.HAVC_stabilizer(np.zeros((8, 8), np.uint8))                        # not RGB24


def test_frame_size_rule():
    """__init__.py:2798-2803"""
    assert [havc._stabilizer_frame_size(0, w)[0] for w in (640, 768, 1920)] == [16, 19, 32]
    assert havc._stabilizer_frame_size(24, 1920) == (24, 384) and havc._stabilizer_frame_size(0, 1920) == (32, 512)
    assert havc._stabilizer_frame_size(24, 300) == (24, 300) and havc._stabilizer_frame_size(64, 1000) == (64, 1000)     # capped at the width
    assert havc._stabilizer_frame_size(16, 1920) == (16, 256) and havc._stabilizer_frame_size(64, 1920) == (64, 1024)


def test_public_function_is_exported_with_the_reference_argument_list():
    import inspect

    import vsdeoldify_amd
    assert vsdeoldify_amd.HAVC_stabilizer is havc.HAVC_stabilizer
    p = inspect.signature(havc.HAVC_stabilizer).parameters
    assert list(p) == ["clip", "dark", "dark_p", "smooth", "smooth_p", "stab", "stab_p", "colormap", "render_factor", "device_index"]
    assert (p["dark"].default, tuple(p["dark_p"].default), p["smooth"].default, tuple(p["smooth_p"].default), p["stab"].default,
            tuple(p["stab_p"].default), p["colormap"].default, p["render_factor"].default) == \
        (False, (0.2, 0.8), False, (0.3, 0.7, 0.9, 0.0, "none"), False, (5, 'A', 1, 15, 0.2, 0.8), "none", 24)


def test_stage_records_follow_the_frame_bodies():
    """the (mode, tresh, grad) the stage records carry are the ones stabilizer._luma_merge hands to havc_image_luma_merge, and the tweak arguments the ones
    imfilters.image_tweak_np / image_chroma_tweak_np hand to their entry points"""
    from vsdeoldify_amd import stabilizer as S
    assert S._luma_merge_mode(0.3, 0.7) == (1, 76, round(1 / (178 - 76), 3)) and S._luma_merge_mode(0.1, 0.1) == (0, 26, 0.0)
    assert S._luma_merge_mode(0.0, 0.0)[0] == 3 and S._luma_merge_mode(0.0, 0.6)[0] == 2 and S._luma_merge_mode(0.7, 0.3)[0] == -1
    assert S._luma_merge_mode(0.3, 0.32) == (1, 72, round(1 / 10, 3))                       # tresh = min(76, 82 - 10)
    d = S._dark_stage(0.2, 0.8, "280:360,0:30")
    assert (d.kind, d.merge_mode, d.tresh, d.n_ranges, list(d.hue_ranges[:4])) == (0, 1, 26, 2, [280.0, 360.0, 0.0, 30.0])
    assert d.brightness == ctypes.c_float(1 - 0.8 / 255).value and d.color == ctypes.c_float(1.1 - 0.8).value and d.hue_offset == 0
    assert S._dark_stage(0.05, 1.0).merge_mode == 0                                          # threshold clamped to 0.1 == the dark limit: hard mask
    s = S._chroma_stage(0.9, -0.0, "none", (0.3, 0.7))
    assert (s.kind, s.identity, s.has_adjust, s.merge_mode, s.sat, s.bright) == (1, 0, 0, 1, 0.9, 0.0)
    assert S._chroma_stage(1.0, -0.0, "none", (0.3, 0.7)).identity == 1                      # np_image_chroma_tweak returns its input (restcolor.py:290-291)
    assert S._chroma_stage(1.0, 0.0, "", (0.3, 0.7)).identity == 0
    c = S._chroma_stage(hue_adjust="300:360,0:20|+40,0.90")
    assert (c.merge_mode, c.has_adjust, c.n_ranges, c.adj_hue, c.adj_sat, c.adj_weight, c.identity) == (-1, 1, 2, 40, 1.0, 0.9, 0)
    with pytest.raises(ValueError):
        S._dark_stage(0.2, 0.8, ",".join(["0:10"] * 9))


def test_stage_struct_and_signature_match_the_header(tmp_path):
    fields = [n for n, _ in nat.StabStage._fields_]
    src = tmp_path / "st.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "havc_mi355.h"\nint main(){printf("%zu", sizeof(havc_stab_stage));\n' +
                   "".join(f'printf(" %zu", offsetof(havc_stab_stage, {n}));\n' for n in fields) + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "st"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(nat.StabStage)] + [getattr(nat.StabStage, n).offset for n in fields]
    # every member of the C struct is mirrored, in order
    text = open(HEADER).read()
    body = text[text.index("typedef struct havc_stab_stage {"):text.index("} havc_stab_stage;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decl = [n for stmt in body.split("{", 1)[1].split(";") for n in re.findall(r"(\w+)(?:\[\d+\])?\s*(?:,|$)", stmt.strip())]
    assert decl == fields, (decl, fields)
    # the prototype against the ctypes signature
    proto = re.search(r"int havc_stabilizer_chain\(([^)]*)\)", text).group(1)
    kinds = [ctypes.c_void_p if "*" in a else {"int": ctypes.c_int}[a.split()[0]] for a in proto.split(",")]
    sym = {n: (r, a) for n, r, a in nat.SYMBOLS}["havc_stabilizer_chain"]
    assert sym == (ctypes.c_int, kinds)
    assert hasattr(nat.load(), "havc_stabilizer_chain")


def test_build_stamp_covers_the_new_sources():
    """tools/build_stamp.py hashes every source of the library, the new translation unit and the shared header included: the build-stamp test of
    tests/test_host_logic.py then holds the shipped binary to them"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import build_stamp
    names = {os.path.basename(p) for p in build_stamp.source_files()}
    assert {"stabilizer.hip", "pixel_ops.h", "tweaks.hip", "colorfilters.hip"} <= names
    assert nat.load().havc_build_stamp().decode() == build_stamp.stamp()
    mk = open(os.path.join(ROOT, "vsdeoldify_amd", "csrc", "Makefile")).read()
    assert re.search(r"^OBJS = .*\bstabilizer\.o\b", mk, re.M)
    assert re.search(r"^stabilizer\.o:.*\n\t.*-ffp-contract=off", mk, re.M)                   # the bytes move otherwise


def test_everything_off_graph_tolerates_flipped_spline64_ties():
    """The GPU test of HAVC_stabilizer with every filter off compares against the all-oracle graph under `max <= 1, share of differing bytes < 2e-4`
    (the Spline64 .5-boundary condition of tests/test_havc_harness.py).  On the CPU twin of the resample (oracle/resample.py): round EVERY value of both
    passes that lies within 1e-4 of a .5 boundary the other way -- two orders of magnitude wider than the fp32 accumulation error of a 9- or 41-tap sum
    of u8 values -- and the graph's output on that test's frame stays inside the condition."""
    from oracle import pipeline, resample
    from tests.test_havc_harness import _frame
    f = _frame(3)
    h, w = f.shape[:2]
    fs = havc._stabilizer_frame_size(24, w)[1]

    def flipped(x):
        near = np.abs(x - np.floor(x) - 0.5) < 1e-4
        up = np.floor(x + np.float32(0.5))
        return np.clip(np.where(near, np.where(up > x, up - 1, up + 1), up), 0, 255).astype(np.uint8), int(near.sum())
    want = pipeline.post_process(resample.resize_rgb8(resample.resize_rgb8(f, fs, fs), w, h), f)
    sq, n1 = flipped(resample.resize_rgb8_float(f, fs, fs))
    up, n2 = flipped(resample.resize_rgb8_float(sq, w, h))
    assert n1 > 0 and n2 > 0                                                     # the perturbation is not empty
    d = np.abs(pipeline.post_process(up, f).astype(int) - want.astype(int))
    assert d.max() <= 1 and (d > 0).mean() < 2e-4, (int(d.max()), float((d > 0).mean()))
