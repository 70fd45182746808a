"""CPU (-m "not gpu"): HAVC_clip_slice / HAVC_clip_reconstruct (vsdeoldify/__init__.py:2886-2945, vsslib/vstiles4.py) -- the numpy restatement the GPU
tests compare against (tests/tiles_util.py) is pinned to the executed reference (tests/golden/tiles.npz) for the slice and to the stated mask / rounding
rules for the reconstruct; the argument rules run before any GPU context exists; the C struct, its ctypes mirror and the signatures agree."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from tests import tiles_util as U
from tests.conftest import ROOT
from vsdeoldify_amd import _native as nat
from vsdeoldify_amd import havc

HEADER = os.path.join(ROOT, "include", "havc_mi355.h")
WEIGHTS = (0, 0.001, 0.3, 0.5, 1.0)


def test_restated_slice_reproduces_the_executed_reference():
    g, cases = U.fixture()
    assert "executing the reference" in str(g["provenance"])
    sizes = {tuple(g[f"in_{c['input']}"].shape[1:3]) for c in cases}
    assert {(37, 51), (36, 48), (54, 96)} <= sizes and any(h == 1 for h, _ in sizes)
    assert {c["overlap_x"] for c in cases} == {0, 2, 7, 32} and {c["slices"] for c in cases} == {2, 4}
    for k, c in enumerate(cases):
        clip = g[f"in_{c['input']}"]
        tiles, *numbers = U.slice_np(clip, c["slices"], c["overlap_x"], c["overlap_y"])
        assert numbers == c["numbers"], (c, numbers)
        assert numbers == list(havc._tile_geometry(clip.shape[2], clip.shape[1], c["slices"], c["overlap_x"], c["overlap_y"])[1:]), c
        want = U.fixture_tiles(g, k, c["slices"])
        assert len(tiles) == len(want) == c["slices"]
        for t, (a, b) in enumerate(zip(tiles, want)):
            assert a.shape == b.shape and np.array_equal(a, b), (c, t)
    assert any(c["overlap_x"] == 7 and c["numbers"][2] == 6 for c in cases)                      # rounded down to even
    assert all(c["numbers"][3] == 0 and c["numbers"][1] == g[f"in_{c['input']}"].shape[1] for c in cases if c["slices"] == 2)


def test_mask_values():
    base, ov = 26, 6
    start, end = base - ov, base + ov
    ramp = U.blend_mask(2 * base, ov, base, 0)
    assert (ramp[:start + 1] == 0).all() and ramp[start] == 0 and (ramp[base:] == 255).all()
    assert (np.diff(ramp) >= 0).all() and ramp.min() == 0 and ramp.max() == 255
    assert list(ramp[start:base + 1]) == [0, 43, 85, 128, 170, 213, 255]                         # floor(k * 255 / 6 + 0.5): divides by the overlap, not twice it
    assert np.array_equal(U.blend_mask(2 * base, ov, base, 0.001), ramp)                         # int(round(0.255)) == 0: still the ramp
    for w, v in ((0.5, 128), (1.0, 255), (0.3, 76), (0.002, 1)):
        m = U.blend_mask(2 * base, ov, base, w)
        assert (m[:start] == 0).all() and (m[start:end] == v).all() and (m[end:] == 255).all(), w
    # the stand-in of MaskedMerge: exact at both ends, symmetric rounding in between
    a, b = np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8)[::-1].copy()
    assert np.array_equal(U.masked_merge(a, b, 0), a) and np.array_equal(U.masked_merge(a, b, 255), b)
    assert np.array_equal(U.masked_merge(a, a, 77), a)                                           # equal operands blend to themselves
    assert U.masked_merge(np.uint8([0]), np.uint8([255]), 128)[0] == 128 and U.masked_merge(np.uint8([10]), np.uint8([13]), 128)[0] == 12


def test_two_stage_rounding_is_not_one_stage():
    """top = H(tl, tr) and bottom = H(bl, br) are rounded to uint8 before V(top, bottom): on random tiles that differs from one rounding of the bilinear sum"""
    r = np.random.default_rng(5)
    base_w, base_h, ox, oy = 10, 9, 4, 4
    tiles = [r.integers(0, 256, (1, base_h + oy, base_w + ox, 3), dtype=np.uint8) for _ in range(4)]
    got = U.reconstruct_np(tiles, None, base_w, base_h, ox, oy, 0.3)
    assert got.shape == (1, 2 * base_h, 2 * base_w, 3)
    mx, my = U.blend_mask(2 * base_w, ox, base_w, 0.3), U.blend_mask(2 * base_h, oy, base_h, 0.3)
    y, x = base_h, base_w                                                                        # inside both overlaps: all four tiles meet
    px = [t[0, yy, xx].astype(np.int64) for t, yy, xx in ((tiles[0], y, x), (tiles[1], y, x - (base_w - ox)), (tiles[2], y - (base_h - oy), x),
                                                           (tiles[3], y - (base_h - oy), x - (base_w - ox)))]
    top = (px[0] * (255 - mx[x]) + px[1] * mx[x] + 127) // 255
    bot = (px[2] * (255 - mx[x]) + px[3] * mx[x] + 127) // 255
    assert np.array_equal(got[0, y, x], (top * (255 - my[y]) + bot * my[y] + 127) // 255)
    zone = got[0, base_h - oy:base_h + oy, base_w - ox:base_w + ox].astype(np.int64)
    fx = mx[base_w - ox:base_w + ox, None] / 255.0
    fy = my[base_h - oy:base_h + oy, None, None] / 255.0
    t4 = [t[0].astype(np.float64) for t in tiles]
    one = ((t4[0][base_h - oy:base_h + oy, base_w - ox:] * (1 - fx) + t4[1][base_h - oy:base_h + oy, :2 * ox] * fx) * (1 - fy) +
           (t4[2][:2 * oy, base_w - ox:] * (1 - fx) + t4[3][:2 * oy, :2 * ox] * fx) * fy)
    assert (zone != np.floor(one + 0.5)).any() and np.abs(zone - one).max() <= 1.0


@pytest.mark.parametrize("slices", [2, 4])
def test_restated_reconstruct_of_a_slice_is_the_clip(slices):
    """equal operands blend to themselves, so whatever the mask the overlap zones reproduce the clip; everything else is copied"""
    for seed, (n, h, w) in enumerate([(2, 37, 51), (1, 36, 48), (1, 6, 10)]):
        clip = U.clip(seed, n, h, w)
        for ox in (0, 2, 6):
            if ox >= (w + 1) // 2 or (slices == 4 and ox >= (h + 1) // 2):
                continue
            tiles, bw, bh, rx, ry = U.slice_np(clip, slices, ox, ox)
            for weight in WEIGHTS:
                assert np.array_equal(U.reconstruct_np(tiles, clip, bw, bh, rx, ry, weight), clip), (h, w, ox, weight)


def test_argument_rules_run_before_any_context():
    f = np.zeros((2, 20, 30, 3), np.uint8)
    for bad in ("not a clip", None, [[1, 2, 3]]):
        with pytest.raises(havc.HAVCError, match="HAVC_clip_slice: this is not a clip"):
            havc.HAVC_clip_slice(bad)
    with pytest.raises(havc.HAVCError):
        havc.HAVC_clip_slice(np.zeros((8, 8), np.uint8))                                         # not RGB24
    for kw in (dict(overlap_x=16), dict(overlap_x=32), dict(overlap_x=-1), dict(overlap_x=-2), dict(slices=4, overlap_x=40, overlap_y=2)):
        with pytest.raises(havc.HAVCError, match="HAVC_clip_slice: overlap_x = -?\\d+ must be >= 0 and smaller than the base tile width 15"):
            havc.HAVC_clip_slice(f, **kw)
    for oy in (10, 11, 32, -1):
        with pytest.raises(havc.HAVCError, match="HAVC_clip_slice: overlap_y = -?\\d+ must be >= 0 and smaller than the base tile height 10"):
            havc.HAVC_clip_slice(f, slices=4, overlap_x=2, overlap_y=oy)
    assert havc._tile_geometry(30, 20, 2, 15, 99) == (2, 15, 20, 14, 0)                          # 15 rounds down to 14; overlap_y is not looked at for 2 tiles
    assert havc._tile_geometry(30, 20, 3, 2, -5) == (2, 15, 20, 2, 0)                            # the reference's `else`: anything but 4 = 2 tiles
    assert havc._tile_geometry(51, 37, 4, 7, 7) == (4, 26, 19, 6, 6)
    assert havc._tile_geometry(1920, 1080, 4, 192.0, 108.0) == (4, 960, 540, 192, 108)             # floats, as HAVC_main computes them (__init__.py:761-762)

    t = np.zeros((2, 20, 17, 3), np.uint8)
    ok = havc.ClipTiles(clip_orig=f, tiles=[t, t], base_tile_w=15, base_tile_h=20, overlap_x=2, overlap_y=0)
    for n in (0, 1, 3, 5):
        with pytest.raises(havc.HAVCError, match=f"HAVC_clip_reconstruct: 2 or 4 tiles expected, got {n}"):
            havc.HAVC_clip_reconstruct(havc.ClipTiles(f, [t] * n, 15, 20, 2, 0))
    with pytest.raises(havc.HAVCError, match="chroma_resize=True needs clip_orig"):
        havc.HAVC_clip_reconstruct(havc.ClipTiles(None, [t, t], 15, 20, 2, 0), chroma_resize=True)
    with pytest.raises(havc.HAVCError, match="this is not a clip: tiles"):
        havc.HAVC_clip_reconstruct(havc.ClipTiles(f, [t, None], 15, 20, 2, 0))
    with pytest.raises(havc.HAVCError, match="this is not a clip: clip_orig"):
        havc.HAVC_clip_reconstruct(havc.ClipTiles("clip", [t, t], 15, 20, 2, 0))
    for w in (-0.1, 1.01, 2):
        with pytest.raises(havc.HAVCError, match="blend_weight must be between 0 and 1"):
            havc.HAVC_clip_reconstruct(ok, blend_weight=w)
    with pytest.raises(havc.HAVCError, match="does not match base tile \\+ overlap"):
        havc.HAVC_clip_reconstruct(havc.ClipTiles(f, [t, t[:, :, :16]], 15, 20, 2, 0))
    with pytest.raises(havc.HAVCError, match="does not match base tile \\+ overlap"):
        havc.HAVC_clip_reconstruct(havc.ClipTiles(f, [t, t[:1]], 15, 20, 2, 0))                  # another frame count
    with pytest.raises(havc.HAVCError, match="an overlap must be smaller than the base tile"):
        havc.HAVC_clip_reconstruct(havc.ClipTiles(f, [t, t], 15, 20, 16, 0))
    with pytest.raises(havc.HAVCError, match="is not covered by the tiles"):
        havc.HAVC_clip_reconstruct(havc.ClipTiles(np.zeros((2, 20, 31, 3), np.uint8), [t, t], 15, 20, 2, 0))
    with pytest.raises(havc.HAVCError, match="is not covered by the tiles"):
        havc.HAVC_clip_reconstruct(havc.ClipTiles(f[:1], [t, t], 15, 20, 2, 0))


def test_tiled_preset_params():
    """__init__.py:761-764 by hand: 1920 x 1080 -> 0.2 * 960 = 192 and 0.2 * 540 = 108 (both at their caps), trunc((960 + 192) / 16) = 72 -> 32;
    720 x 576 -> 72 and max(57.6, 64) = 64, trunc((360 + 72) / 16) = 27"""
    for slices in (2, 4):
        assert havc.tiled_preset_params(1920, 1080, slices) == (192, 108, 32)
        assert havc.tiled_preset_params(720, 576, slices) == (72, 64, 27)
        assert all(type(v) is int for v in havc.tiled_preset_params(725, 577, slices))
    assert havc.tiled_preset_params(725, 480, 4) == (72, 64, 27)                                 # round(72.5) = 72 (half to even), trunc(434.5 / 16) = 27
    assert havc.tiled_preset_params(320, 240, 2) == (64, 64, 22)                                 # both floors: 64 pixels, render factor 22


def test_public_functions_are_exported_with_the_reference_argument_lists():
    import dataclasses

    import vsdeoldify_amd
    for name in ("HAVC_clip_slice", "HAVC_clip_reconstruct", "ClipTiles", "tiled_preset_params"):
        assert getattr(vsdeoldify_amd, name) is getattr(havc, name)
    p = inspect.signature(havc.HAVC_clip_slice).parameters
    assert [(k, v.default) for k, v in p.items()][1:] == [("slices", 2), ("overlap_x", 32), ("overlap_y", 32)] and list(p)[0] == "clip"
    p = inspect.signature(havc.HAVC_clip_reconstruct).parameters
    assert [(k, v.default) for k, v in p.items()][1:] == [("blend_weight", 0.5), ("chroma_resize", False)] and list(p)[0] == "clip_tiles"
    assert [f.name for f in dataclasses.fields(havc.ClipTiles)] == ["clip_orig", "tiles", "base_tile_w", "base_tile_h", "overlap_x", "overlap_y"]
    ct = havc.ClipTiles(None, [1, 2], 3, 4, 0, 0)
    ct.tiles[1] = 5                                                                              # __init__.py:865 overwrites the tiles in place
    assert ct.tiles == [1, 5]
    assert "MaskedMerge" in havc.__doc__ and "resize_to_chroma" in havc.__doc__                 # the two stand-ins are named where the others are


def test_geometry_struct_and_signatures_match_the_header(tmp_path):
    fields = [n for n, _ in nat.TileGeom._fields_]
    src = tmp_path / "tg.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "havc_mi355.h"\nint main(){printf("%zu", sizeof(havc_tile_geom));\n' +
                   "".join(f'printf(" %zu", offsetof(havc_tile_geom, {n}));\n' for n in fields) + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "tg"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(nat.TileGeom)] + [getattr(nat.TileGeom, n).offset for n in fields]
    text = open(HEADER).read()
    body = text[text.index("typedef struct havc_tile_geom {"):text.index("} havc_tile_geom;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decl = [n for stmt in body.split("{", 1)[1].split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", stmt.strip())]
    assert decl == fields, (decl, fields)
    syms = {n: (r, a) for n, r, a in nat.SYMBOLS}
    for name in ("havc_tile_slice", "havc_tile_reconstruct"):
        proto = re.search(r"int %s\(([^)]*)\)" % name, text).group(1)
        assert all("*" in a for a in proto.split(","))
        assert syms[name] == (ctypes.c_int, [ctypes.c_void_p] * len(proto.split(",")))
        assert hasattr(nat.load(), name)


def test_build_covers_the_new_translation_unit():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import build_stamp
    assert "tiles.hip" in {os.path.basename(p) for p in build_stamp.source_files()}
    mk = open(os.path.join(ROOT, "vsdeoldify_amd", "csrc", "Makefile")).read()
    assert re.search(r"^OBJS = .*\btiles\.o\b", mk, re.M)
    assert re.search(r"^tiles\.o:.*pixel_ops\.h\n\t.*-ffp-contract=off", mk, re.M)               # every unit that includes pixel_ops.h is built that way
    src = open(os.path.join(ROOT, "vsdeoldify_amd", "csrc", "tiles.hip")).read()
    assert "yuv_merge_pixel(" in src                                                             # the luma re-attach is the shared body, not a copy
    assert "yuv_merge_pixel(" in open(os.path.join(ROOT, "vsdeoldify_amd", "csrc", "colorfilters.hip")).read()
