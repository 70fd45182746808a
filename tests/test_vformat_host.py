"""No GPU: vsdeoldify_amd/vformat.py against tests/golden/vformat.json (the reference's convert_format_RGB24 / restore_format EXECUTED against a recording
vapoursynth stand-in, tools/gen_golden_vformat.py), the refusals, the numpy definition tests/vformat_util.py against tests/tweak_util.py where the two
overlap (709 / full / 8 bit / 4:2:0), and the bindings against the header."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from tests import tweak_util as TU
from tests import vformat_util as U
from vsdeoldify_amd import _native as nat
from vsdeoldify_amd import vformat as VF
from vsdeoldify_amd.havc import HAVCError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "vformat.json")))
CASES = GOLDEN["cases"]


def test_fixture_covers_every_supported_format_and_prop():
    seen = {(c["format"], c["matrix"], c["color_range"]) for c in CASES}
    want = {(f, m, r) for f in VF.FORMATS for m in (None,) + tuple(VF.MATRIX_CODES) for r in (None, "limited", "full")}
    assert seen == want and len(CASES) == len(want) == 15 * 5 * 3


@pytest.mark.parametrize("fmt", list(VF.FORMATS))
def test_plans_and_clip_info_equal_the_reference(fmt):
    for c in (c for c in CASES if c["format"] == fmt):
        key = (fmt, c["matrix"], c["color_range"])
        assert "error" not in c["convert"] and "error" not in c["restore"], key
        assert VF.convert_calls(*key) == c["convert"]["calls"], key
        fields = VF.clip_info_fields(*key)
        assert dict(clip_orig=None, **fields) == c["convert"]["info"], key
        assert VF.restore_calls(fields) == c["restore"]["calls"], key
        assert VF.restore_calls(VF.ClipInfo(clip_orig=None, **fields)) == c["restore"]["calls"], key
        if fmt == "RGB24":
            assert c["convert"]["out_format"] == c["restore"]["out_format"] == "RGB24" and c["restore"]["passes"], key
        else:
            assert c["convert"]["out_format"] == "RGB24" and c["convert"]["out_props"]["_Range"] == VF.RANGE_FULL, key
            assert VF.restore_steps(*key)["format"] == c["restore"]["out_format"], key


def test_kept_quirks_show_in_the_steps():
    """what the plans come to as fields of havc_vformat: each quirk of the module docstring once"""
    s = VF.convert_steps("YUV420P10")                                               # missing props: 709, limited
    assert s == dict(matrix="709", full_range=False, depth_full_range=False, dither=True)
    s = VF.convert_steps("YUV422P12", "470bg", "full")                              # the depth step takes the clip's range, the matrix step says limited
    assert s == dict(matrix="470bg", full_range=False, depth_full_range=True, dither=True)
    assert VF.convert_steps("YUV444P8", "2020ncl", "full") == dict(matrix="2020ncl", full_range=False, depth_full_range=True, dither=True)
    assert VF.convert_steps("GRAY16", None, "full") == dict(matrix="709", full_range=False, depth_full_range=True, dither=False)
    assert VF.restore_steps("YUV420P10", "170m", "full") == dict(format="YUV420P10", matrix="170m", full_range=True, dither=True)
    assert VF.restore_steps("YUV444P16") == dict(format="YUV444P16", matrix="709", full_range=False, dither=True)
    assert VF.restore_steps("GRAY8", "2020ncl", "full") == dict(format="YUV420P8", matrix="709", full_range=True, dither=True)
    assert VF.restore_steps("GRAY16") == dict(format="YUV420P8", matrix="709", full_range=False, dither=True)


def _planes(fmt, n=1, h=4, w=6):
    f = VF.FORMATS[fmt]
    dt = np.uint8 if f["bits"] == 8 else np.uint16
    shapes = [(n, h, w)] + ([] if f["family"] == "GRAY" else [(n, h >> f["sub_h"], w >> f["sub_w"])] * 2)
    return tuple(np.zeros(s, dt) for s in shapes)


def test_refusals():
    for fmt in ("RGB48", "RGB30", "RGBS", "YUV444PS", "YUV444PH", "GRAYS", "GRAYH", "YUV410P8", "YUV411P8", "YUV440P8", "YUV420P9", "YUV420P14"):
        with pytest.raises(NotImplementedError):
            VF.VideoClip(_planes("YUV444P8"), fmt)
    with pytest.raises(NotImplementedError):
        VF.VideoClip(_planes("YUV420P8"), "YUV420P8", matrix="240m")
    with pytest.raises(NotImplementedError, match="chroma_resize"):
        VF.convert_format_RGB24(VF.VideoClip(_planes("YUV420P8"), "YUV420P8"), chroma_resize=True)
    bad = [lambda: VF.VideoClip(_planes("YUV420P8"), "NV12"),
           lambda: VF.VideoClip(_planes("YUV420P8"), "YUV420P8", color_range="tv"),
           lambda: VF.VideoClip(_planes("YUV420P8")[:2], "YUV420P8"),
           lambda: VF.VideoClip(_planes("YUV420P8"), "GRAY8"),
           lambda: VF.VideoClip(_planes("YUV420P8"), "YUV420P10"),                                  # dtype
           lambda: VF.VideoClip(_planes("YUV420P10"), "YUV420P8"),
           lambda: VF.VideoClip(_planes("YUV420P8"), "YUV444P8"),                                   # chroma shape
           lambda: VF.VideoClip(_planes("YUV444P8", w=7), "YUV422P8"),                              # odd width with 4:2:x
           lambda: VF.VideoClip(_planes("YUV444P8", h=5), "YUV420P8"),                              # odd height with 4:2:0
           lambda: VF.VideoClip(_planes("GRAY8", h=1, w=4097), "GRAY8"),
           lambda: VF.VideoClip(_planes("GRAY8", h=4097, w=1), "GRAY8"),
           lambda: VF.VideoClip((np.zeros((4, 6), np.uint8),), "GRAY8"),
           lambda: VF.VideoClip(np.zeros((1, 4, 6, 3), np.uint8), "RGB24"),
           lambda: VF.convert_format_RGB24(np.zeros((1, 4, 6), np.uint8)),
           lambda: VF.restore_format(np.zeros((1, 4, 6), np.uint8), VF.ClipInfo(None, **VF.clip_info_fields("YUV420P8"))),
           lambda: VF.restore_format(np.zeros((1, 5, 6, 3), np.uint8), VF.ClipInfo(None, **VF.clip_info_fields("YUV420P8"))),
           lambda: VF.restore_format(np.zeros((1, 4, 7, 3), np.uint8), VF.ClipInfo(None, **VF.clip_info_fields("GRAY8")))]
    for fn in bad:
        with pytest.raises(HAVCError):
            fn()
    VF.VideoClip(_planes("YUV444P8", h=5, w=7), "YUV444P8")                                        # odd sizes are fine without subsampling
    VF.VideoClip(_planes("YUV422P8", h=5), "YUV422P8")
    VF.VideoClip(_planes("GRAY16", h=1, w=4096), "GRAY16")
    # a clip that is not RGB24: the reference's text
    assert GOLDEN["restore_not_rgb24"] == dict(calls=[], error=VF.NOT_RGB24)
    with pytest.raises(HAVCError, match=re.escape(VF.NOT_RGB24)):
        VF.restore_format(VF.VideoClip(_planes("YUV420P8"), "YUV420P8"), VF.ClipInfo(None, **VF.clip_info_fields("YUV420P8")))


def test_rgb24_passes_both_functions_without_a_context():
    clip = np.zeros((2, 4, 6, 3), np.uint8)
    rgb, info = VF.convert_format_RGB24(clip)
    assert rgb is clip and info == VF.ClipInfo(None, "RGB24", "RGB", 8, 1, VF.RANGE_LIMITED, False)
    assert VF.restore_format(rgb, info) is clip


def test_definition_equals_tweak_util_where_they_overlap():
    """709 / full / 8 bit / 4:2:0: the bytes of tweak_util.yuv420_to_rgb (with dither) and of tweak_util.rgb_to_yuv420 (dither = 0)"""
    for h, w, n in ((2, 2, 1), (6, 10, 2), (18, 14, 1)):
        r = np.random.default_rng(h * w + n)
        y, u, v = (r.integers(0, 256, s, dtype=np.uint8) for s in ((n, h, w), (n, h // 2, w // 2), (n, h // 2, w // 2)))
        assert np.array_equal(U.planes_to_rgb(y, u, v, 1, 1, 8, "709", True, False, True), TU.yuv420_to_rgb(y, u, v))
        clip = TU.make_clip(h, w, n)
        for got, want in zip(U.rgb_to_planes(clip, 1, 1, 8, "709", True, False), TU.rgb_to_yuv420(clip)):
            assert got.dtype == np.uint8 and np.array_equal(got, want)
        x = np.stack(TU.yuv420_to_rgb_float(y, u, v))
        assert np.array_equal(U.dither_fs(x, 255), TU.dither_fs(x))


def test_definition_scalings():
    """the written-down scalings at their corners: reference white and black of a limited clip, the depth step, GRAY"""
    for bits in (8, 10, 12, 16):
        step, dt = 1 << (bits - 8), np.uint8 if bits == 8 else np.uint16
        white = np.full((1, 2, 2, 3), 255, np.uint8)
        for dither in (False, True):
            y, u, v = U.rgb_to_planes(white, 0, 0, bits, "709", False, dither)
            assert y.dtype == dt and (y == 235 * step).all() and (u == 128 * step).all() and (v == 128 * step).all()
            y, u, v = U.rgb_to_planes(white, 0, 0, bits, "2020ncl", True, dither)
            assert (y == (1 << bits) - 1).all() and (u == 1 << (bits - 1)).all()
        y = np.array([[[16 * step, 235 * step, 0, (1 << bits) - 1]]], dt)
        c = np.full((1, 1, 4), 128 * step, dt)
        assert U.planes_to_rgb(y, c, c, 0, 0, bits, "170m", False, False, True)[0, 0, :, 1].tolist() == [0, 255, 0, 255]
        assert U.gray_to_rgb(y, bits)[0, 0].tolist() == [[0] * 3, [255] * 3, [0] * 3, [255] * 3]
    assert U.depth_to_8(np.array([0, 2, 6, 1023], np.uint16), 10, False, False).tolist() == [0, 0, 2, 255]          # round half to even, clamp
    assert U.depth_to_8(np.array([0, 512, 1023], np.uint16), 10, True, True).tolist() == [0, 128, 255]
    assert U.depth_to_8(np.array([0, 65535], np.uint16), 16, True, False).tolist() == [0, 255]


def test_header_and_bindings_agree():
    assert ctypes.sizeof(nat.VFormat) == 52                                                         # static_assert of rt_filters.cpp
    header = open(os.path.join(ROOT, "include", "havc_mi355.h")).read()
    body = re.search(r"typedef struct havc_vformat \{(.*?)\} havc_vformat;", header, re.S).group(1)
    fields = [n.strip() for line in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") if line.strip() for n in line.strip()[len("int "):].split(",")]
    assert fields == [n for n, t in nat.VFormat._fields_] and all(t is ctypes.c_int for _, t in nat.VFormat._fields_)
    names = [s[0] for s in nat.SYMBOLS]
    for sym in ("havc_planes_to_rgb24", "havc_rgb24_to_planes"):
        assert re.search(r"\bint " + sym + r"\(", header) and sym in names, sym
    lib = nat.load()
    assert lib.havc_planes_to_rgb24 and lib.havc_rgb24_to_planes
    assert VF.MAX_SIDE == int(re.search(r"#define TW_MAX_SIDE (\d+)", open(os.path.join(ROOT, "vsdeoldify_amd", "csrc", "kernels.h")).read()).group(1))
    import vsdeoldify_amd
    for name in ("VideoClip", "ClipInfo", "convert_format_RGB24", "restore_format"):
        assert getattr(vsdeoldify_amd, name) is getattr(VF, name)
