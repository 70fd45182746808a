"""-m gpu: havc_planes_to_rgb24 / havc_rgb24_to_planes (csrc/vformat.hip) and convert_format_RGB24 / restore_format (vsdeoldify_amd/vformat.py) against the
numpy definition of tests/vformat_util.py: every comparison is byte-equal, and both operands are the definition and the library.

Shapes, n x h x w:   2 x 2 x 2, 2 x 6 x 10   planes narrower than the resampler: every tap mirrored, some more than once
                     3 x 70 x 134            crosses a 64-row band and a 64-step chunk, cw = 67 is odd          1 x 130 x 66   three bands
                     1 x 2 x 4096            the side limit (the error row in LDS)                               1 x 7 x 9      odd sizes (4:4:4, GRAY)
                     5 x 6 x 10 with chunk_frames = 2: a ragged last chunk
Content: seeded random codes over the whole code range (so codes outside a limited range are in every clip), plus planes of 0 and the maximum code only, and
RGB of 0 and 255 only, where every clamp is hit."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

from tests import tweak_util as TU
from tests import vformat_util as U
from vsdeoldify_amd import _native as nat
from vsdeoldify_amd import tweak as TW
from vsdeoldify_amd import vformat as VF
from vsdeoldify_amd.device import DeviceImage

pytestmark = pytest.mark.gpu

S420 = [(2, 2, 2), (2, 6, 10), (3, 70, 134), (1, 130, 66), (1, 2, 4096)]
FORMAT_SHAPES = ([("YUV420P8", s) for s in S420] + [("YUV420P10", s) for s in S420] +
                 [(f, s) for f in ("YUV422P8", "YUV422P10") for s in ((2, 6, 10), (3, 70, 134))] +
                 [(f, s) for f in ("YUV444P8", "YUV444P10", "GRAY8", "GRAY16") for s in ((1, 7, 9), (3, 70, 134))] + [("YUV420P16", (2, 6, 10))])
STEPS = dict(matrix="709", full_range=False, depth_full_range=False, dither=True)


def _same(got, want, what):
    got = got.numpy() if hasattr(got, "numpy") else got
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, len(bad), bad[0].tolist(), int(got[tuple(bad[0])]), int(want[tuple(bad[0])]))


@functools.lru_cache(maxsize=None)
def _planes(fmt, shape, extremes=False):
    f = VF.FORMATS[fmt]
    return U.make_planes(f["bits"], f["sub_w"], f["sub_h"], *shape, gray=f["family"] == "GRAY", extremes=extremes)


@functools.lru_cache(maxsize=None)
def _rgb(shape, extremes=False):
    n, h, w = shape
    clip = TU.make_clip(h, w, n)
    return (np.random.default_rng(h + w).integers(0, 2, clip.shape) * 255).astype(np.uint8) if extremes else clip


def _steps(**kw):
    return dict(STEPS, **kw)


def _key(steps):
    return tuple(sorted(steps.items()))


@functools.lru_cache(maxsize=None)
def _ref_to_rgb(fmt, shape, key, extremes=False):
    f, s = VF.FORMATS[fmt], dict(key)
    planes = _planes(fmt, shape, extremes)
    if f["family"] == "GRAY":
        return U.gray_to_rgb(planes[0], f["bits"], s["depth_full_range"])
    return U.planes_to_rgb(*planes, f["sub_w"], f["sub_h"], f["bits"], s["matrix"], s["full_range"], s["depth_full_range"], s["dither"])


@functools.lru_cache(maxsize=None)
def _ref_from_rgb(fmt, shape, key, extremes=False):
    f, s = VF.FORMATS[fmt], dict(key)
    return U.rgb_to_planes(_rgb(shape, extremes), f["sub_w"], f["sub_h"], f["bits"], s["matrix"], s["full_range"], s["dither"])


def _to_rgb(ctx, fmt, shape, steps, extremes=False, **kw):
    return VF.planes_to_rgb24_np(ctx, VF.VideoClip(_planes(fmt, shape, extremes), fmt), steps, **kw)


def _check_both(ctx, fmt, shape, steps, extremes=False, **kw):
    gray = VF.FORMATS[fmt]["family"] == "GRAY"
    if gray:
        steps = dict(steps, dither=False)
    _same(_to_rgb(ctx, fmt, shape, steps, extremes, **kw), _ref_to_rgb(fmt, shape, _key(steps), extremes), ("to_rgb", fmt, shape, steps))
    if not gray:
        fsteps = dict(steps, depth_full_range=False)
        got = VF.rgb24_to_planes_np(ctx, _rgb(shape, extremes), fmt, fsteps, **kw)
        for name, g, r in zip("yuv", got, _ref_from_rgb(fmt, shape, _key(fsteps), extremes)):
            _same(g, r, ("from_rgb", name, fmt, shape, steps))


@pytest.mark.parametrize("fmt,shape", FORMAT_SHAPES, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_formats_and_shapes(ctx, fmt, shape):
    _check_both(ctx, fmt, shape, STEPS)


@pytest.mark.parametrize("matrix", list(VF.MATRIX_CODES))
def test_matrices_ranges_dither_modes(ctx, matrix):
    for full, dither in itertools.product((False, True), (False, True)):
        _check_both(ctx, "YUV420P8", (2, 6, 10), _steps(matrix=matrix, full_range=full, dither=dither))
    _check_both(ctx, "YUV422P10", (2, 6, 10), _steps(matrix=matrix, full_range=True, depth_full_range=True))


@pytest.mark.parametrize("fmt", ["YUV420P8", "YUV420P10", "YUV422P8", "YUV444P10", "GRAY16"])
def test_undithered_bands_and_depth_ranges(ctx, fmt):
    """dither = 0: the bands of the back kernel become blocks of their own and the way forward goes through the tiled kernel: a shape with more than one band
    and more than one tile, odd and tiny ones, the side limit; and the depth step in both ranges"""
    _check_both(ctx, fmt, (3, 70, 134), _steps(dither=False, depth_full_range=fmt.endswith("10") or fmt.endswith("16")))
    small = (1, 7, 9) if VF.FORMATS[fmt]["sub_w"] == 0 else (2, 6, 10)
    _check_both(ctx, fmt, small, _steps(depth_full_range=True))
    _check_both(ctx, fmt, small, _steps(dither=False))
    if VF.FORMATS[fmt]["sub_h"]:
        _check_both(ctx, fmt, (1, 2, 4096), _steps(dither=False))


@pytest.mark.parametrize("fmt", ["YUV420P10", "YUV444P8", "YUV422P16", "GRAY8"])
def test_every_clamp(ctx, fmt):
    """planes of 0 and the maximum code in a limited-range clip, RGB of 0 and 255 into a full-range clip: the clamps of the depth step, of both roundings and
    of the error diffusion at both ends"""
    shape = (2, 6, 10)
    _check_both(ctx, fmt, shape, STEPS, extremes=True)
    _check_both(ctx, fmt, shape, _steps(full_range=True, depth_full_range=True), extremes=True)
    _check_both(ctx, fmt, shape, _steps(full_range=True, dither=False), extremes=True)


def test_ragged_last_chunk(ctx):
    for fmt in ("YUV420P10", "YUV444P8", "GRAY16"):
        _check_both(ctx, fmt, (5, 6, 10), STEPS, chunk_frames=2)


def test_second_call_gives_the_same_bytes(ctx):
    fmt, shape = "YUV420P10", (3, 70, 134)
    for _ in range(2):
        _check_both(ctx, fmt, shape, STEPS)


def _vf(fmt, shape, steps):
    return VF._vformat(VF.FORMATS[fmt], *shape, steps, steps["depth_full_range"])


def test_operand_kinds(ctx):
    """every pointer host or device on its own: all 16 mixes of each call give the all-host bytes (which test_formats_and_shapes ties to the definition)"""
    fmt, shape = "YUV420P10", (2, 6, 10)
    n, h, w = shape
    planes, rgb = _planes(fmt, shape), _rgb(shape)
    want_rgb, want_planes = _ref_to_rgb(fmt, shape, _key(STEPS)), _ref_from_rgb(fmt, shape, _key(STEPS))
    p = _vf(fmt, shape, STEPS)
    for kinds in itertools.product("hd", repeat=4):
        # planes -> RGB24
        ins = [VF.DevicePlane.from_numpy(ctx, q) if k == "d" else q for q, k in zip(planes, kinds)]
        out = DeviceImage(ctx, (n, h, w, 3)) if kinds[3] == "d" else np.zeros((n, h, w, 3), np.uint8)
        nat.check(ctx.lib.havc_planes_to_rgb24(ctx.h, *[VF._plane_ptr(q) for q in ins], out.ptr if kinds[3] == "d" else nat.as_ptr(out), C.byref(p)), ctx.h)
        _same(out, want_rgb, ("to_rgb", kinds))
        # RGB24 -> planes
        src = DeviceImage.from_numpy(ctx, rgb) if kinds[0] == "d" else rgb
        outs = [VF.DevicePlane(ctx, q.shape, q.dtype) if k == "d" else np.zeros_like(q) for q, k in zip(planes, kinds[1:])]
        nat.check(ctx.lib.havc_rgb24_to_planes(ctx.h, src.ptr if kinds[0] == "d" else nat.as_ptr(src), *[VF._plane_ptr(q) for q in outs], C.byref(p)), ctx.h)
        for name, g, r in zip("yuv", outs, want_planes):
            _same(g, r, ("from_rgb", name, kinds))


def test_equal_to_the_tweak_conversions_on_the_device(ctx):
    """709 / full / 8 bit / 4:2:0: havc_planes_to_rgb24 with dither = havc_yuv420_to_rgb, havc_rgb24_to_planes without = havc_rgb_to_yuv420"""
    shape = (3, 70, 134)
    planes, rgb = _planes("YUV420P8", shape), _rgb(shape)
    full = _steps(full_range=True)
    _same(_to_rgb(ctx, "YUV420P8", shape, full), TW.yuv420_to_rgb_np(ctx, *planes), "back")
    _same(_to_rgb(ctx, "YUV420P8", shape, full), _ref_to_rgb("YUV420P8", shape, _key(full)), "back, definition")
    fwd = _steps(full_range=True, dither=False)
    for name, g, r, d in zip("yuv", VF.rgb24_to_planes_np(ctx, rgb, "YUV420P8", fwd), TW.rgb_to_yuv420_np(ctx, rgb), _ref_from_rgb("YUV420P8", shape, _key(fwd))):
        _same(g, r, ("forward", name))
        _same(g, d, ("forward, definition", name))


def test_invalid_fields_run_nothing(ctx):
    fmt, shape = "YUV420P8", (1, 6, 10)
    planes, rgb = _planes(fmt, shape), _rgb(shape)
    out = np.full(shape + (3,), 7, np.uint8)
    bad = [dict(width=0), dict(height=4097), dict(n_frames=0), dict(family=2), dict(sub_w=0, sub_h=1), dict(sub_w=2), dict(width=9), dict(height=5), dict(bits=7),
           dict(bits=17), dict(matrix=2), dict(matrix=7), dict(full_range=2), dict(depth_full_range=-1), dict(dither=2), dict(chunk_frames=-1), dict(reserved=1),
           dict(family=1), dict(family=1, sub_w=0, sub_h=0)]                                         # GRAY with subsampling; GRAY with a dither
    for kw in bad:
        p = _vf(fmt, shape, STEPS)
        for k, v in kw.items():
            setattr(p, k, v)
        with pytest.raises(ValueError, match="invalid argument"):
            nat.check(ctx.lib.havc_planes_to_rgb24(ctx.h, *[nat.as_ptr(q) for q in planes], nat.as_ptr(out), C.byref(p)), ctx.h)
        assert (out == 7).all(), kw
    outs = [np.full_like(q, 7) for q in planes]
    for kw in bad[:17] + [dict(family=1, sub_w=0, sub_h=0, dither=0), dict(depth_full_range=1)]:   # GRAY is no destination; the depth step belongs to the other call
        p = _vf(fmt, shape, STEPS)
        for k, v in kw.items():
            setattr(p, k, v)
        with pytest.raises(ValueError, match="invalid argument"):
            nat.check(ctx.lib.havc_rgb24_to_planes(ctx.h, nat.as_ptr(rgb), *[nat.as_ptr(q) for q in outs], C.byref(p)), ctx.h)
        assert all((q == 7).all() for q in outs), kw
    p = _vf(fmt, shape, STEPS)
    assert ctx.lib.havc_planes_to_rgb24(ctx.h, nat.as_ptr(planes[0]), None, nat.as_ptr(planes[2]), nat.as_ptr(out), C.byref(p)) != 0 and (out == 7).all()


CLIPS = [("YUV420P10", None, None, (3, 70, 134)), ("YUV422P8", "470bg", "full", (2, 6, 10)), ("YUV444P16", "2020ncl", "limited", (1, 7, 9)),
         ("GRAY16", None, "full", (2, 6, 10)), ("GRAY8", "170m", None, (2, 6, 10))]


@pytest.mark.parametrize("fmt,matrix,color_range,shape", CLIPS)
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_convert_then_restore_through_python(ctx, fmt, matrix, color_range, shape, device):
    """convert_format_RGB24 -> restore_format equals the definition's composition; the quirks come from the pinned plans (a full-range clip converted as
    limited, the depth step in the clip's own range, GRAY back as YUV420P8 in the original's range)"""
    planes = _planes(fmt, shape)
    want_rgb = U.convert(planes, fmt, matrix, color_range)
    want_fmt, want_planes = U.restore(want_rgb, fmt, matrix, color_range)
    clip = VF.VideoClip([VF.DevicePlane.from_numpy(ctx, p) for p in planes] if device else planes, fmt, matrix, color_range)
    rgb, info = VF.convert_format_RGB24(clip)
    assert isinstance(rgb, DeviceImage) == device and info == VF.ClipInfo(None, **VF.clip_info_fields(fmt, matrix, color_range))
    _same(rgb, want_rgb, ("convert", fmt))
    back = VF.restore_format(rgb, info)
    family = VF.FORMATS[fmt]["family"]
    assert back.format == want_fmt == ("YUV420P8" if family == "GRAY" else fmt) and back.on_device == device
    assert back.matrix == ("709" if family == "GRAY" else matrix or "709") and back.color_range == (color_range or "limited")
    for name, g, r in zip("yuv", back.planes, want_planes):
        _same(g, r, ("restore", name, fmt))
    if not device:                                                                                  # host planes, RGB on the device: the upload is the planes
        rgb_d, _ = VF.convert_format_RGB24(clip, rgb_on_device=True)
        assert isinstance(rgb_d, DeviceImage)
        _same(rgb_d, want_rgb, ("convert, rgb_on_device", fmt))
        for name, g, r in zip("yuv", VF.restore_format(rgb_d, info).planes, want_planes):
            assert isinstance(g, VF.DevicePlane)
            _same(g, r, ("restore from the device", name, fmt))


def test_rgb24_passes_on_the_device(ctx):
    clip = DeviceImage.from_numpy(ctx, _rgb((2, 6, 10)))
    rgb, info = VF.convert_format_RGB24(clip)
    assert rgb is clip and info.format_id == "RGB24" and VF.restore_format(rgb, info) is clip
