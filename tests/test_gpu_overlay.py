"""-m gpu: havc_overlay_clip (csrc/overlay.hip) and HAVC_clip_overlay against the numpy definition of tests/overlay_util.py: every comparison is byte-equal.

Base 34 x 66 (more than one block of four-pixel groups, a ragged last group with 3 frames of odd sizes below), overlay 20 x 30 placed inside, at the corner,
hanging off the top left, off the right and bottom, and outside; an overlay larger than the base; every one of the nine modes; no mask, a gray mask, a
3-plane mask with mask_first_plane both ways; opacity 1, 0.5 and 0; planes None, 1 and [0, 2]; a one-frame overlay on a 3-frame base; every (overlay sample,
base sample) pair per mode, which is what catches a division or a rounding that differs."""
import functools

import numpy as np
import pytest

from tests import overlay_util as U
from vsdeoldify_amd import havc
from vsdeoldify_amd.device import DeviceImage

pytestmark = pytest.mark.gpu

PLACES = [(0, 0), (5, 7), (-6, -4), (50, 25), (100, 100)]


def _same(got, want, what):
    bad = np.argwhere(got != want)
    assert got.shape == want.shape and len(bad) == 0, (what, len(bad), bad[0].tolist(), int(got[tuple(bad[0])]), int(want[tuple(bad[0])]))


@functools.lru_cache(maxsize=None)
def _clips():
    return U.make_clip(3, 34, 66, 11), U.make_clip(3, 20, 30, 12), U.make_clip(3, 20, 30, 13)                # base, overlay, 3-plane mask


@pytest.mark.parametrize("mode", U.MODES)
def test_every_mode_at_every_place(ctx, mode):
    base, ov, mask = _clips()
    for x, y in PLACES:
        _same(havc.HAVC_clip_overlay(base, ov, x, y, mode=mode), U.clip_overlay(base, ov, x, y, mode=mode), (mode, x, y, "no mask"))
        _same(havc.HAVC_clip_overlay(base, ov, x, y, mask[..., 1], 0.5, mode.upper()), U.clip_overlay(base, ov, x, y, mask[..., 1], 0.5, mode),
              (mode, x, y, "gray mask, opacity 0.5"))
    _same(havc.HAVC_clip_overlay(base, ov, 100, 100, mode=mode), base, (mode, "outside: the base"))


@pytest.mark.parametrize("mode", U.MODES)
def test_every_pair_of_samples(ctx, mode):
    base, ov = U.pair_sweep()
    _same(havc.HAVC_clip_overlay(base, ov, mode=mode), U.clip_overlay(base, ov, mode=mode), (mode, "opaque"))
    mask = np.arange(256, dtype=np.uint8)[None, None, :].repeat(256, 1)[..., ::-1].copy()
    _same(havc.HAVC_clip_overlay(base, ov, 0, 0, mask, 0.7, mode), U.clip_overlay(base, ov, 0, 0, mask, 0.7, mode), (mode, "mask ramp, opacity 0.7"))


def test_every_mask_sample_with_every_opacity_step(ctx):
    """m and opacity alone: normal mode, overlay 255 on base 0 gives the merged mask back"""
    m = np.arange(256, dtype=np.uint8)[None, None, :].repeat(64, 1)
    base, ov = np.zeros((1, 64, 256, 3), np.uint8), np.full((1, 64, 256, 3), 255, np.uint8)
    for opacity in (0.999, 0.5, 1 / 3, 0.1, 0.002):
        _same(havc.HAVC_clip_overlay(base, ov, 0, 0, m, opacity), U.clip_overlay(base, ov, 0, 0, m, opacity), opacity)


@pytest.mark.parametrize("opacity", [1.0, 0.5, 0.0])
@pytest.mark.parametrize("planes", [None, 1, [0, 2]])
def test_masks_opacity_and_planes(ctx, opacity, planes):
    base, ov, mask = _clips()
    for m, first in ((None, True), (mask[..., 0], True), (mask, True), (mask, False)):
        for mode in ("normal", "overlay", "divide"):
            got = havc.HAVC_clip_overlay(base, ov, 5, 7, m, opacity, mode, planes, first)
            _same(got, U.clip_overlay(base, ov, 5, 7, m, opacity, mode, planes, first), (opacity, planes, None if m is None else m.shape, first, mode))
    if opacity == 0.0:
        _same(havc.HAVC_clip_overlay(base, ov, 5, 7, None, opacity, "addition", planes), base, "opacity 0: the base")


def test_larger_overlay_single_frame_overlay_and_odd_sizes(ctx):
    base, _, _ = _clips()
    big, bigmask = U.make_clip(3, 50, 90, 21), U.make_clip(3, 50, 90, 22)
    for x, y in ((-10, -8), (0, 0), (-60, 3)):
        _same(havc.HAVC_clip_overlay(base, big, x, y, bigmask, 0.8, "exclusion", None, False), U.clip_overlay(base, big, x, y, bigmask, 0.8, "exclusion", None, False),
              ("larger overlay", x, y))
    one, onemask = U.make_clip(1, 20, 30, 23)[0], U.make_clip(1, 20, 30, 24)[0]
    _same(havc.HAVC_clip_overlay(base, one, 40, 20, onemask[..., 0], 0.9, "average"), U.clip_overlay(base, one, 40, 20, onemask[..., 0], 0.9, "average"),
          "one frame, gray mask")
    _same(havc.HAVC_clip_overlay(base, one[None], 40, 20, onemask[None], 1.0, "subtract", None, False),
          U.clip_overlay(base, one[None], 40, 20, onemask[None], 1.0, "subtract", None, False), "one frame [1, h, w, 3], 3-plane mask")
    odd, small = U.make_clip(3, 3, 5, 25), U.make_clip(3, 2, 2, 26)                                          # 45 pixels: a ragged last group
    _same(havc.HAVC_clip_overlay(odd, small, 2, 1, mode="difference"), U.clip_overlay(odd, small, 2, 1, mode="difference"), "3 x 5")
    tiny = U.make_clip(1, 1, 1, 27)
    _same(havc.HAVC_clip_overlay(tiny, tiny[:, :, :, ::-1].copy(), mode="multiply"), U.clip_overlay(tiny, tiny[:, :, :, ::-1], mode="multiply"), "1 x 1")


def test_host_and_device_operands_mix(ctx):
    base, ov, mask = _clips()
    want = U.clip_overlay(base, ov, -6, -4, mask, 0.5, "overlay", None, False)
    dev = lambda a: DeviceImage.from_numpy(ctx, a)
    for b, o, m in ((dev(base), dev(ov), dev(mask)), (dev(base), ov, mask), (base, dev(ov), mask), (base, ov, dev(mask)), (dev(base), ov, dev(mask))):
        got = havc.HAVC_clip_overlay(b, o, -6, -4, m, 0.5, "overlay", None, False)
        assert isinstance(got, DeviceImage) == isinstance(b, DeviceImage)
        _same(got.numpy() if isinstance(got, DeviceImage) else got, want, [type(v).__name__ for v in (b, o, m)])
    got = havc.HAVC_clip_overlay(dev(base), dev(ov), 100, 100)
    assert isinstance(got, DeviceImage)
    _same(got.numpy(), base, "outside, on the device")
    one = dev(ov).frame(1)                                                                                   # a view at an offset
    _same(havc.HAVC_clip_overlay(dev(base), one, 5, 7).numpy(), U.clip_overlay(base, ov[1], 5, 7), "a device frame view as the overlay")


def test_c_abi_refusals(ctx):
    import ctypes as C
    from vsdeoldify_amd import _native as nat
    base, ov, mask = _clips()
    out = np.empty_like(base)

    def call(dst=out, m=None, **kw):
        f = dict(base_w=66, base_h=34, ov_w=30, ov_h=20, n_frames=3, x=5, y=7, mode=0, plane_mask=7, mask_planes=0, mask_first_plane=1, overlay_frames=3, opacity=1.0)
        f.update(kw)
        p = nat.OverlayParams(**f)
        return ctx.lib.havc_overlay_clip(ctx.h, nat.as_ptr(base), nat.as_ptr(ov), None if m is None else nat.as_ptr(m), nat.as_ptr(dst), C.byref(p))

    assert call() == 0
    _same(out, U.clip_overlay(base, ov, 5, 7), "the plain call")
    for kw in (dict(mode=9), dict(mode=-1), dict(plane_mask=8), dict(mask_planes=1), dict(mask_planes=2), dict(overlay_frames=2), dict(opacity=1.5),
               dict(opacity=float("nan")), dict(base_w=0), dict(ov_h=-1), dict(n_frames=0), dict(x=1 << 30), dict(y=-(1 << 30))):
        assert call(**kw) == nat.HAVC_E_INVALID, kw
    assert call(m=mask) == nat.HAVC_E_INVALID                                                                # a mask with mask_planes 0
    assert call(dst=base) == nat.HAVC_E_INVALID and call(dst=ov) == nat.HAVC_E_INVALID
