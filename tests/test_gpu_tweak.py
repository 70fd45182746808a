"""-m gpu: havc_rgb_to_yuv420, havc_yuv420_to_rgb, havc_tweak_clip, havc_adjust_rgb_clip (csrc/tweak.hip) and HAVC_tweak / HAVC_adjust_rgb / HAVC_rgb_denoise
against the numpy definition of tests/tweak_util.py: every comparison is byte-equal.

Sizes, h x w:   2 x 2      every tap is mirrored                  34 x 66    one band, partial tiles
                70 x 130   rows cross the 64-row band, columns cross two tiles
                6 x 258    the skew is longer than the band is tall        258 x 6    five bands of mostly idle lanes
Clips of 1 and 3 frames, different content per frame: seeded noise, the last frame a smooth gradient (tweak_util.make_clip)."""
import functools

import numpy as np
import pytest

from tests import equalize_util as EU
from tests import tweak_util as U
from vsdeoldify_amd import equalize as EQ
from vsdeoldify_amd import havc
from vsdeoldify_amd import tweak as TW
from vsdeoldify_amd.device import DeviceImage

pytestmark = pytest.mark.gpu

SIZES = [(2, 2), (34, 66), (70, 130), (6, 258), (258, 6)]
FRAMES = [1, 3]
TWEAKS = [dict(hue=25.0, sat=1.3), dict(bright=12.0, cont=0.9), dict(gamma=1.4), dict(hue=-70.0, sat=0.6, bright=-0.1, cont=1.25, gamma=0.8)]


def _same(got, want, what):
    bad = np.argwhere(got != want)
    assert got.shape == want.shape and len(bad) == 0, (what, len(bad), bad[0].tolist(), int(got[tuple(bad[0])]), int(want[tuple(bad[0])]))


@functools.lru_cache(maxsize=None)
def _planes(h, w, n):
    return U.rgb_to_yuv420(U.make_clip(h, w, n))


@functools.lru_cache(maxsize=None)
def _random_planes(h, w, n):
    r = np.random.default_rng(7 * h + w + n)
    return (r.integers(0, 256, (n, h, w), dtype=np.uint8), r.integers(0, 256, (n, h // 2, w // 2), dtype=np.uint8),
            r.integers(0, 256, (n, h // 2, w // 2), dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def _back_ref(h, w, n):
    return U.yuv420_to_rgb(*_random_planes(h, w, n))


@pytest.mark.parametrize("n", FRAMES)
@pytest.mark.parametrize("h,w", SIZES)
def test_rgb_to_yuv420_alone(ctx, h, w, n):
    got = TW.rgb_to_yuv420_np(ctx, U.make_clip(h, w, n))
    for name, g, r in zip("yuv", got, _planes(h, w, n)):
        _same(g, r, (name, h, w, n))


@pytest.mark.parametrize("n", FRAMES)
@pytest.mark.parametrize("h,w", SIZES)
def test_yuv420_to_rgb_alone_on_random_planes(ctx, h, w, n):
    _same(TW.yuv420_to_rgb_np(ctx, *_random_planes(h, w, n)), _back_ref(h, w, n), (h, w, n))


@pytest.mark.parametrize("n", FRAMES)
@pytest.mark.parametrize("h,w", SIZES)
def test_tweak_parameter_sets(ctx, h, w, n):
    clip = U.make_clip(h, w, n)
    sets = TWEAKS if n == 3 else TWEAKS[-1:]
    for kw, want in zip(sets, U.tweak_many(clip, sets)):
        _same(havc.HAVC_tweak(clip, **kw), want, (h, w, n, kw))
    assert havc.HAVC_tweak(clip) is clip                                          # neutral: the input itself, as in the reference


def test_grey_in_grey_out_and_sat_zero(ctx):
    h, w = 70, 130
    g = np.random.default_rng(3).integers(0, 256, (2, h, w), dtype=np.uint8)
    grey = np.stack([g, g, g], -1)
    for kw in (dict(hue=40.0, sat=1.8), dict(hue=-180.0, sat=0.25)):
        _same(havc.HAVC_tweak(grey, **kw), grey, kw)
    clip = U.make_clip(h, w, 2)
    out = havc.HAVC_tweak(clip, sat=0)
    y = TW.rgb_to_yuv420_np(ctx, clip)[0]
    for c in range(3):
        _same(out[..., c], y, ("sat 0", c))


def test_constant_planes_keep_their_sum(ctx):
    h, w = 70, 130
    for yv, uv, vv in [(100, 90, 160), (30, 200, 60), (220, 120, 140), (128, 40, 40)]:
        planes = (np.full((h, w), yv, np.uint8), np.full((h // 2, w // 2), uv, np.uint8), np.full((h // 2, w // 2), vv, np.uint8))
        out = TW.yuv420_to_rgb_np(ctx, *planes)
        for c, x in enumerate(U.yuv420_to_rgb_float(*planes)):
            if 1 < x.min() and x.max() < 254:                                     # away from the clamp
                d = abs(float(out[..., c].sum(dtype=np.int64)) - float(x.astype(np.float64).sum()))
                print(f"constant planes {(yv, uv, vv)} channel {c}: |sum out - sum x| = {d:.3f}, bound {(w + h) / 2}")
                assert d < (w + h) / 2, (yv, uv, vv, c, d)


def test_a_frame_of_a_clip_equals_the_frame_alone(ctx):
    clip = U.make_clip(70, 130, 3)
    kw = TWEAKS[-1]
    whole = havc.HAVC_tweak(clip, **kw)
    for k in range(3):
        _same(havc.HAVC_tweak(clip[k], **kw), whole[k], k)
    _same(TW.tweak_np(ctx, clip, TW.tweak_plan(**kw), chunk_frames=2), whole, "chunks of 2")


def test_host_clip_and_device_clip_give_the_same_bytes(ctx):
    clip = U.make_clip(34, 66, 3)
    kw = TWEAKS[0]
    dev = havc.HAVC_tweak(DeviceImage.from_numpy(ctx, clip), **kw)
    assert isinstance(dev, DeviceImage)
    _same(dev.numpy(), havc.HAVC_tweak(clip, **kw), "tweak")
    dev = havc.HAVC_adjust_rgb(DeviceImage.from_numpy(ctx, clip), 0.5, (1.1, 0.9, 1.0), (4, -3, 0), (1.2, 1.0, 0.9))
    assert isinstance(dev, DeviceImage)
    _same(dev.numpy(), havc.HAVC_adjust_rgb(clip, 0.5, (1.1, 0.9, 1.0), (4, -3, 0), (1.2, 1.0, 0.9)), "adjust_rgb")


@pytest.mark.parametrize("strength", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("color_range", [None, "full"])
def test_adjust_rgb(ctx, strength, color_range):
    for h, w in ((33, 47), (70, 130)):
        clip = U.make_clip(h, w, 3).copy()
        clip[1, :, :, 2] = 0                                                      # a blue mean of 0: the small_number branch
        clip[0] = (clip[0] * np.array([0.5, 0.9, 0.7])).astype(np.uint8)
        for kw in (dict(), dict(factor=(1.3, 0.8, 1.05), bias=(16, -32, 5.5), gamma=(1.2, 1.0, 0.8))):
            _same(havc.HAVC_adjust_rgb(clip, strength, color_range=color_range, **kw), U.adjust_rgb(clip, strength, color_range=color_range, **kw),
                  (h, w, strength, color_range, kw))


def test_rgb_denoise(ctx):
    clip = EU.make_clip(40, 72)
    for kw in (dict(), dict(denoise_levels=(0.3, 0.2), rgb_factors=(0.98, 1.02, 1.0))):
        got = havc.HAVC_rgb_denoise(clip, **kw)
        _same(got, U.rgb_denoise(clip, **kw), kw)
        dl, rf = kw.get("denoise_levels", (0.4, 0.3)), kw.get("rgb_factors", (0.95, 1.05, 1.01))
        by_hand = EQ.rgb_equalizer_np(ctx, clip, method=0, strength=dl[1], luma_blend=False, range_tv=True, balance=(dl[0], list(rf)),
                                      lut_in=EQ.tv_in_table(), lut_out=EQ.tv_out_table())
        _same(got, by_hand, ("by hand", kw))
