"""-m gpu: havc_equalize_clip (csrc/equalize.hip) against the numpy restatement of tests/equalize_util.py -- exact byte equality: everything is integer or a
stated float32 / float64 sequence -- and HAVC_auto_levels / HAVC_bw_tune against the composed restatement.

Clips of 6 frames (equalize_util.make_clip: below the gate, above it, in the blend zone, at or above 0.40, constant, tinted) at
    8 x 8       tile 1 x 1, clip limit 1: no tile can clip
    16 x 24     tile 2 x 3
    9 x 11      padded to 16 x 16 (reflect-101, 7 padded rows and 5 padded columns)
    70 x 90     ragged tiles: padded to 72 x 96
    64 x 64     tile 8 x 8
    130 x 257   pixel count no multiple of four: frames start at odd byte offsets; padded to 136 x 264, tile 17 x 33 = 561 pixels, more than there are bins
methods 0-3, luma_blend on / off, range_tv on / off, strengths 0.98 / 0.30, clip_limit 1.0 / 2.0: the full product at every size."""
import itertools

import numpy as np
import pytest

from tests import equalize_util as U
from vsdeoldify_amd import equalize as EQ
from vsdeoldify_amd import havc
from vsdeoldify_amd.device import DeviceImage

pytestmark = pytest.mark.gpu

SIZES = [(8, 8), (16, 24), (9, 11), (70, 90), (64, 64), (130, 257)]                              # (height, width)


def _lumas(clip, range_tv):
    y = U.cvcolor.rgb2yuv_u8(clip)[..., 0]
    return [EQ.f_luma(int(f.sum(dtype=np.int64)), f.size, range_tv) for f in y]


def _same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} bytes differ, first at {bad[0].tolist()}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}")


@pytest.mark.parametrize("h,w", SIZES)
def test_equalizer_equals_numpy(ctx, h, w):
    clip = U.make_clip(h, w)
    dclip = DeviceImage.from_numpy(ctx, clip)
    # the frames are what they were built for, with either range
    for range_tv in (False, True):
        lu = _lumas(clip, range_tv)
        assert lu[0] < 0.15 and lu[1] > 0.70 and 0.15 <= lu[2] < 0.40 and 0.40 <= lu[3] <= 0.70 and 0.15 <= lu[4] <= 0.70 and 0.15 <= lu[5] <= 0.70
    assert (clip[4] == clip[4][0, 0]).all()
    stats = {}
    for method, blend, range_tv, strength, limit in itertools.product(range(4), (True, False), (True, False), (0.98, 0.30), (1.0, 2.0)):
        what = (h, w, method, blend, range_tv, strength, limit)
        want = U.rgb_equalizer(clip, method, limit, strength, 0.3, blend, range_tv, stats=stats.setdefault(limit, {}))
        got = EQ.rgb_equalizer_np(ctx, clip, method, limit, 8, strength, 0.3, blend, range_tv)
        assert got.shape == clip.shape and got.dtype == np.uint8
        _same(got, want, what)
        assert np.array_equal(want[0], clip[0]) and np.array_equal(want[1], clip[1])            # gated frames: bit-identical to the input
        assert not np.array_equal(want[3], clip[3])                                              # an ordinary frame is changed
        if method == 1:
            assert np.array_equal(want[4], clip[4])                                              # a constant frame: total == hist[i0], the plane keeps its value
    # what the restatement saw on the way: a clipped tile with a residual, a tile that clips nothing, a channel whose first occupied bin is not 0
    tiles = [t for s in stats.values() for t in s["clahe"]]
    if (h, w) == (8, 8):
        assert all(c == 0 for c, _ in tiles)                                                     # one pixel per tile, clip limit 1
    else:
        assert any(c > 0 and r > 0 for c, r in tiles) and any(c == 0 for c, _ in tiles)
    assert any(i0 > 0 for s in stats.values() for i0 in s["hist"])
    # device clip: the same bytes, the input untouched, a second run bit-identical
    for method in range(4):
        want = EQ.rgb_equalizer_np(ctx, clip, method, 2.0, 8, 0.98, 0.3, True, True)
        dout = EQ.rgb_equalizer_np(ctx, dclip, method, 2.0, 8, 0.98, 0.3, True, True)
        assert isinstance(dout, DeviceImage) and dout.shape == clip.shape
        first = dout.numpy()
        _same(first, want, ("device", h, w, method))
        assert np.array_equal(EQ.rgb_equalizer_np(ctx, dclip, method, 2.0, 8, 0.98, 0.3, True, True).numpy(), first)
    assert np.array_equal(dclip.numpy(), clip)


def test_balance_and_tables_equal_numpy(ctx):
    """rgb_balance in front and the in / out tables, as HAVC_bw_tune composes them, on the two sizes with padding"""
    for h, w in ((9, 11), (130, 257)):
        clip = U.make_clip(h, w)
        for method, (bal_s, fact) in itertools.product(range(4), ((0.30, [0.96, 1.03, 1.0]), (0.50, [0.92, 1.08, 1.0]), (1.0, [1.3, 0.7, 1.1]))):
            want = EQ.tv_out_table()[U.rgb_equalizer(U.rgb_balance(EQ.tv_in_table()[clip], bal_s, fact), method, 1.0, 0.4, 0.4, True, True)]
            got = EQ.rgb_equalizer_np(ctx, clip, method, 1.0, 8, 0.4, 0.4, True, True, balance=(bal_s, fact), lut_in=EQ.tv_in_table(),
                                      lut_out=EQ.tv_out_table())
            _same(got, want, (h, w, method, bal_s))


def test_public_functions_equal_the_composed_restatement(ctx):
    clip = U.make_clip(70, 90)
    dclip = DeviceImage.from_numpy(ctx, clip)
    for tune, method, range_tv in itertools.product(("Light", "Strong"), range(4), (True, False)):
        want = U.auto_levels(clip, tune, method, False, range_tv)
        _same(havc.HAVC_auto_levels(clip, tune, method, False, range_tv), want, ("auto_levels", tune, method, range_tv))
        want = U.bw_tune(clip, tune, method, True, range_tv)
        _same(havc.HAVC_bw_tune(clip, tune, method, True, range_tv), want, ("bw_tune", tune, method, range_tv))
    out = havc.HAVC_bw_tune(dclip)                                                               # the defaults of every HAVC_main preset, on a device clip
    assert isinstance(out, DeviceImage)
    _same(out.numpy(), U.bw_tune(clip), "bw_tune defaults, device clip")
    out = havc.HAVC_auto_levels(dclip, "Medium", luma_blend=True)
    _same(out.numpy(), U.auto_levels(clip, "Medium", 0, True, True), "auto_levels Medium, device clip")
    _same(havc.HAVC_auto_levels(clip, "None"), EQ.tv_out_table()[EQ.tv_in_table()[clip]], "auto_levels None: the range round trip alone")
    assert np.array_equal(dclip.numpy(), clip)


def test_single_frame_in_single_frame_out(ctx):
    clip = U.make_clip(70, 90)
    frame = clip[3]
    want = U.bw_tune(clip[3:4])[0]
    got = havc.HAVC_bw_tune(frame)
    assert got.shape == frame.shape
    _same(got, want, "frame")
    dgot = havc.HAVC_bw_tune(DeviceImage.from_numpy(ctx, frame))
    assert isinstance(dgot, DeviceImage) and dgot.shape == frame.shape
    _same(dgot.numpy(), want, "device frame")
    got = EQ.rgb_equalizer_np(ctx, frame, 2, 2.0, 8, 0.98, 0.3, True, False)
    _same(got, U.rgb_equalizer(clip[3:4], 2, 2.0, 0.98, 0.3, True, False)[0], "rgb_equalizer_np frame")
