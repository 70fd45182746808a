"""-m gpu: havc_scene_stats (csrc/scdetect.hip) against the numpy restatement of tests/scdetect_util.py -- exact integer equality -- and HAVC_SceneDetect
against scene_flags of the numpy statistics.  5-frame clips of 1 x 1, 3 x 5, 7 x 9 (pixel count no multiple of four: frames start at odd byte
offsets), 64 x 64 (exactly one block of full groups) and 130 x 257 (five blocks per frame, ragged last block, ragged last group); offsets 1, 2 and 5
(5 on 5 frames: every frame against frame 0); both coefficient sets; normalisation off and on, host and device clips."""
import numpy as np
import pytest

from tests import scdetect_util as U
from vsdeoldify_amd import havc
from vsdeoldify_amd import scdetect as SD
from vsdeoldify_amd.device import DeviceImage

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (3, 5), (7, 9), (64, 64), (130, 257)]                                           # (height, width)
FIELDS = ("sum_y", "sad", "sum_raw", "min_y", "max_y")


def _same(rec, want, what):
    for k in FIELDS:
        assert np.array_equal(rec[k].astype(np.int64), want[k]), (what, k, rec[k], want[k])


def test_scene_stats_equal_numpy(ctx):
    for h, w in SIZES:
        clip = U.noise_clip(h * 1000 + w, 5, h, w)
        dclip = DeviceImage.from_numpy(ctx, clip)
        for coeffs in (SD.LUMA_LIMITED, SD.LUMA_FULL):
            for offset in (1, 2, 5):
                want = U.scene_stats_np(clip, offset, False, coeffs)
                rec = SD.scene_stats(ctx, clip, offset, False, coeffs)
                _same(rec, want, (h, w, coeffs, offset))
                assert np.array_equal(rec["sum_raw"], rec["sum_y"]) and rec["sad"][0] == 0
                drec = SD.scene_stats(ctx, dclip, offset, False, coeffs)
                assert drec.tobytes() == rec.tobytes()                                           # host and device clips: the same bytes
        if h * w > 1:
            assert (want["sad"][1:] > 0).all()
        assert np.array_equal(dclip.numpy(), clip)                                               # the input is left alone
    again = SD.scene_stats(ctx, dclip, 5, False, SD.LUMA_FULL)
    assert again.tobytes() == drec.tobytes()                                                     # bit-identical from run to run


def test_scene_stats_normalised_equal_numpy(ctx):
    for h, w in SIZES:
        clip = U.normalize_clip(h * 77 + w, h, w)
        dclip = DeviceImage.from_numpy(ctx, clip)
        for coeffs in (SD.LUMA_LIMITED, SD.LUMA_FULL):
            raw = U.scene_stats_np(clip, 1, False, coeffs)
            luma = raw["sum_y"] / (h * w) / 255.0
            assert luma[0] < 0.19 and luma[1] > 0.70 and 0.19 < luma[2] < 0.70 and raw["min_y"][2] == raw["max_y"][2]
            for offset in (1, 2, 5):
                want = U.scene_stats_np(clip, offset, True, coeffs)
                rec = SD.scene_stats(ctx, clip, offset, True, coeffs)
                _same(rec, want, (h, w, coeffs, offset))
                assert rec["sum_y"][2] == 0                                                      # the flat frame inside the thresholds: all zeros
                assert rec["sum_y"][0] == rec["sum_raw"][0] and rec["sum_y"][1] == rec["sum_raw"][1]     # outside the thresholds: as they are
                drec = SD.scene_stats(ctx, dclip, offset, True, coeffs)
                assert drec.tobytes() == rec.tobytes()
            if h * w > 16:
                assert rec["sum_y"][3] != rec["sum_raw"][3]                                      # an ordinary frame is stretched
        # other thresholds move frames across the line: nothing inside (0.5, 0.5) -> the plain statistics
        off = SD.scene_stats(ctx, clip, 1, True, SD.LUMA_LIMITED, 0.5, 0.5)
        _same(off, U.scene_stats_np(clip, 1, False, SD.LUMA_LIMITED), (h, w, "no frame inside"))


def test_scene_stats_refuses_bad_arguments(ctx):
    clip = U.noise_clip(1, 2, 4, 4)
    for kw in (dict(offset=0), dict(offset=26), dict(coeffs=(40000, 40000, 40000, 0)), dict(coeffs=(-1, 2, 3, 4)),
               dict(normalize=True, tht_black=0.8, tht_white=0.2)):
        with pytest.raises(ValueError, match="scene_stats"):
            SD.scene_stats(ctx, clip, **kw)


def test_scene_detect_equals_scene_flags_of_the_numpy_statistics(ctx):
    clip = U.detect_clip()
    assert clip.shape == (24, 96, 160, 3)
    dclip = DeviceImage.from_numpy(ctx, clip)
    npix = 96 * 160
    # custom path (threshold < 0.10), offsets 1 and 2, with and without normalisation; default (plugin) path
    cases = [dict(sc_threshold=0.05), dict(sc_threshold=0.05, sc_tht_offset=2), dict(sc_threshold=0.08, sc_normalize=True, sc_min_freq=10),
             dict(), dict(sc_min_freq=7), dict(sc_normalize=True, luma_range="full")]
    for kw in cases:
        coeffs = SD.LUMA_FULL if kw.get("luma_range") == "full" else SD.LUMA_LIMITED
        thr, off, freq = kw.get("sc_threshold", 0.10), kw.get("sc_tht_offset", 1), kw.get("sc_min_freq", 0)
        st = U.scene_stats_np(clip, off, kw.get("sc_normalize", False), coeffs)
        want = SD.scene_flags(st["sum_y"], st["sad"], npix, thr, freq, off, 1, 0.70, 0.10)
        for c in (clip, dclip):
            got = havc.HAVC_SceneDetect(c, **kw)
            assert isinstance(got, SD.SceneInfo) and (got.sc_threshold, got.sc_frequency) == (thr, freq)
            for f in ("scene_change_prev", "scene_change_next", "sc_luma", "sc_ratio"):
                assert np.array_equal(getattr(got, f), getattr(want, f)), (kw, f)
    # the constructed clip does what it was built for.  Default path: the three cuts; the cut into the black stretch (frame 8) falls to the luma filter and the
    # fade stays below the threshold.  Custom path: the reference lets no cut through for DEF_SC_MIN_DISTANCE = 15 frames after frame 0 and then compares with
    # frame 0's floor difference (0.0001), so frame 15 is its first scene change -- its behaviour, restated, not a property of the clip.
    assert list(np.flatnonzero(havc.HAVC_SceneDetect(clip).scene_change_prev)) == [0, 5, 11, 19]
    assert list(np.flatnonzero(havc.HAVC_SceneDetect(clip, sc_threshold=0.05).scene_change_prev)) == [0, 15]
    # early returns touch no pixel; one frame in
    assert not havc.HAVC_SceneDetect(dclip, sc_threshold=0, sc_min_freq=0).scene_change_prev.any()
    assert list(np.flatnonzero(havc.HAVC_SceneDetect(dclip, sc_threshold=0, sc_min_freq=10).scene_change_prev)) == [0, 10, 20]
    one = havc.HAVC_SceneDetect(clip[3], sc_threshold=0.05)
    assert list(one.scene_change_prev) == [1] and one.sc_luma.shape == (1,)


def test_scene_detect_resamples_a_large_clip_first(ctx):
    """a clip taller than 480 lines: resize_min_HW's size, the library's Spline64 on the RGB clip, then the statistics -- host and device clips"""
    r = np.random.default_rng(5)
    n, h, w = 4, 600, 800
    yy, xx = np.mgrid[0:h, 0:w]
    base = [100 + 60 * np.sin(xx / 37.0 + yy / 23.0), 140 + 50 * np.cos(xx / 19.0 - yy / 41.0)]
    clip = np.stack([np.clip(base[i // 2][..., None] + r.integers(-20, 21, (h, w, 3)), 0, 255) for i in range(n)]).astype(np.uint8)      # a cut at frame 2
    assert SD.resize_min_hw(w, h) == (640, 480)
    dclip = DeviceImage.from_numpy(ctx, clip)
    small = havc.spline64(ctx, clip, 640, 480)
    assert small.shape == (n, 480, 640, 3) and np.array_equal(havc.spline64(ctx, dclip, 640, 480).numpy(), small)
    for kw in (dict(), dict(sc_threshold=0.05, sc_tht_offset=2, sc_normalize=True)):
        st = U.scene_stats_np(small, kw.get("sc_tht_offset", 1), kw.get("sc_normalize", False))
        want = SD.scene_flags(st["sum_y"], st["sad"], 640 * 480, kw.get("sc_threshold", 0.10), 0, kw.get("sc_tht_offset", 1), 1, 0.70, 0.10)
        for c in (clip, dclip):
            got = havc.HAVC_SceneDetect(c, **kw)
            for f in ("scene_change_prev", "scene_change_next", "sc_luma", "sc_ratio"):
                assert np.array_equal(getattr(got, f), getattr(want, f)), (kw, f)
    assert list(havc.HAVC_SceneDetect(dclip).scene_change_prev) == [1, 0, 1, 0]
    assert np.array_equal(dclip.numpy(), clip)
