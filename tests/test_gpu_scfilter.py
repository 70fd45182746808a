"""-m gpu: havc_scene_ssim / havc_scene_hist (csrc/scfilter.hip) against the numpy restatements of tests/scfilter_util.py, and the reference-frame
extraction end to end.

Shapes (height, width): 7 x 7 (one window), 8 x 13, 9 x 70 and 37 x 65 (a ragged tile in each direction), and around the 32-position tile of the SSIM
kernel = frames of 38: 37, 38, 39 in both directions, 37 x 39, and 71 x 37 (three tile rows, the last one a single row of windows).  Contents per shape
(scfilter_util.kernel_clip): random, identical, +-20 perturbed, two constants, a step edge on a tile border, frames far apart.

The SSIM bound 1e-9 is derived, not tuned: the window sums are exact integers on both sides, so the two differ in float64 roundings only -- a handful per
position (1e-16 relative each) and the order of a sum of at most 2^22 terms of magnitude <= 1 (below 1e-12 in the mean); the factor left over is headroom for
fused multiply-adds."""
import os

import numpy as np
import pytest

from tests import scfilter_util as U
from vsdeoldify_amd import havc
from vsdeoldify_amd import scdetect as SD
from vsdeoldify_amd.device import DeviceImage

pytestmark = pytest.mark.gpu

SSIM_BOUND = 1e-9


def test_ssim_equals_numpy_and_is_deterministic(ctx):
    worst = 0.0
    for h, w in U.SHAPES:
        clip, pairs = U.kernel_clip(h, w)
        g = U.gray(clip)
        want = np.array([U.ssim_np(g[a], g[b]) for a, b in pairs])
        got = SD.scene_ssim(ctx, clip, pairs)
        err = np.abs(got - want)
        print(f"ssim {h} x {w}: max |gpu - numpy| = {err.max():.3e}")
        worst = max(worst, float(err.max()))
        assert err.max() <= SSIM_BOUND, (h, w, got, want)
        dclip = DeviceImage.from_numpy(ctx, clip)
        again = SD.scene_ssim(ctx, dclip, pairs)
        assert again.tobytes() == got.tobytes() and SD.scene_ssim(ctx, dclip, pairs).tobytes() == got.tobytes()        # host / device clip, run to run
        assert got[pairs.index((0, 0))] == 1.0 and got[pairs.index((4, 4))] == 1.0 and got[pairs.index((7, 7))] == 1.0
        # repeats, both orders, frames far apart: every pair's value is what a one-pair launch gives, bit for bit
        mixed = [(8, 0), (0, 1), (0, 8), (0, 1), (1, 0), (5, 6), (8, 0), (3, 4)]
        many = SD.scene_ssim(ctx, dclip, mixed)
        for p, v in zip(mixed, many):
            assert SD.scene_ssim(ctx, dclip, [p])[0].tobytes() == v.tobytes(), (h, w, p)
        assert many[1] == many[3] == many[4] and many[0] == many[2] == many[6]                                        # SSIM is symmetric, exactly
        assert np.array_equal(dclip.numpy(), clip)
    print(f"ssim: max |gpu - numpy| over all shapes = {worst:.3e}")


def test_histogram_equals_bincount(ctx):
    for h, w in U.SHAPES + [(130, 257)]:                                           # 130 x 257: several blocks per frame, a ragged last group
        clip, _ = U.kernel_clip(h, w)
        g = U.gray(clip)
        idx = [3, 0, 8, 3, 3, 5, 1, 0, 7]                                          # repeats; frame 3 is one value: every pixel contends for one bin
        want = np.stack([U.hist(g[i]) for i in idx])
        got = SD.scene_hist(ctx, clip, idx)
        assert got.dtype == np.uint32 and np.array_equal(got.astype(np.int64), want), (h, w)
        assert got[0, U.gray(np.array([37, 37, 37], np.uint8))] == h * w and (got.sum(1) == h * w).all()
        dclip = DeviceImage.from_numpy(ctx, clip)
        assert SD.scene_hist(ctx, dclip, idx).tobytes() == got.tobytes()
        assert np.array_equal(SD.scene_hist(ctx, dclip, [6])[0].astype(np.int64), U.hist(g[6]))


def test_kernels_refuse_bad_arguments(ctx):
    clip, _ = U.kernel_clip(8, 13)
    for fn, lst in ((SD.scene_hist, [0, 9]), (SD.scene_hist, [-1]), (SD.scene_ssim, [(0, 9)]), (SD.scene_ssim, [(-1, 0)])):
        with pytest.raises(ValueError, match="outside the clip"):
            fn(ctx, clip, lst)
    small = np.zeros((2, 6, 20, 3), np.uint8)
    with pytest.raises(ValueError, match="7 x 7"):
        SD.scene_ssim(ctx, small, [(0, 1)])
    with pytest.raises(ValueError, match="7 x 7"):
        SD.scene_ssim(ctx, np.zeros((2, 20, 6, 3), np.uint8), [(0, 1)])
    assert SD.scene_hist(ctx, small, [1])[0, 0] == 120                                                                  # the histogram has no such limit
    with pytest.raises(ValueError, match="not empty"):
        SD.scene_ssim(ctx, clip, [])


CASES = [dict(sc_tht_ssim=0.60), dict(sc_tht_ssim=0.60, sc_min_int=3), dict(sc_threshold=0.05, sc_tht_ssim=0.60, sc_min_int=10), dict(sc_min_int=4),
         dict(sc_tht_ssim=1.0, sc_min_int=3)]


def _margins(dbg, ssim_tht):
    """the condition on the inputs: no reference score within 1e-6 of a 4-decimal rounding boundary or of a threshold it is compared with"""
    for t_n, (s, hs) in dbg["raw"].items():
        for v, thresholds in ((s, (ssim_tht, SD.DEF_SSIM_SCORE_EQUAL)), (hs, (SD.DEF_HIST_SCORE_HIGH, SD.DEF_HIST_SCORE_EQUAL))):
            frac = (v * 1e4) % 1.0
            assert abs(frac - 0.5) > 1e-2, (t_n, v)                                # 1e-2 of a unit in the fourth decimal = 1e-6
            assert all(abs(v - t) > 1e-6 for t in thresholds), (t_n, v)


def test_extract_reference_frames_end_to_end(ctx, tmp_path):
    clip = U.filter_clip()
    assert clip.shape == (24, 48, 64, 3)
    dclip = DeviceImage.from_numpy(ctx, clip)
    fallbacks = 0
    for k, kw in enumerate(CASES):
        want, ref = U.detect_filtered_np(clip, threshold=kw.get("sc_threshold", 0.10), sc_tht_filter=kw.get("sc_tht_ssim", 0.0), min_length=kw.get("sc_min_int", 1))
        _margins(ref, kw.get("sc_tht_ssim", 0.0))
        flagged = [i for i in range(24) if i == 0 or want.scene_change_prev[i] == 1]
        for j, c in enumerate((clip, dclip)):
            d, dbg = str(tmp_path / f"case{k}_{j}"), {}
            got = havc.HAVC_extract_reference_frames(c, sc_framedir=d, ref_ext="png" if k % 2 else "jpg", debug=dbg, **kw)
            assert isinstance(got, SD.SceneInfo)
            for f in ("scene_change_prev", "scene_change_next", "sc_luma", "sc_ratio"):
                assert np.array_equal(getattr(got, f), getattr(want, f)), (kw, f)
            assert dbg["candidates"] == sorted(set([0] + ref["stage1"]))
            assert dbg["scores"] == ref["scores"] and dbg["reasons"] == ref["reasons"]                                  # the rounded scores, candidate by candidate
            # one histogram launch and one SSIM launch over all candidates; another pair only behind a rejection
            foreseen = set(zip(dbg["candidates"][1:], dbg["candidates"][:-1]))
            assert dbg["fallback_pairs"] == [p for p in ref["asked"] if p not in foreseen] and dbg["fallback_launches"] == len(dbg["fallback_pairs"])
            if kw.get("sc_tht_ssim") == 1.0:
                assert (dbg["hist_launches"], dbg["ssim_launches"], dbg["fallback_launches"]) == (0, 0, 0)
            else:
                assert (dbg["hist_launches"], dbg["ssim_launches"]) == (1, 1)
            fallbacks += dbg["fallback_launches"]
            # exactly the flagged frames are written, with the bytes of the host writer
            ext = "png" if k % 2 else "jpg"
            assert sorted(os.listdir(d)) == [f"ref_{i:06d}.{ext}" for i in flagged] and dbg["written"] == [os.path.join(d, f) for f in sorted(os.listdir(d))]
            hd = str(tmp_path / f"host{k}_{j}")
            havc.HAVC_export_reference_frames(clip, hd, ref_ext=ext, scenes=want)
            for f in os.listdir(d):
                assert open(os.path.join(d, f), "rb").read() == open(os.path.join(hd, f), "rb").read(), f
        if j == 1:
            assert np.array_equal(dclip.numpy(), clip)
    assert fallbacks > 0, "no rejection forced a one-pair launch"
    # what the clip was built for, with the documented best settings (0.60, 10): frame 1 is flagged by stage 1 (the first difference is measured against the
    # 0.0001 floor) and rejected as similar, the cut into the dark stretch at 14 is skipped inside the interval
    best = havc.HAVC_extract_reference_frames(dclip, sc_tht_ssim=0.60, sc_min_int=10, sc_framedir=str(tmp_path / "best"))
    assert list(np.flatnonzero(best.scene_change_prev)) == [0, 4, 7, 10, 12, 17, 20, 22]
