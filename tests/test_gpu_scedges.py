"""-m gpu: havc_scene_edge_stats (csrc/scedge.hip) against the numpy definition of tests/scedges_util.py, and HAVC_SceneDetectEdges end to end.

Sizes (height x width, scedges_util.SIZES): 1 x 1, 3 x 5 and 7 x 9 are smaller than the halo, so reflection folds more than once; 32 x 64 is exactly one
tile; 33 x 65 one tile plus one pixel in each direction; 130 x 257 several ragged tiles and blocks per frame.  Offsets 1, 2 and 5 on six frames (the clamp
index j on both sides of N - offset), both coefficient sets, sigma 1.2 (r = 4) and 0.6 (r = 2).  Everything is integer or a stated float32 sequence:
every comparison is exact."""
import numpy as np
import pytest

from tests import scedges_util as U
from vsdeoldify_amd import havc
from vsdeoldify_amd import scdetect as SD
from vsdeoldify_amd import scdetect_edge as SE
from vsdeoldify_amd.device import DeviceImage

pytestmark = pytest.mark.gpu

FIELDS = ("sum_y", "sad_prev", "sad_next", "sum_masked")


@pytest.mark.parametrize("h,w", U.SIZES)
def test_edge_stats_equal_numpy(ctx, h, w):
    clip = np.array(U.kernel_clip(h, w))
    dclip = DeviceImage.from_numpy(ctx, clip)
    for sigma in (SE.DEF_CANNY_SIGMA, 0.6):
        assert U.radius(sigma) == (4 if sigma == SE.DEF_CANNY_SIGMA else 2)
        for limited in (True, False):
            for offset in (1, 2, 5):
                want, mask = U.reference_stats(h, w, offset, limited, sigma)
                if h >= 64 and w >= 64:                                    # the cap that keeps the comparison from being about saturated masks only
                    extreme = ((mask == 0) | (mask == 255)).reshape(len(mask), -1).mean(1)
                    assert extreme.max() <= 0.5 and (mask == 0).any() and (mask == 255).any()
                coeffs = SD.LUMA_LIMITED if limited else SD.LUMA_FULL
                rec, tap = SE.edge_stats(ctx, clip, offset, coeffs, sigma, mask_tap=True)
                what = (h, w, sigma, limited, offset)
                bad = np.flatnonzero((tap != mask).reshape(len(mask), -1).any(1))
                assert tap.tobytes() == mask.tobytes(), (what, "frames", bad.tolist(), "first at", np.argwhere(tap != mask)[:4].tolist())
                for k in FIELDS:
                    assert np.array_equal(rec[k], want[k]), (what, k, rec[k], want[k])
                drec, dtap = SE.edge_stats(ctx, dclip, offset, coeffs, sigma, mask_tap=True)          # device clip; second run
                assert drec.tobytes() == rec.tobytes() and dtap.tobytes() == tap.tobytes(), what
                assert SE.edge_stats(ctx, dclip, offset, coeffs, sigma).tobytes() == rec.tobytes(), what  # without the tap
    assert np.array_equal(dclip.numpy(), U.kernel_clip(h, w)) and np.array_equal(clip, U.kernel_clip(h, w))


def test_edge_stats_refuse_bad_arguments(ctx):
    clip = np.array(U.kernel_clip(7, 9))
    for kw in (dict(offset=6), dict(offset=0), dict(offset=26), dict(sigma=0.0), dict(sigma=2.6), dict(coeffs=(40000, 40000, 40000, 0))):
        with pytest.raises(ValueError):
            SE.edge_stats(ctx, clip, **kw)
    with pytest.raises(ValueError, match="smaller than the number of frames"):
        SE.edge_stats(ctx, clip[:3], offset=3)
    assert len(SE.edge_stats(ctx, clip[:3], offset=2)) == 3
    assert SE.edge_stats(ctx, clip, sigma=2.5, offset=5)["sum_y"][0] == U.edge_stats_np(clip, 5, sigma=2.5)[0]["sum_y"][0]      # r = 8 is accepted


CASES = [dict(sc_tht_ssim=0), dict(), dict(sc_tht_ssim=0, sc_min_int=4), dict(sc_min_int=4), dict(sc_min_int=4, sc_tht_ssim=1.0)]


def test_scene_detect_edges_end_to_end(ctx):
    clip = np.array(U.detect_clip())
    assert clip.shape == (24, 96, 160, 3)
    dclip = DeviceImage.from_numpy(ctx, clip)
    rejected = 0
    for kw in CASES:
        ssim_tht = kw.get("sc_tht_ssim", 0.80)
        want, ref = U.detect_edges_np(clip, ssim_threshold=ssim_tht, sc_min_int=kw.get("sc_min_int", 20))
        for t_n, (s, hs) in ref["raw"].items():             # no score within 1e-6 of a 4-decimal rounding boundary or of a threshold it is compared with
            for v, thresholds in ((s, (ssim_tht, SD.DEF_SSIM_SCORE_EQUAL)), (hs, (SD.DEF_HIST_SCORE_HIGH, SD.DEF_HIST_SCORE_EQUAL))):
                assert abs((v * 1e4) % 1.0 - 0.5) > 1e-2 and all(abs(v - t) > 1e-6 for t in thresholds), (t_n, v)
        for c in (clip, dclip):
            got = havc.HAVC_SceneDetectEdges(c, **kw)
            assert isinstance(got, SE.EdgeSceneInfo) and isinstance(got, SD.SceneInfo)
            for f in ("scene_change_prev", "scene_change_next", "sc_luma", "sc_ratio", "sc_reason"):
                assert np.array_equal(getattr(got, f), getattr(want, f)), (kw, f, getattr(got, f), getattr(want, f))
            assert (got.sc_threshold, got.sc_frequency) == (0.035, 0)
            assert got.scene_change_prev[0] == 1 and got.scene_change_prev[8] == 1 and got.scene_change_prev[21] == 1, kw      # the two cuts
        if ssim_tht:
            assert (want.sc_luma == SE.ROUTED_LUMA).all() and not want.sc_reason.any()
            rejected += sum(1 for t_n in ref["reasons"] if t_n and not want.scene_change_prev[t_n])
        else:
            assert want.sc_reason[0] == 4 and want.sc_reason[8] == 3 and want.sc_reason[21] == 3
    assert rejected > 0, "the filter rejected no candidate"
    assert np.array_equal(dclip.numpy(), U.detect_clip())
    # the launches: one for the statistics; with the filter one histogram and one SSIM launch over the candidates, a one-pair launch behind a rejection
    dbg = {}
    SE.scene_detect_edges(ctx, dclip, threshold=0.035, ssim_threshold=0.80, sc_min_int=4, sc_mult_tht=15, tht_black=0.10, debug=dbg)
    assert (dbg["hist_launches"], dbg["ssim_launches"]) == (1, 1) and dbg["candidates"][0] == 0 and len(dbg["candidates"]) > 3
    foreseen = set(zip(dbg["candidates"][1:], dbg["candidates"][:-1]))
    assert dbg["fallback_launches"] == len(dbg["fallback_pairs"]) and not foreseen & set(dbg["fallback_pairs"])
