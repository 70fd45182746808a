"""CPU (-m "not gpu"): scene detection (vsslib/vsscdect.py; vsdeoldify_amd/scdetect.py, csrc/scdetect.hip) -- scene_flags against the executed reference's
selectors (tests/golden/scdetect.npz, tools/gen_golden_scdetect.py), SceneDetect's branch choice, the normalisation arithmetic over every (k, d) pair
against numpy's float64 expression (the Python form AND the library's own host-compiled form, the function the kernel calls), resize_min_HW's sizes, the C
struct layouts, and HAVC_SceneDetect's refusals before any GPU context exists."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import scdetect_util as U
from tests.conftest import ROOT
from vsdeoldify_amd import _native as nat
from vsdeoldify_amd import havc
from vsdeoldify_amd import scdetect as SD

HEADER = os.path.join(ROOT, "include", "havc_mi355.h")


def test_custom_detector_equals_the_executed_reference():
    g = U.fixture()
    assert "executing the reference" in str(g["provenance"])
    n_cases = int(g["n_custom"])
    assert n_cases >= 6
    seen_ratio_rf = seen_ratio_vhi = seen_freq = seen_inside_min = False
    for i in range(n_cases):
        p = U.params(g, f"custom_{i}_params")
        sum_y, sad = g[f"custom_{i}_sum_y"], g[f"custom_{i}_sad"]
        assert 40 <= len(sum_y) <= 60
        prev, nxt, luma, ratio = SD.custom_detector(sum_y, sad, 256, p["threshold"], p["frequency"], p["min_length"], p["tht_white"], p["tht_black"])
        assert np.array_equal(prev, g[f"custom_{i}_prev"]) and np.array_equal(nxt, g[f"custom_{i}_next"]), i
        assert np.array_equal(luma, g[f"custom_{i}_luma"]) and np.array_equal(ratio, g[f"custom_{i}_ratio"]), i      # exact: the same roundings
        if p["min_length"] == SD.DEF_SC_MIN_DISTANCE:          # what SceneDetect passes: the whole function gives the same answer
            info = SD.scene_flags(sum_y, sad, 256, p["threshold"], p["frequency"], p["offset"], 1, p["tht_white"], p["tht_black"],
                                  sc_tht_filter=0.0 if (p["threshold"] < 0.10 or p["offset"] > 1) else 1.0)
            assert np.array_equal(info.scene_change_prev, prev) and np.array_equal(info.scene_change_next, nxt)
            assert np.array_equal(info.sc_luma, luma) and np.array_equal(info.sc_ratio, ratio)
            assert info.sc_threshold == p["threshold"] and info.sc_frequency == p["frequency"]
        seen_ratio_rf |= bool(((ratio > 2.0) & (ratio <= 15.0)).any())
        seen_ratio_vhi |= bool((ratio > 15.0).any())
        seen_freq |= p["frequency"] > 1
        cuts = np.flatnonzero(prev)
        seen_inside_min |= bool(((ratio > 15.0) & (prev == 0)).any()) or bool((np.diff(cuts) < 15).any())
    assert seen_ratio_rf and seen_ratio_vhi and seen_freq and seen_inside_min
    # two more branches the sequences were built for, so that a regenerated fixture cannot lose them unnoticed
    p, prev, ratio, luma = U.params(g, "custom_1_params"), g["custom_1_prev"], g["custom_1_ratio"], g["custom_1_luma"]
    sad = g["custom_1_sad"]
    last = [max(j for j in range(i) if prev[j]) if i else 0 for i in range(len(prev))]
    only_ref_luma = [i for i in np.flatnonzero(prev)[1:] if sad[i] / (256 * 255) <= p["threshold"] and ratio[i] <= 2.0 and luma[last[i]] < 0.19 <= luma[i] <= 0.70]
    assert only_ref_luma, "no frame is flagged by the _sc_ref_luma override alone (dark reference, bright frame, quiet difference)"
    p, prev, ratio, luma = U.params(g, "custom_5_params"), g["custom_5_prev"], g["custom_5_ratio"], g["custom_5_luma"]
    rejected = [i for i in range(len(prev)) if ratio[i] > 15.0 and i - last_ref(prev, i) >= 15 and not prev[i] and not (p["tht_black"] < luma[i] < p["tht_white"])]
    assert rejected, "no candidate (ratio beyond 15, outside min_length) is rejected by the black / white thresholds"


def last_ref(prev, i):
    return max(j for j in range(i) if prev[j])


def test_black_white_filter_equals_the_executed_reference():
    g = U.fixture()
    n_cases = int(g["n_bw"])
    assert n_cases >= 2
    for i in range(n_cases):
        p = U.params(g, f"bw_{i}_params")
        sum_y, sad = g[f"bw_{i}_sum_y"], g[f"bw_{i}_sad"]
        pp, pn = SD.plugin_flags(sad, 256, p["threshold"])
        assert np.array_equal(pp, g[f"bw_{i}_plugin_prev"]) and np.array_equal(pn, g[f"bw_{i}_plugin_next"])   # the stand-in both sides used
        assert pp[0] == 1 and pn[-1] == 1
        prev, nxt, luma = SD.filter_black_white(pp, pn, sum_y, 256, p["frequency"], p["tht_white"], p["tht_black"])
        assert np.array_equal(prev, g[f"bw_{i}_prev"]) and np.array_equal(nxt, g[f"bw_{i}_next"]) and np.array_equal(luma, g[f"bw_{i}_luma"]), i
        info = SD.scene_flags(sum_y, sad, 256, p["threshold"], p["frequency"], 1, 1, p["tht_white"], p["tht_black"])
        assert np.array_equal(info.scene_change_prev, prev) and np.array_equal(info.scene_change_next, nxt) and np.array_equal(info.sc_luma, luma)
        assert np.array_equal(info.sc_ratio, g[f"bw_{i}_ratio"]) and not info.sc_ratio.any()
        # a cut followed by a cut (next = 1) and cuts on black / white frames are dropped
        assert (pp.sum() > prev.sum()) and prev[0] == 1
    assert {U.params(g, f"bw_{i}_params")["frequency"] for i in range(n_cases)} == {0, 25}


def test_branch_choice_and_early_returns():
    assert SD.detect_branch(0, 0) == "none"
    assert SD.detect_branch(0.10, 1) == SD.detect_branch(0, 1) == SD.detect_branch(0, 25) == SD.detect_branch(0.05, 1, 0.5, 7, 9) == "frequency"
    assert SD.detect_branch(0.10, 0) == SD.detect_branch(0.10, 25) == SD.detect_branch(0.5, 0, 0.0, 1, 1) == "plugin"
    assert SD.detect_branch(0.10, 0, tht_offset=0) == SD.detect_branch(0.10, 0, tht_offset=-3) == "plugin"            # clamped to 1
    assert SD.detect_branch(0.0999, 0) == SD.detect_branch(0.10, 0, tht_offset=2) == SD.detect_branch(0.10, 0, tht_offset=99) == "custom"
    assert SD.detect_branch(0.10, 0, sc_tht_filter=1.0) == SD.detect_branch(0.2, 25, sc_tht_filter=1.5) == "custom"
    assert SD.detect_branch(0.10, 0, min_length=0) == "plugin"                                                          # clamped to 1
    for kw in (dict(sc_tht_filter=0.5), dict(min_length=2), dict(sc_tht_filter=0.999, min_length=25), dict(sc_tht_filter=1.0, min_length=2)):
        with pytest.raises(NotImplementedError, match="structural_similarity.*cv2"):
            SD.detect_branch(0.10, 0, **kw)
    z = np.zeros(30, np.int64)
    info = SD.scene_flags(z, z, 4, 0, 0)
    assert not info.scene_change_prev.any() and not info.scene_change_next.any() and (info.sc_luma == 0.5).all() and not info.sc_ratio.any()
    assert (info.sc_threshold, info.sc_frequency) == (0, 0)
    assert SD.scene_flags(z, z, 4, 0.10, 1).scene_change_prev.all()
    info = SD.scene_flags(z, z, 4, 0, 25)
    assert list(np.flatnonzero(info.scene_change_prev)) == [0, 25] and not info.scene_change_next.any()


def test_normalisation_arithmetic_over_every_pair():
    lib = nat.load()
    for d in range(1, 256):
        k = np.arange(0, d + 1, dtype=np.uint8)
        want = np.multiply(255, (k - np.uint8(0)) / (np.uint8(d) - np.uint8(0))).clip(0, 255).astype('uint8')          # vsutils.py:314-316 with min = 0
        assert [SD.norm_value(int(x), d) for x in k] == list(want), d
        assert [lib.havc_scene_norm_value(int(x), d) for x in k] == list(want), d
    assert SD.norm_value(0, 0) == lib.havc_scene_norm_value(0, 0) == 0                                                  # flat frame: defined as 0


def test_restated_normalisation_equals_the_executed_reference():
    g = U.fixture()
    n = int(g["n_norm"])
    changed = 0
    for i in range(n):
        a, want = g[f"norm_{i}_in"], g[f"norm_{i}_out"]
        got = U.frame_normalize(a, SD.DEF_THT_BLACK_MIN, SD.DEF_THT_WHITE_MIN)
        assert np.array_equal(got, want), i
        changed += int(not np.array_equal(a, want))
        mn, mx = int(a.min()), int(a.max())
        if not np.array_equal(a, want):
            assert np.array_equal(np.array([SD.norm_value(int(v) - mn, mx - mn) for v in a.ravel()], np.uint8).reshape(a.shape), want)
    assert 0 < changed < n                                                                                              # both sides of the thresholds
    flat = np.full((4, 4), 120, np.uint8)
    assert not U.frame_normalize(flat, 0.19, 0.70).any()


def test_resize_min_hw_sizes():
    assert SD.resize_min_hw(1920, 1080) == (852, 480)             # round(853.33) = 853 -> odd -> 852
    assert SD.resize_min_hw(854, 480) == (854, 480) and SD.resize_min_hw(640, 360) == (640, 360)     # already small: as it is
    assert SD.resize_min_hw(1080, 1920) == (512, 910)             # portrait: round(910.2) = 910
    assert SD.resize_min_hw(1000, 1333) == (512, 682)             # round(682.5) = 682 (banker's rounding), even
    assert SD.resize_min_hw(900, 1201) == (512, 684)              # round(683.2) = 683 -> odd -> rounded UP for a portrait clip
    assert SD.resize_min_hw(1001, 777) == (618, 480)              # round(618.4) = 618
    assert SD.resize_min_hw(1003, 777) == (620, 480)              # round(619.6) = 620
    assert SD.resize_min_hw(600, 600) == (512, 512)               # square goes the portrait way
    assert SD.resize_min_hw(512, 512) == (512, 512) and SD.resize_min_hw(481, 481) == (481, 481)
    assert SD.resize_min_hw(3, 5) == (3, 5)
    for w, h in ((1920, 1080), (1279, 719), (719, 1279), (4096, 2160)):
        tw, th = SD.resize_min_hw(w, h)
        assert tw % 2 == 0 and th % 2 == 0 and min(tw, th) in (480, 512)


def test_struct_layouts_match_the_header():
    src = open(HEADER).read()
    m = re.search(r"typedef struct havc_scene_params \{(.*?)\} havc_scene_params;", src, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == [f[0] for f in nat.SceneParams._fields_]
    assert ctypes.sizeof(nat.SceneParams) == 56 and nat.SceneParams.tht_black.offset == 40
    m = re.search(r"typedef struct havc_scene_rec \{(.*?)\} havc_scene_rec;", src, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == list(nat.SCENE_REC_DTYPE.names)
    assert nat.SCENE_REC_DTYPE.itemsize == 32 and [nat.SCENE_REC_DTYPE.fields[n][1] for n in names] == [0, 8, 16, 24, 28]
    assert "int havc_scene_stats(havc_ctx* ctx, const uint8_t* clip, const havc_scene_params* params, havc_scene_rec* out);" in src
    sym = {s[0]: s for s in nat.SYMBOLS}
    assert len(sym["havc_scene_stats"][2]) == 4 and len(sym["havc_scene_norm_value"][2]) == 2
    # the coefficient sets: limited range sums to round(219 / 255 * 65536), full range to 65536; neither can leave 0..255
    assert sum(SD.LUMA_LIMITED[:3]) == 56284 == round(219 / 255 * 65536) and sum(SD.LUMA_FULL[:3]) == 65536
    for c in (SD.LUMA_LIMITED, SD.LUMA_FULL):
        assert (sum(c[:3]) * 255 + c[3]) >> 16 <= 255
    assert (SD.LUMA_LIMITED[3] >> 16, (sum(SD.LUMA_LIMITED[:3]) * 255 + SD.LUMA_LIMITED[3]) >> 16) == (16, 235)


def test_scene_detect_refusals_come_before_any_gpu_work(monkeypatch):
    def no_gpu(*a, **k):
        raise AssertionError("a GPU context was asked for")
    monkeypatch.setattr(havc, "get_context", no_gpu)
    clip = np.zeros((3, 8, 8, 3), np.uint8)
    with pytest.raises(havc.HAVCError, match="not a clip"):
        havc.HAVC_SceneDetect(None)
    with pytest.raises(havc.HAVCError, match="not a clip"):
        havc.HAVC_SceneDetect([[1, 2, 3]])
    with pytest.raises(havc.HAVCError, match="luma_range"):
        havc.HAVC_SceneDetect(clip, luma_range="pc")
    for kw in (dict(sc_tht_ssim=0.6), dict(sc_min_int=5)):
        with pytest.raises(NotImplementedError, match="structural_similarity"):
            havc.HAVC_SceneDetect(clip, **kw)
    # the early returns touch no pixel: no context either
    assert not havc.HAVC_SceneDetect(clip, sc_threshold=0, sc_min_freq=0).scene_change_prev.any()
    assert list(havc.HAVC_SceneDetect(clip, sc_threshold=0, sc_min_freq=2).scene_change_prev) == [1, 0, 1]
    assert havc.HAVC_SceneDetect(clip, sc_min_freq=1).scene_change_prev.all()
    with pytest.raises(havc.HAVCError, match="RGB24"):
        havc.HAVC_SceneDetect(np.zeros((3, 8, 8), np.uint8).reshape(3, 8, 8, 1), sc_threshold=0.05)
    # the reference's argument list and defaults (vsdeoldify/__init__.py:3191-3194)
    import inspect
    sig = inspect.signature(havc.HAVC_SceneDetect)
    assert [(k, v.default) for k, v in sig.parameters.items() if v.kind is v.POSITIONAL_OR_KEYWORD][1:] == [
        ("sc_threshold", 0.10), ("sc_tht_offset", 1), ("sc_tht_ssim", 0.0), ("sc_min_int", 1), ("sc_min_freq", 0), ("sc_normalize", False),
        ("sc_tht_white", 0.70), ("sc_tht_black", 0.10), ("sc_debug", False)]
    # HAVC_colorizer keeps refusing scene detection of its own
    with pytest.raises(NotImplementedError, match="scene detection"):
        havc.HAVC_colorizer(clip, sc_threshold=0.1)
