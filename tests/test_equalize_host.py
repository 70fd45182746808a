"""CPU (-m "not gpu"): the restated selector logic of HAVC_bw_tune / HAVC_auto_levels (vsdeoldify_amd/equalize.py, tests/equalize_util.py) against the
reference EXECUTED by tools/gen_golden_equalize.py (tests/golden/equalize.npz), the gate / blend-weight / gain arithmetic of the library's host entry
against the same Python, the Levels / range / Merge tables, the signatures, the refusals before any GPU context exists, and the struct layout."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from tests import equalize_util as U
from tests.conftest import ROOT
from vsdeoldify_amd import _native as nat
from vsdeoldify_amd import equalize as EQ
from vsdeoldify_amd import havc

HEADER = os.path.join(ROOT, "include", "havc_mi355.h")


def test_selectors_equal_the_executed_reference():
    g = U.fixture()
    assert "executing the reference" in str(g["provenance"])
    seen = dict(gated=0, blended=0, plain=0, clamped=0)
    for kind, selector in (("yuv", U.selector_yuv), ("rgb", U.selector_rgb)):
        n = int(g[f"n_{kind}"])
        assert n >= 40
        for i in range(n):
            p = U.params(g, f"{kind}_{i}_params")
            img, eq, want = g[f"{kind}_{i}_in"], g[f"{kind}_{i}_eq"], g[f"{kind}_{i}_out"]
            assert img.shape[0] <= 24 and img.shape[1] <= 40
            planes = [eq[:, :, k] for k in range(eq.shape[2])]
            got = selector(img, lambda _plane: planes.pop(0), p["range_tv"], p["blend"])
            assert np.array_equal(got, want), (kind, i, p)
            assert p["used"] == eq.shape[2] - len(planes)                    # the reference asked cv2 for as many planes as the restatement
            luma = EQ.f_luma(int(U.cvcolor.rgb2yuv_u8(img)[:, :, 0].sum(dtype=np.int64)), img.shape[0] * img.shape[1], p["range_tv"])
            if not EQ.luma_gate(luma):
                seen["gated"] += 1
                assert np.array_equal(want, img)
            elif p["blend"] and luma < 0.40:
                seen["blended"] += 1
            else:
                seen["plain"] += 1
            if kind == "yuv" and p["range_tv"] and EQ.luma_gate(luma) and (eq.min() < 16 or eq.max() > 235):
                seen["clamped"] += 1
    assert min(seen.values()) >= 4, seen


def test_gains_equal_the_executed_reference():
    g = U.fixture()
    npix = int(g["gain_npix"])
    for i in range(int(g["n_gain"])):
        sums, fact, want = g[f"gain_{i}_sums"], g[f"gain_{i}_factor"], g[f"gain_{i}_out"]
        avg = [EQ.plane_average(s, npix) for s in sums]
        got = EQ.balance_gains(avg[0], avg[1], avg[2], list(fact))
        assert list(got) == list(want), (i, got, want)
        lib = EQ.frame_params(0, npix, True, sums, fact)["gains"]             # the library's float64 sequence, as the float32 std.Expr makes of it
        assert [np.float32(v) for v in want] == list(lib), (i, lib, want)


def _on_threshold(target, range_tv):
    """the value f_luma takes when the rounded mean sits on a threshold: the threshold itself, or with range_tv what float64 makes of (t + 0.07) - 0.07"""
    return round(target + 0.07, 6) - 0.07 if range_tv else target


def _sums_on_thresholds(npix, range_tv):
    """sum_y values whose f_luma lands on 0.15, 0.40 and 0.70 after rounding, and their neighbours: four per threshold (below, first, last, above)"""
    out = []
    for target in (0.15, 0.40, 0.70):
        centre = int(round((target + (0.07 if range_tv else 0.0)) * (235 if range_tv else 255) * npix))
        hits = [s for s in range(centre - 800, centre + 801) if EQ.f_luma(s, npix, range_tv) == _on_threshold(target, range_tv)]
        assert hits and hits[0] > centre - 800 and hits[-1] < centre + 800, (target, range_tv)
        out += [hits[0] - 1, hits[0], hits[-1], hits[-1] + 1]
    return out


def test_gate_and_blend_weights_over_a_sweep_of_sum_y():
    npix = 1920 * 1080
    for range_tv in (False, True):
        on = _sums_on_thresholds(npix, range_tv)
        sums = list(range(0, 255 * npix, 255 * npix // 997)) + [255 * npix] + on
        exact = {_on_threshold(t, range_tv): 0 for t in (0.15, 0.40, 0.70)}
        for s in sums:
            luma = EQ.f_luma(s, npix, range_tv)
            lib = EQ.frame_params(s, npix, range_tv)
            assert lib["f_luma"] == float(luma), (s, range_tv)
            assert lib["gate"] == EQ.luma_gate(luma) == (0.15 <= luma <= 0.70)
            for key, consts in (("w_yuv", EQ.BLEND_YUV), ("w_rgb", EQ.BLEND_RGB)):
                w = EQ.blend_weight(luma, *consts)
                assert (lib[key] is None) == (w is None) == (not luma < 0.40)
                if w is not None:
                    assert lib[key] == np.float32(w), (s, key)                  # Image.blend takes a C float
                    assert consts[2] <= w <= 0.9 and w == round(w, 6)
            if luma in exact:
                exact[luma] += 1
        assert all(v >= 2 for v in exact.values()), exact
        gates = [EQ.frame_params(s, npix, range_tv)["gate"] for s in on]
        blends = [EQ.frame_params(s, npix, range_tv)["w_yuv"] is not None for s in on]
        if not range_tv:
            # on 0.15 and on 0.70: inside (<=); one step outside: not.  On 0.40: no blend any more (<)
            assert gates == [False, True, True, True, True, True, True, True, True, True, True, False]
            assert blends[4:8] == [True, False, False, False]
        else:
            # (t + 0.07) - 0.07 in float64: 0.22 - 0.07 == 0.15 and 0.77 - 0.07 == 0.70 (inside), but 0.47 - 0.07 is one ulp BELOW 0.40: still blended
            assert 0.22 - 0.07 == 0.15 and 0.47 - 0.07 < 0.40 and 0.77 - 0.07 == 0.70
            assert gates == [False, True, True, True, True, True, True, True, True, True, True, False]
            assert blends[4:8] == [True, True, True, False]
    assert EQ.blend_weight(0.15, *EQ.BLEND_YUV) == 0.35 and EQ.blend_weight(0.15, *EQ.BLEND_RGB) == 0.15   # the floors
    assert EQ.blend_weight(0.399999, *EQ.BLEND_YUV) == round(0.9 * (0.399999 / 0.4) ** 2.0, 6)


def test_levels_range_and_merge_tables_match_their_closed_forms():
    def levels(v, a, b, c, d):
        return int(min(max((v - a) / (b - a), 0), 1) * (d - c) + c + 0.5)
    down, up = EQ.levels_table(0, 255, 16, 235), EQ.levels_table(16, 235, 0, 255)
    assert [int(down[v]) for v in (0, 16, 235, 255)] == [16, 30, 218, 235] == [levels(v, 0, 255, 16, 235) for v in (0, 16, 235, 255)]
    assert [int(up[v]) for v in (0, 16, 235, 255)] == [0, 0, 255, 255] == [levels(v, 16, 235, 0, 255) for v in (0, 16, 235, 255)]
    lim, full = EQ.range_table(True), EQ.range_table(False)
    assert [int(lim[v]) for v in (0, 16, 235, 255)] == [16, 30, 218, 235] == [int(np.floor(v * 219 / 255 + 16 + 0.5)) for v in (0, 16, 235, 255)]
    assert [int(full[v]) for v in (0, 16, 235, 255)] == [0, 0, 255, 255]
    assert all(int(full[v]) == min(max(int(np.floor((v - 16) * 255 / 219 + 0.5)), 0), 255) for v in range(256))
    assert all(int(lim[v]) == int(np.floor(v * 219 / 255 + 16 + 0.5)) for v in range(256))
    # the reference applies Levels AND the range conversion, each way: composed, 0..255 is squeezed twice on the way in
    tin, tout = EQ.tv_in_table(), EQ.tv_out_table()
    assert [int(tin[v]) for v in (0, 16, 235, 255)] == [int(lim[down[v]]) for v in (0, 16, 235, 255)] == [30, 42, 203, 218]
    assert [int(tout[v]) for v in (0, 16, 235, 255)] == [int(full[up[v]]) for v in (0, 16, 235, 255)] == [0, 0, 255, 255]
    assert np.all(np.diff(tin.astype(int)) >= 0) and np.all(np.diff(tout.astype(int)) >= 0)
    # std.Merge: w = 0 -> a, w = 1 -> b, exactly; in between the closed form
    a, b = np.array([0, 16, 235, 255, 255, 0], np.uint8), np.array([255, 235, 16, 0, 255, 0], np.uint8)
    assert np.array_equal(EQ.merge15(a, b, 0.0), a) and np.array_equal(EQ.merge15(a, b, 1.0), b)
    for w in (0.02, 0.3, 0.5, 0.7):
        want = [int(x) + (((int(y) - int(x)) * int(w * 32768 + 0.5) + 16384) >> 15) for x, y in zip(a, b)]
        assert EQ.merge15(a, b, w).tolist() == want
    assert EQ.w15(0.02) == 655 and EQ.w15(0.7) == 22938 and EQ.w15(1.0) == 32768
    assert EQ.expr_mul(np.array([0, 16, 235, 255], np.uint8), 1.03).tolist() == [0, 16, 242, 255]
    assert EQ.expr_mul(np.array([2, 6, 10], np.uint8), 0.25).tolist() == [0, 2, 2]            # halves go to even


def test_opencv_restatements_on_hand_made_planes():
    # a constant plane keeps its value; two levels spread to 0 and 255; the first occupied bin maps to 0
    assert np.array_equal(U.equalize_hist(np.full((8, 8), 77, np.uint8)), np.full((8, 8), 77, np.uint8))
    p = np.array([[10] * 8] * 4 + [[200] * 8] * 4, np.uint8)
    assert np.array_equal(U.equalize_hist(p), np.where(p == 10, 0, 255).astype(np.uint8))
    # CLAHE of a constant 64 x 64 plane: every tile's histogram is one bin of 64, clipped to the limit 1 -> 63 spread as residual (step 4) -> the table of
    # value v is round((1 + #{i <= v: i % 4 == 0 and i // 4 < 63}) * 255 / 64) once v is reached
    stats = []
    out = U.clahe(np.full((64, 64), 100, np.uint8), 1.0, stats)
    assert stats == [(63, 63)] * 64
    assert np.all(out == int(np.rint(np.float32(1 + 26) * (np.float32(255) / np.float32(64)))))
    assert U.tile_size(11, 9) == (2, 2) and U.tile_size(90, 70) == (12, 9) and U.tile_size(64, 64) == (8, 8) and U.tile_size(9, 16) == (2, 3)


def test_signatures_equal_the_reference():
    def pos(fn):
        return [(k, v.default) for k, v in inspect.signature(fn).parameters.items() if v.kind is v.POSITIONAL_OR_KEYWORD]
    assert pos(havc.HAVC_auto_levels) == [("clip", None), ("mode", "Light"), ("method", 0), ("luma_blend", False), ("range_tv", True)]   # __init__.py:3150-3151
    assert pos(havc.HAVC_bw_tune) == [("clip", None), ("bw_tune", "Light"), ("bw_method", 0), ("luma_blend", True), ("range_tv", True),
                                      ("chroma_resize", False)]                                                                    # __init__.py:1266-1267
    assert pos(EQ.rgb_equalizer_np) == [("ctx", inspect.Parameter.empty), ("clip", inspect.Parameter.empty), ("method", 0), ("clip_limit", 1.0),
                                        ("gridsize", 8), ("strength", 0.5), ("weight3", 0.3), ("luma_blend", True), ("range_tv", True)]   # havc_utils.py:836-838
    import vsdeoldify_amd
    assert vsdeoldify_amd.HAVC_auto_levels is havc.HAVC_auto_levels and vsdeoldify_amd.HAVC_bw_tune is havc.HAVC_bw_tune


def test_refusals_come_before_any_gpu_work(monkeypatch):
    def no_gpu(*a, **k):
        raise AssertionError("GPU work was started")
    monkeypatch.setattr(havc, "get_context", no_gpu)
    monkeypatch.setattr(EQ, "rgb_equalizer_np", no_gpu)
    c = np.zeros((2, 16, 16, 3), np.uint8)
    E, R = havc.HAVCError, NotImplementedError
    for fn, key, tune in ((havc.HAVC_auto_levels, "method", "mode"), (havc.HAVC_bw_tune, "bw_method", "bw_tune")):
        with pytest.raises(R, match="timecube"):
            fn(c, **{key: 4})
        with pytest.raises(R, match="Retinex"):
            fn(c, **{key: 5})
        with pytest.raises(E, match="B&W tune choice is invalid:  heavy"):
            fn(c, **{tune: "Heavy"})
        with pytest.raises(E, match="not a clip"):
            fn(None)
        with pytest.raises(E, match="not a clip"):
            fn([[1, 2, 3]])
        with pytest.raises(E, match="smaller than the 8 x 8 tile grid"):
            fn(np.zeros((2, 7, 16, 3), np.uint8))
        with pytest.raises(E, match="smaller than the 8 x 8 tile grid"):
            fn(np.zeros((16, 7, 3), np.uint8))
        with pytest.raises(E, match="RGB24"):
            fn(np.zeros((2, 16, 16, 4), np.uint8))
    with pytest.raises(R, match="Retinex"):
        havc.HAVC_bw_tune(c, bw_method=9)                                      # min(5, bw_method), __init__.py:1301
    with pytest.raises(R, match="chroma_resize"):
        havc.HAVC_bw_tune(c, chroma_resize=True)
    assert havc.HAVC_bw_tune(c, bw_tune="None") is c                           # __init__.py:1312-1313


def test_rgb_equalizer_np_refusals_need_no_context():
    c = np.zeros((2, 16, 16, 3), np.uint8)
    with pytest.raises(havc.HAVCError, match="gridsize"):
        EQ.rgb_equalizer_np(None, c, gridsize=4)
    with pytest.raises(havc.HAVCError, match="8 x 8"):
        EQ.rgb_equalizer_np(None, c[:, :, :7])
    with pytest.raises(havc.HAVCError, match="8 x 8"):
        EQ.rgb_equalizer_np(None, c[:, :5])
    with pytest.raises(NotImplementedError, match="timecube"):
        EQ.rgb_equalizer_np(None, c, method=4)
    with pytest.raises(NotImplementedError, match="Retinex"):
        EQ.rgb_equalizer_np(None, c, method=5)


def test_struct_layout_matches_the_header():
    src = open(HEADER).read()
    m = re.search(r"typedef struct havc_equalize_params \{(.*?)\} havc_equalize_params;", src, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = [re.sub(r"\[\d+\]", "", n).strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == [f[0] for f in nat.EqualizeParams._fields_]
    P = nat.EqualizeParams
    assert ctypes.sizeof(P) == 600 and P.clip_limit.offset == 32 and P.rgb_factor.offset == 64 and P.lut_in.offset == 88 and P.lut_out.offset == 344
    assert "int havc_equalize_clip(havc_ctx* ctx, const uint8_t* src, uint8_t* dst, const havc_equalize_params* params);" in src
    sym = {s[0]: s for s in nat.SYMBOLS}
    assert len(sym["havc_equalize_clip"][2]) == 4 and len(sym["havc_equalize_frame_params"][2]) == 6
