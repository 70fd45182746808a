"""CPU (-m "not gpu"): HAVC_tweak, HAVC_adjust_rgb, HAVC_rgb_denoise.  What vsdeoldify_amd/tweak.py derives -- coefficients, tables, strings and the order of the
native calls -- against the reference EXECUTED by tools/gen_golden_tweak.py (tests/golden/tweak.npz), case by case; the signatures and every refusal with its
text; the properties of the numpy definition (tests/tweak_util.py) that do not depend on it being right in detail; the composed tables of HAVC_adjust_rgb
against the stage-by-stage definition; and the library's host entry points (the kernels' C++ compiled for the host) against the Python."""
import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest

from tests import tweak_util as U
from vsdeoldify_amd import _native as nat
from vsdeoldify_amd import equalize as EQ
from vsdeoldify_amd import havc
from vsdeoldify_amd import tweak as TW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "tweak.npz")


def _golden(kind):
    g = np.load(GOLDEN)
    assert "executing the reference" in str(g["provenance"])
    return json.loads(str(g[kind]))


def _pos(fn):
    return [(k, v.default) for k, v in inspect.signature(fn).parameters.items() if v.kind is v.POSITIONAL_OR_KEYWORD]


def _kwonly(fn):
    return [(k, v.default) for k, v in inspect.signature(fn).parameters.items() if v.kind is v.KEYWORD_ONLY]


def test_signatures_equal_the_reference():
    assert _pos(havc.HAVC_tweak) == [("clip", None), ("hue", 0), ("sat", 1), ("bright", 0), ("cont", 1), ("gamma", 1)]                     # __init__.py:1377-1378
    assert _kwonly(havc.HAVC_tweak) == [("device_index", 0)]
    assert _pos(havc.HAVC_adjust_rgb) == [("clip", None), ("strength", 0.0), ("factor", (1.0, 1.0, 1.0)), ("bias", (0, 0, 0)),
                                          ("gamma", (1.0, 1.0, 1.0))]                                                                      # :1342-1343
    assert _kwonly(havc.HAVC_adjust_rgb) == [("device_index", 0), ("color_range", None)]
    assert _pos(havc.HAVC_rgb_denoise) == [("clip", None), ("denoise_levels", (0.4, 0.3)), ("rgb_factors", (0.95, 1.05, 1.01))]            # :924-925
    assert _kwonly(havc.HAVC_rgb_denoise) == [("device_index", 0)]
    import vsdeoldify_amd
    for name in ("HAVC_tweak", "HAVC_adjust_rgb", "HAVC_rgb_denoise"):
        assert getattr(vsdeoldify_amd, name) is getattr(havc, name) and name in havc.__doc__
    assert "UNPINNED" in TW.__doc__ and "PINNED" in TW.__doc__ and "refusals inside the other entry points" in TW.__doc__
    assert "stay exactly as they are" in havc.__doc__


def test_refusals_come_before_the_gpu(monkeypatch):
    monkeypatch.setattr(havc, "get_context", lambda *a, **k: pytest.fail("a refusal must not create a context"))
    ok = np.zeros((2, 4, 6, 3), np.uint8)
    for fn in (havc.HAVC_tweak, havc.HAVC_adjust_rgb, havc.HAVC_rgb_denoise):
        for bad in (None, [[1, 2, 3]], "clip"):
            with pytest.raises(havc.HAVCError, match=fn.__name__ + ": this is not a clip"):
                fn(bad)
    for fn, kw in ((havc.HAVC_tweak, dict(sat=0.5)), (havc.HAVC_adjust_rgb, dict()), (havc.HAVC_rgb_denoise, dict())):
        for bad in (np.zeros((4, 6), np.uint8), np.zeros((4, 6, 4), np.uint8), np.zeros((1, 2, 4, 6, 3), np.uint8), np.zeros((4, 6, 3), np.float32),
                    np.zeros((0, 4, 6, 3), np.uint8)):
            with pytest.raises(havc.HAVCError, match="only RGB24 clips"):
                fn(bad, **kw)
    for shape in ((5, 6, 3), (4, 7, 3), (2, 3, 3, 3)):
        with pytest.raises(havc.HAVCError, match="cannot be YUV420P8: width and height must be even"):
            havc.HAVC_tweak(np.zeros(shape, np.uint8), sat=0.5)
    with pytest.raises(havc.HAVCError, match="larger than 4096 x 4096"):
        havc.HAVC_tweak(np.zeros((2, 4098, 3), np.uint8), sat=0.5)
    for g in (0, -1.0, float("nan")):
        with pytest.raises(havc.HAVCError, match="std.Levels needs gamma > 0"):
            havc.HAVC_tweak(ok, gamma=g)
    with pytest.raises(havc.HAVCError, match="color_range must be"):
        havc.HAVC_adjust_rgb(ok, color_range="tv")
    with pytest.raises(havc.HAVCError, match="smaller than the 8 x 8 tile grid"):
        havc.HAVC_rgb_denoise(ok)
    assert havc.HAVC_tweak(ok) is ok                                              # the neutral call needs no GPU either


def test_tweak_plan_reproduces_every_recorded_trace():
    cases = _golden("tweak")
    assert len(cases) >= 20
    for c in cases:
        plan = TW.tweak_plan(**c["args"])
        assert ([] if plan is None else plan["calls"]) == c["calls"], c["args"]
        if plan is not None and plan["exprs"] is not None:                        # the kernel's constants are the numbers inside the strings
            assert [float(plan["exprs"][0].split()[3]), float(plan["exprs"][0].split()[8])] == list(plan["hue_sat"])
    args = [c["args"] for c in cases]
    assert {} in args and dict(bright=0.5) in args and dict(bright=-0.5) in args and dict(bright=-40) in args and dict(cont=0.5) in args
    assert dict(hue=180) in args and dict(hue=-180) in args and dict(sat=0) in args
    neutral = [c for c in cases if not c["calls"]]
    assert len(neutral) == 2                                                      # the bare call and the one that spells the defaults out
    luts = {json.dumps(c["args"], sort_keys=True): next(k[1]["lut"] for k in c["calls"] if k[0] == "std.Lut") for c in cases
            if any(k[0] == "std.Lut" for k in c["calls"])}
    assert luts['{"bright": 0.5}'][0] == 128 and luts['{"bright": -0.5}'][255] == 128 and luts['{"bright": 0.999}'][0] == 255    # scaled by 255 (:792-793)
    assert luts['{"bright": 1.0}'][0] == 1 and luts['{"bright": -1.0}'][1] == 0                                                  # at +-1: not scaled
    assert luts['{"bright": -40}'][:41] == [0] * 41 and luts['{"bright": -40}'][41] == 1 and luts['{"bright": -40}'][42] == 2   # int() truncates towards 0


def test_adjust_plan_reproduces_every_recorded_trace_and_refusal():
    cases = _golden("adjust")
    refused = 0
    for c in cases:
        a = dict(c["args"])
        strength, averages, cr = a.pop("strength"), a.pop("averages", None), a.pop("color_range")
        if "error" in c:
            refused += 1
            with pytest.raises(havc.HAVCError, match="^" + re.escape(c["error"]) + "$"):
                TW.adjust_plan(a.get("factor", (1.0, 1.0, 1.0)), a.get("bias", (0, 0, 0)), a.get("gamma", (1.0, 1.0, 1.0)), cr)
            with pytest.raises(ValueError, match="^" + re.escape(c["error"]) + "$"):                  # through the public function, before any GPU work
                havc.HAVC_adjust_rgb(np.zeros((4, 6, 3), np.uint8), strength, color_range=cr, **a)
            continue
        plan = TW.adjust_plan(a.get("factor", (1.0, 1.0, 1.0)), a.get("bias", (0, 0, 0)), a.get("gamma", (1.0, 1.0, 1.0)), cr)
        assert TW.adjust_calls(strength, plan, averages) == c["calls"], c["args"]
    assert refused == 21
    texts = {c["error"] for c in cases if "error" in c}
    assert any('"limited" but rb' in t for t in texts) and any('"full" but bb' in t for t in texts) and any("bg needs to be >= 0" in t for t in texts)
    # no range prop = limited: the same strings and the same refusals
    by_range = {cr: [c for c in cases if c["args"]["color_range"] == cr and "averages" not in c["args"]] for cr in (None, "limited", "full")}
    assert [c.get("calls") for c in by_range[None]] == [c.get("calls") for c in by_range["limited"]]
    assert [c.get("error") for c in by_range[None]] == [c.get("error") for c in by_range["limited"]]
    assert [c.get("calls") for c in by_range[None]] != [c.get("calls") for c in by_range["full"]]


def test_denoise_calls_and_routing(monkeypatch):
    for c in _golden("denoise"):
        assert TW.denoise_calls(**c["args"]) == c["calls"], c["args"]
        seen = {}
        monkeypatch.setattr(havc, "_equalize_clip", lambda clip, device_index, **kw: seen.update(kw) or clip)
        havc.HAVC_rgb_denoise(np.zeros((8, 8, 3), np.uint8), **c["args"])
        bal, eq = c["calls"][2][1], c["calls"][3][1]
        assert seen == dict(method=eq["method"], strength=eq["strength"], luma_blend=eq["luma_blend"], range_tv=eq["range_tv"], range_tv_tables=True,
                            balance=(bal["strength"], bal["rgb_factor"])), (seen, c["calls"])


def test_definition_grey_stays_grey_and_sat_zero_is_luma():
    g = np.random.default_rng(1).integers(0, 256, (2, 34, 66), dtype=np.uint8)
    grey = np.stack([g, g, g], -1)
    y, u, v = U.rgb_to_yuv420(grey)
    assert (u == 128).all() and (v == 128).all() and np.array_equal(y, g)
    outs = U.tweak_many(grey, [dict(hue=30.0, sat=1.7), dict(hue=-180, sat=0.3), dict(hue=180)])
    assert all(np.array_equal(o, grey) for o in outs)
    clip = U.make_clip(34, 66, 2)
    out, y = U.tweak(clip, sat=0), U.rgb_to_yuv420(clip)[0]
    assert all(np.array_equal(out[..., c], y) for c in range(3))
    assert U.tweak(clip) is clip


def test_definition_error_diffusion_keeps_the_sum_of_constant_planes():
    h, w = 70, 130
    worst = 0.0
    for yv, uv, vv in [(100, 90, 160), (30, 200, 60), (220, 120, 140), (128, 40, 40)]:
        planes = (np.full((h, w), yv, np.uint8), np.full((h // 2, w // 2), uv, np.uint8), np.full((h // 2, w // 2), vv, np.uint8))
        xs = np.stack(U.yuv420_to_rgb_float(*planes))
        keep = [c for c in range(3) if 1 < xs[c].min() and xs[c].max() < 254]
        out = U.dither_fs(xs[keep])
        for c, o in zip(keep, out):
            d = abs(float(o.sum(dtype=np.int64)) - float(xs[c].astype(np.float64).sum()))
            worst = max(worst, d)
            assert d < (w + h) / 2, (yv, uv, vv, c, d)
    print(f"largest |sum out - sum x| = {worst:.3f}, bound {(w + h) / 2}")


def test_definition_mirror_and_weights():
    assert [U.mirror(p, 5) for p in (-3, -2, -1, 0, 4, 5, 6)] == [2, 1, 0, 0, 4, 4, 3]
    assert [U.mirror(p, 1) for p in (-3, -1, 0, 1, 2)] == [0, 0, 0, 0, 0] and [U.mirror(p, 2) for p in (-3, 4)] == [1, 0]
    lib = TW.native_weights()
    want = (U.down_weights(True), U.down_weights(False), np.stack([U.up_weights(True, o)[0] for o in (0, 1)]),
            np.stack([U.up_weights(False, o)[0] for o in (0, 1)]))
    for got, ref in zip(lib, want):
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (got, ref)
        assert abs(float(ref.astype(np.float64).sum(-1).max()) - 1.0) < 1e-6
    assert [U.up_weights(True, 0)[1], U.up_weights(True, 1)[1], U.up_weights(False, 0)[1], U.up_weights(False, 1)[1]] == [-2, -1, -1, -1]


def _all_values_frame(seed):
    """3 frames of 32 x 24 in which every channel holds all 256 values, with different means per channel and frame; frame 1 has no blue at all"""
    r = np.random.default_rng(seed)
    clip = np.empty((3, 32, 24, 3), np.uint8)
    for f in range(3):
        for c in range(3):
            extra = r.integers(0, 40 + 70 * c + 30 * f, 32 * 24 - 256)
            clip[f, :, :, c] = r.permutation(np.concatenate([np.arange(256), extra])).reshape(32, 24)
    clip[1, :, :, 2] = 0
    return clip


@pytest.mark.parametrize("strength", [0.0, 0.3, 1, 1.5])
def test_composed_tables_equal_the_stage_by_stage_definition(strength):
    clip = _all_values_frame(5)
    for cr in (None, "full"):
        for kw in (dict(), dict(factor=(1.3, 0.8, 1.05), bias=(16, -32, 5.5), gamma=(1.2, 1.0, 0.8)), dict(factor=(0.5, 2, 1), gamma=(0, 2.2, 1))):
            plan = TW.adjust_plan(kw.get("factor", (1.0, 1.0, 1.0)), kw.get("bias", (0, 0, 0)), kw.get("gamma", (1.0, 1.0, 1.0)), cr)
            want = U.adjust_rgb(clip, strength, color_range=cr, **kw)
            for f in range(3):
                sums = [int(clip[f, :, :, c].sum(dtype=np.int64)) for c in range(3)]
                tab = TW.adjust_tables(sums, 32 * 24, strength, plan)
                for c in range(3):
                    assert np.array_equal(tab[c][clip[f, :, :, c]], want[f, :, :, c]), (strength, cr, kw, f, c)
                    if c < 2 or f != 1:
                        assert len(np.unique(clip[f, :, :, c])) == 256


def test_the_library_gains_equal_the_python_gains_bit_for_bit():
    r = np.random.default_rng(11)
    n = 1920 * 1080
    sums = [tuple(int(v) for v in r.integers(0, n * 255 + 1, 3)) for _ in range(200)] + [(0, 0, 0), (5, 0, 0), (0, 0, 7), (n * 255,) * 3, (1, 2, 0)]
    for s in sums:
        py = TW.normalize_gains(*[EQ.plane_average(v, n) for v in s])
        lib = TW.adjust_frame_params(s, n)
        assert np.array_equal(np.array(py).view(np.uint64), np.array(lib).view(np.uint64)), (s, py, lib)
    for c in _golden("adjust"):                                                   # and the recorded strings come out of the same function
        if "averages" in c["args"] and c["calls"] and 0 < c["args"]["strength"] <= 1:
            assert c["calls"][0][1] == TW.normalize_exprs(TW.normalize_gains(*c["args"]["averages"]))
    with pytest.raises(ValueError):
        TW.adjust_frame_params((1, -1, 0), n)


def test_header_and_bindings_agree():
    assert ctypes.sizeof(nat.TweakParams) == 560 and ctypes.sizeof(nat.AdjustParams) == 816          # static_asserts of rt_filters.cpp
    header = open(os.path.join(ROOT, "include", "havc_mi355.h")).read()
    names = [s[0] for s in nat.SYMBOLS]
    for sym in ("havc_tweak_clip", "havc_rgb_to_yuv420", "havc_yuv420_to_rgb", "havc_tweak_weights", "havc_adjust_rgb_clip", "havc_adjust_frame_params"):
        assert re.search(r"\bint " + sym + r"\(", header) and sym in names, sym
    assert TW.MAX_SIDE == int(re.search(r"#define TW_MAX_SIDE (\d+)", open(os.path.join(ROOT, "vsdeoldify_amd", "csrc", "kernels.h")).read()).group(1))
    assert np.array_equal(TW.gamma_table(1), np.arange(256)) and TW.gamma_table(0).tolist() == [0] * 255 + [255]
    assert TW.gamma_table(2.2)[128] == int(pow(128 / 255, 1 / 2.2) * 255 + 0.5)
