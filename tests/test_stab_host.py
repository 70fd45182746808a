"""CPU (-m "not gpu"): HAVC_stabilizer(stab=True) -- what vsdeoldify_amd/chroma_stab.py derives against tests/golden/chroma_stab.npz (the executed reference,
tools/gen_golden_stab.py), the frame-level decision of the kernels (havc_chroma_stab_frame_params: their C++ on the host) against tests/stab_util.py, the
refusals, and stab_util's AverageFrames scene walk and flicker stand-in on hand-written cases."""
import inspect
import json
import os

import numpy as np
import pytest

from tests import stab_util as SU
from tests.conftest import GOLDEN
from vsdeoldify_amd import chroma_stab as CS
from vsdeoldify_amd import havc
from vsdeoldify_amd.scdetect import SceneInfo


def _fixture():
    with np.load(os.path.join(GOLDEN, "chroma_stab.npz")) as g:
        return json.loads(str(g["plans"])), json.loads(str(g["probes"]))


def test_plan_equals_the_executed_reference():
    plans, _ = _fixture()
    seen = set()
    for p in plans:
        a = p["args"]
        kw = {k: a[k] for k in ("nframes", "mode", "sat", "tht", "weight", "tht_scen") if k in a}
        if "error" in p:
            with pytest.raises(havc.HAVCError) as e:
                CS.stab_plan(**kw)
            assert str(e.value) == p["error"] and p["calls"] == []
            continue
        got = CS.stab_plan(**kw)
        assert got["calls"] == p["calls"], a
        if "N" in p:
            assert (got["N"], got["weights"]) == (p["N"], p["weights"]), a
            seen.add((a["nframes"], a["mode"], a["tht"] > 0))
    assert seen == {(n, m, t) for n in range(2, 17) for m in "AW" for t in (False, True)}
    assert CS.weight_list(5, "W") == (5, [6, 13, 62, 6, 13])                    # the asymmetric list, as written
    assert CS.weight_list(4, "A")[0] == 5 and CS.weight_list(40, "A")[0] == 15 and CS.weight_list(1, "W")[0] == 3


def test_recover_rule_equals_the_executed_color_frame():
    _, probes = _fixture()
    taken = set()
    for p in probes:
        got = CS.recover_rule(p["n"], p["luma"], p["weight"])
        want = None if p["result"] is None else p["result"]["weight"]
        assert got == want, p
        taken.add((want is None, want is not None and want != p["weight"]))
        if p["result"] is not None:
            assert (p["result"]["color"], p["result"]["gray"], p["result"]["hue_adjust"], p["result"]["return_mask"]) == ("color", "gray", "none", False)
    assert taken == {(True, False), (False, False), (False, True)}


def test_frame_params_equal_the_definition():
    npix = 34 * 66
    cases = []
    for weight in (0.2, 0.0, -0.3, -0.8, -0.95):
        for tht_scen in (0.0, 0.25, 0.5, 0.8, 1.0, 1.5, -0.1):
            for count in (0, 1, npix // 4, npix // 2 - 1, npix // 2, npix // 2 + 1, npix - 1, npix):
                for mean in (0.0, 255 * 0.21, 255 * 0.5, 255 * 0.79, 255.0):
                    cases.append((int(mean * npix), count, npix, weight, tht_scen))
    # the boundaries: f_luma exactly 0.22 / 0.78 (1000 pixels: sum / 1000 / 255) and one rounding step on either side; fraction exactly == tht_scen
    for s in (56100, 56099, 56101, 198900, 198899, 198901, 56099872 // 1000):
        cases.append((s, 500, 1000, 0.2, 0.5))
    for count, ts in ((500, 0.5), (501, 0.5), (250, 0.25), (251, 0.25), (800, 0.8), (801, 0.8), (1000, 1.0), (1000, 0.999), (0, 0.0), (1, 0.0)):
        cases.append((128000, count, 1000, 0.2, ts))
    gates = set()
    for c in cases:
        assert CS.frame_params(*c) == SU.frame_decision(*c), c
        gates.add(CS.frame_params(*c)[1])
    assert gates == {False, True}
    assert CS.frame_params(56100, 0, 1000, 0.2, 0.5) == (0.2, False) and CS.frame_params(56099, 0, 1000, 0.2, 0.5)[0] == -0.8       # 0.22 is inside
    assert CS.frame_params(198900, 0, 1000, 0.2, 0.5)[0] == 0.2 and CS.frame_params(198901, 0, 1000, 0.2, 0.5)[0] == -0.8            # 0.78 is inside
    assert CS.frame_params(128000, 500, 1000, 0.2, 0.5)[1] is False and CS.frame_params(128000, 501, 1000, 0.2, 0.5)[1] is True      # > tht_scen, not >=
    assert CS.frame_params(128000, 1000, 1000, 0.2, 1.0)[1] is False and CS.frame_params(128000, 1000, 1000, 0.2, 0.0)[1] is False   # 0 and 1 switch it off
    assert CS.frame_params(56099, 0, 1000, -0.9, 0.5)[0] == -0.9                                                                      # min(weight, -0.8)
    for bad in ((-1, 0, 10, 0.2, 0.5), (0, 11, 10, 0.2, 0.5), (0, 0, 0, 0.2, 0.5), (0, 0, 10, float("nan"), 0.5)):
        with pytest.raises(ValueError):
            CS.frame_params(*bad)


def test_frame_decision_agrees_with_the_frame_path():
    """stab_util.frame_decision (integer sums) and stab_util.restore_frame (the frames themselves) are the same rule"""
    from oracle import cvcolor
    clip = SU.make_clip(34, 66, 19)
    for f in (15, 16, 17, 18):
        book = {}
        SU.restore_frame(f, clip[f], clip[f - 1], 1.0, 15, 0.2, 0.5, "k", book)
        sum_y = int(cvcolor.rgb2yuv_u8(clip[f])[:, :, 0].sum(dtype=np.int64))
        count = int((cvcolor.rgb2hsv_u8(clip[f])[:, :, 1] < 15).sum())
        w, gate = SU.frame_decision(sum_y, count, 34 * 66, 0.2, 0.5)
        assert (w != 0.2, gate) == (book["band"]["k"], book["gate"]["k"])


def _info(n, prev=(), nxt=()):
    p, q = np.zeros(n, np.int8), np.zeros(n, np.int8)
    p[list(prev)] = 1
    q[list(nxt)] = 1
    return SceneInfo(p, q, np.full(n, 0.5), np.zeros(n), 0.1, 0)


def test_average_frames_scene_walk_by_hand():
    src = SU.temporal_sources(6, 5)
    assert src.tolist() == [[0, 0, 0, 1, 2], [0, 0, 1, 2, 3], [0, 1, 2, 3, 4], [1, 2, 3, 4, 5], [2, 3, 4, 5, 5], [3, 4, 5, 5, 5]]      # clamped to the clip
    book = {}
    src = SU.temporal_sources(6, 5, _info(6, prev=[3], nxt=[2]), book=book)
    # frame 3 starts a scene: nothing from before it reaches frames 3..5, nothing from it on reaches frames 0..2
    assert src.tolist() == [[0, 0, 0, 1, 2], [0, 0, 1, 2, 2], [0, 1, 2, 2, 2], [3, 3, 3, 4, 5], [3, 3, 4, 5, 5], [3, 4, 5, 5, 5]]
    assert book["replaced"] == 6
    # the walk starts AT the centre and stops at the first flag: frame 4's own flag wins over frame 3's
    assert SU.temporal_sources(6, 5, _info(6, prev=[3, 4]))[4].tolist() == [4, 4, 4, 5, 5]
    assert SU.temporal_sources(6, 5, _info(6, prev=[3, 4]))[5].tolist() == [4, 4, 5, 5, 5]
    # scenechange=False (vs_get_clip_frame) ignores the flags
    assert SU.temporal_sources(6, 5, _info(6, prev=[3], nxt=[2]), scenechange=False).tolist() == SU.temporal_sources(6, 5).tolist()
    plane = np.array([[10], [20], [30], [200], [210], [220]], np.uint8)
    got = SU.average_temporal(plane, [6, 13, 62, 6, 13], _info(6, prev=[3], nxt=[2]))
    want = [(6 * 10 + 13 * 10 + 62 * 10 + 6 * 20 + 13 * 30 + 50) // 100, (6 * 10 + 13 * 10 + 62 * 20 + 6 * 30 + 13 * 30 + 50) // 100,
            (6 * 10 + 13 * 20 + 62 * 30 + 6 * 30 + 13 * 30 + 50) // 100, (6 * 200 + 13 * 200 + 62 * 200 + 6 * 210 + 13 * 220 + 50) // 100,
            (6 * 200 + 13 * 200 + 62 * 210 + 6 * 220 + 13 * 220 + 50) // 100, (6 * 200 + 13 * 210 + 62 * 220 + 6 * 220 + 13 * 220 + 50) // 100]
    assert got[:, 0].tolist() == want
    assert SU.average([np.array([255], np.uint8)] * 3, [50, 50, 50]).tolist() == [255]           # clamped
    assert SU.average([np.array([1], np.uint8), np.array([2], np.uint8), np.array([1], np.uint8)], [25, 50, 25]).tolist() == [2]    # 1.5 rounds up


def test_reduce_flicker_by_hand():
    col = lambda v: np.array(v, np.uint8).reshape(-1, 1, 1, 1).repeat(3, -1)
    # a sample that alternates (the frames two away agree with it: d = 0) is pulled to the average; the first and last two frames pass
    assert SU.reduce_flicker(col([140, 100, 140, 100, 140, 100, 140]))[:, 0, 0, 0].tolist() == [140, 100, 120, 120, 120, 100, 140]
    # a single spike stays: with d = 40 the limits of frame 2 are [140, 140], and its neighbours' limits are their own value
    assert SU.reduce_flicker(col([100, 100, 140, 100, 100, 100, 100]))[:, 0, 0, 0].tolist() == [100, 100, 140, 100, 100, 100, 100]
    # a real change (the frames two away differ as much) is left alone
    assert SU.reduce_flicker(col([0, 0, 0, 200, 200, 200]))[:, 0, 0, 0].tolist() == [0, 0, 0, 200, 200, 200]
    four = col([1, 200, 3, 100])
    assert np.array_equal(SU.reduce_flicker(four), four)


def test_refusals_and_the_single_frame_rule():
    f = np.zeros((8, 8, 3), np.uint8)
    with pytest.raises(NotImplementedError, match="vs_chroma_stabilizer_ex.*pass a clip"):
        havc.HAVC_stabilizer(f, stab=True)
    clip = np.zeros((3, 8, 8, 3), np.uint8)
    with pytest.raises(havc.HAVCError, match="HybridAVC: unknown average method: Q"):
        havc.HAVC_stabilizer(clip, stab=True, stab_p=(5, "Q", 1, 15, 0.2, 0.8))
    with pytest.raises(havc.HAVCError, match="YUV420 round trip"):
        havc.HAVC_stabilizer(np.zeros((3, 8, 7, 3), np.uint8), stab=True)        # frame_size = min(384, 7) = 7
    with pytest.raises(havc.HAVCError, match="scenes= must be the SceneInfo of this clip"):
        havc.HAVC_stabilizer_scenes(clip, _info(4), stab=True)
    with pytest.raises(havc.HAVCError, match="stab_p needs"):
        havc.HAVC_stabilizer(clip, stab=True, stab_p=(5, "A"))
    import vsdeoldify_amd
    assert vsdeoldify_amd.HAVC_stabilizer_scenes is havc.HAVC_stabilizer_scenes
    a, b = list(inspect.signature(havc.HAVC_stabilizer).parameters.values()), list(inspect.signature(havc.HAVC_stabilizer_scenes).parameters.values())
    assert [q.name for q in b] == ["clip", "scenes"] + [q.name for q in a[1:]] and [q.default for q in b[2:]] == [q.default for q in a[1:]]


def test_native_symbols_and_struct_layout():
    import ctypes as C
    from vsdeoldify_amd import _native as nat
    lib = nat.load()
    for name in ("havc_chroma_stab_clip", "havc_chroma_stab_frame_params", "havc_reduce_flicker_clip"):
        assert hasattr(lib, name)
    assert C.sizeof(nat.ChromaStabParams) == 136                                 # the static_assert of csrc/rt_filters.cpp
    out = (C.c_double * 2)()
    assert lib.havc_chroma_stab_frame_params(0, 0, 10, 0.2, 0.5, None) == -1 and lib.havc_chroma_stab_frame_params(0, 0, 10, 0.2, 0.5, out) == 0
