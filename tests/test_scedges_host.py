"""CPU: edge-masked scene detection (vsdeoldify_amd/scdetect_edge.py) against tests/golden/scdetect_edges.npz -- made by tools/gen_golden_scedges.py, which
executes the reference's SceneDetectEdges, vs_edge_based_scenedetect and the edge file's SceneDetectionFiltered --, the self-checks of the numpy pixel
definition (tests/scedges_util.py), the ABI, and HAVC_SceneDetectEdges' refusals before any GPU context exists."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from tests import scedges_util as U
from vsdeoldify_amd import _native as nat
from vsdeoldify_amd import havc
from vsdeoldify_amd import scdetect as SD
from vsdeoldify_amd import scdetect_edge as SE

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "havc_mi355.h")


def _scores(g, asked):
    k, a, b = (int(v) for v in g["key"])

    def scores(t_n, last):
        asked.append((t_n, last))
        return np.float64(g["ssim_table"][(a * t_n + b * last) % k]), float(g["hist_table"][(a * t_n + b * last) % k])
    return scores


def _sad_prev(scd, n_pixels):
    """a difference that makes the misc.SCDetect stand-in give the prescribed flag"""
    return np.where(np.asarray(scd) == 1, n_pixels * 255, 0).astype(np.int64)


def test_scene_flags_edges_reproduce_the_executed_reference():
    g = U.fixture()
    npix = int(g["n_pixels"])
    reached, statuses = set(), set()
    for i in range(int(g["n_edges"])):
        kw = U.params(g, f"edges_{i}_params")
        kw.pop("sc_debug", None)
        kw.pop("sc_diff_offset", None)                                 # the offset enters the statistics, not the selectors
        asked, dbg = [], {}
        got = SE.scene_flags_edges(g[f"edges_{i}_sum_y"], _sad_prev(g[f"edges_{i}_scd"], npix), g[f"edges_{i}_sad_next"], g[f"edges_{i}_sum_masked"], npix,
                                   scores=_scores(g, asked), debug=dbg, **kw)
        assert isinstance(got, SE.EdgeSceneInfo) and isinstance(got, SD.SceneInfo)
        has_flags, has_luma, has_reason = g[f"edges_{i}_has_props"]
        assert np.array_equal(got.scene_change_prev, g[f"edges_{i}_prev"]) and np.array_equal(got.scene_change_next, g[f"edges_{i}_next"]), i
        if has_luma:
            assert np.array_equal(got.sc_luma, g[f"edges_{i}_luma"]) and np.array_equal(got.sc_reason, g[f"edges_{i}_reason"]), i
        else:                                                          # the early returns set neither prop
            assert not has_reason and not got.sc_luma.any() and not got.sc_reason.any()
        assert not got.sc_ratio.any() and (got.sc_threshold, got.sc_frequency) == (kw["threshold"], kw.get("frequency", 0))
        assert asked == [tuple(p) for p in g[f"edges_{i}_pairs"]], i
        if kw.get("ssim_threshold", 0) > 0 and has_luma:               # the routing: the filter ran on the constants, and they are what the clip carries
            assert (got.sc_luma == SE.ROUTED_LUMA).all() and (got.sc_reason == SE.ROUTED_REASON).all()
        elif has_luma:
            reached |= set(got.sc_reason[1:].tolist())
            assert got.sc_luma[0] == 0.10 and got.sc_reason[0] == 4    # frame 0 is hard-wired
        statuses |= set(dbg.get("status", {}).values())
        assert has_flags or not got.scene_change_prev.any()
    assert reached == {0, 1, 2, 3, 4}
    assert statuses == {"Accepted(First)", "Accepted", "Accepted(edge_max)", "Accepted(tht_max)", "Accepted(tht_max+edge_max)", "Skipped", "Rejected"}


def test_edge_detector_alone_and_its_rules():
    g = U.fixture()
    npix = int(g["n_pixels"])
    for i in (0, 2):                                                   # the cases without the filter: every prop is the detector's
        kw = U.params(g, f"edges_{i}_params")
        prev, nxt, luma, reason = SE.edge_detector(g[f"edges_{i}_sum_y"], g[f"edges_{i}_scd"], g[f"edges_{i}_sad_next"], g[f"edges_{i}_sum_masked"], npix,
                                                   kw["threshold"], kw["sc_min_int"], kw["sc_mult_tht"], kw["tht_white"], kw["tht_black"])
        assert np.array_equal(prev, g[f"edges_{i}_prev"]) and np.array_equal(luma, g[f"edges_{i}_luma"]) and np.array_equal(reason, g[f"edges_{i}_reason"])
        assert not nxt.any()
        lum = g[f"edges_{i}_luma"][1:]
        rejected = (lum < kw["tht_black"]) | (lum > kw["tht_white"])
        assert (lum < kw["tht_black"]).any() and (lum > kw["tht_white"]).any() and not prev[1:][rejected].any()      # a dark and a bright frame
    # the distance rule max(int(sc_mult_tht * 0.5), 3) and sc_mult_tht == 0 -> 7, on SCDetect flags two frames apart (everything else quiet)
    n, z = 12, np.zeros(12, np.int64)
    sum_y = np.full(n, int(0.4 * 255 * npix), np.int64)
    scd = np.zeros(n, np.int8)
    scd[[2, 4, 6, 9]] = 1
    for mult, want in ((4, [0, 2, 6, 9]), (6, [0, 2, 6, 9]), (8, [0, 2, 6]), (15, [0, 2, 9]), (0, [0, 2, 6, 9])):
        prev = SE.edge_detector(sum_y, scd, z, z, npix, 0.035, 20, mult, 0.70, 0.10)[0]
        assert np.flatnonzero(prev).tolist() == want, (mult, np.flatnonzero(prev))
    # sc_mult_tht == 0 means 7, not "every edge difference above 0 is mandatory": 10 * 300 / (256 * 255) = 0.04596 lies below 7 * 0.035
    quiet = SE.edge_detector(sum_y, np.zeros(n, np.int8), z, np.full(n, 300, np.int64), npix, 0.035, 20, 0, 0.70, 0.10)
    assert quiet[0].tolist() == [1] + [0] * 11 and not quiet[3][1:].any()
    loud = SE.edge_detector(sum_y, np.zeros(n, np.int8), z, np.full(n, 1700, np.int64), npix, 0.035, 20, 0, 0.70, 0.10)     # 0.26 > 0.245: edge_max
    assert np.flatnonzero(loud[0]).tolist() == [0, 1, 4, 7, 10] and set(loud[3][[1, 4, 7, 10]]) == {2}


def test_edge_scene_filter_reproduces_the_executed_reference():
    g = U.fixture()
    overridden = 0
    for i in range(int(g["n_filter"])):
        p = U.params(g, f"filter_{i}_params")
        asked, dbg = [], {}
        prev, nxt = SE.edge_scene_filter(g[f"filter_{i}_in_prev"], np.zeros_like(g[f"filter_{i}_in_prev"]), g[f"filter_{i}_luma"], g[f"filter_{i}_reason"],
                                         _scores(g, asked), p["ssim_tht"], p["min_length"], p["tht_white"], p["tht_black"], p["frequency"], chunk=p["chunk"],
                                         debug=dbg)
        assert np.array_equal(prev, g[f"filter_{i}_prev"]) and np.array_equal(nxt, g[f"filter_{i}_next"]), i
        assert asked == [tuple(q) for q in g[f"filter_{i}_pairs"]], i
        if g[f"filter_{i}_reason"][0] < 2:                              # _sc_prev_reason stays what frame 0 carried: the override is open or shut per case
            overridden += sum(1 for t_n in dbg["scores"] if g[f"filter_{i}_reason"][t_n] > 1)
    assert overridden > 0
    last = int(g["n_filter"]) - 1                                       # a chunk boundary: candidates scored on both sides of frame 5000
    assert g[f"filter_{last}_pairs"][:, 0].min() < 5000 <= g[f"filter_{last}_pairs"][:, 0].max()


def test_next_index_is_the_reference_clip_arithmetic():
    g = U.fixture()
    seen = set()
    for i in range(int(g["n_edges"])):
        j = g[f"edges_{i}_next_index"]
        if len(j):
            n, offset = len(j), max(U.params(g, f"edges_{i}_params").get("sc_diff_offset", 2), 1)
            assert [SE.next_index(k, n, offset) for k in range(n)] == j.tolist()
            seen.add(offset)
    assert {1, 2, 5, 25} <= seen
    for n in (6, 9):
        for offset in (1, 2, n - 1):
            assert [SE.next_index(k, n, offset) for k in range(n)] == [k + offset if k + offset < n else n - offset for k in range(n)]
    assert [SE.next_index(k, 6, 5) for k in range(6)] == [5, 1, 1, 1, 1, 1]


def test_numpy_definition_self_checks():
    # reflect: n = 1, 2, 3
    assert U.reflect(np.arange(-4, 5), 1).tolist() == [0] * 9
    assert U.reflect(np.arange(-4, 5), 2).tolist() == [0, 1, 0, 1, 0, 1, 0, 1, 0]
    assert U.reflect(np.arange(-5, 8), 3).tolist() == [1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1]
    # a constant frame has mask 0
    for v in (0, 37, 255):
        assert not U.edge_mask(np.full((9, 13), v, np.uint8)).any()
    # every Kirsch pass is |8 S3 - 3 S8| clamped, S3 over the three neighbours the reference's matrix weights 5
    r = np.random.default_rng(1)
    y = r.integers(100, 116, (12, 17)).astype(np.int64)
    nb = {(dy, dx): U.shifted(y, dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0)}
    s8 = sum(nb.values())
    ring = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]              # row-major, as `w[:4] + [0] + w[4:]` lays them out
    mats = U.kirsch_matrices()
    assert mats[0] == [5, 5, 5, -3, 0, -3, -3, -3, -3] and mats[1] == [-3, 5, 5, 5, 0, -3, -3, -3, -3] and all(sum(m) == 0 for m in mats)
    for i, p in enumerate(U.kirsch_passes(y)):
        s3 = sum(nb[ring[(i + k) % 8]] for k in range(3))
        assert np.array_equal(p, np.minimum(np.abs(8 * s3 - 3 * s8), 255)) and 0 < p.max() and p.min() < 255
    # a horizontal ramp: the blur leaves it alone away from the borders and the Prewitt sum of three rows over two columns, halved, is 3 x the slope
    for slope in (1, 2, 5):
        ramp = np.tile(slope * np.arange(40, dtype=np.int64), (20, 1))
        t = U.tcanny(ramp, SE.DEF_CANNY_SIGMA)
        assert (t[:, 6:-6] == 3 * slope).all(), t[5]
    # the table and the weights
    e = U.enhance_table()
    assert e[0] == 0 and e[255] == 255 and e[64] == 128 and (np.diff(e.astype(int)) >= 0).all()
    for sigma, rad in ((1.2, 4), (0.6, 2), (2.5, 8), (0.1, 1)):
        w = U.weights(sigma)
        assert U.radius(sigma) == rad and len(w) == 2 * rad + 1 and w.dtype == np.float32 and np.array_equal(w, w[::-1]) and abs(float(w.sum()) - 1) < 1e-6
    # the recipe clip: a mask around 70, a masked sum near 30 % of the plain one
    st, mask = U.reference_stats(130, 257, 2, True, SE.DEF_CANNY_SIGMA)
    assert 40 < mask.mean() < 100 and 0.15 < st["sum_masked"].sum() / st["sad_next"].sum() < 0.45
    assert st["sad_prev"][0] == 0 and st["sad_next"][4] == st["sad_next"][4] and st["sad_next"][-2] == 0 == st["sum_masked"][-2]     # j == n at n = N - offset


def test_host_tables_equal_the_definition():
    lib = nat.load()
    for sigma in (1.2, 0.6, 2.5, 0.1, 1.0):
        enh, w, r = np.zeros(256, np.uint8), np.full(17, -1, np.float32), ctypes.c_int()
        assert lib.havc_scene_edge_tables(sigma, nat.as_ptr(enh), nat.as_ptr(w), ctypes.byref(r)) == 0
        assert r.value == U.radius(sigma) and np.array_equal(enh, U.enhance_table())
        assert w[:2 * r.value + 1].tobytes() == U.weights(sigma).tobytes() and not w[2 * r.value + 1:].any()
    for sigma in (0.0, -1.0, 2.6, float("nan")):
        assert lib.havc_scene_edge_tables(sigma, nat.as_ptr(enh), nat.as_ptr(w), ctypes.byref(r)) != 0


def test_abi_matches_the_header():
    src = open(HEADER).read()
    m = re.search(r"typedef struct havc_edge_params \{(.*?)\} havc_edge_params;", src, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == [f[0] for f in nat.EdgeParams._fields_]
    assert ctypes.sizeof(nat.EdgeParams) == 40 and nat.EdgeParams.sigma.offset == 32
    m = re.search(r"typedef struct havc_edge_rec \{(.*?)\} havc_edge_rec;", src, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == list(nat.EDGE_REC_DTYPE.names) == ["sum_y", "sad_prev", "sad_next", "sum_masked"]
    assert nat.EDGE_REC_DTYPE.itemsize == 32 and [nat.EDGE_REC_DTYPE.fields[n][1] for n in names] == [0, 8, 16, 24]
    assert "int havc_scene_edge_stats(havc_ctx* ctx, const uint8_t* clip, const havc_edge_params* params, havc_edge_rec* out, uint8_t* mask_tap);" in src
    sym = {s[0]: s for s in nat.SYMBOLS}
    assert len(sym["havc_scene_edge_stats"][2]) == 5 and len(sym["havc_scene_edge_tables"][2]) == 4
    assert hasattr(nat.load(), "havc_scene_edge_stats")


def test_scene_detect_edges_refusals_come_before_any_gpu_work(monkeypatch):
    def no_gpu(*a, **k):
        raise AssertionError("a GPU context was asked for")
    monkeypatch.setattr(havc, "get_context", no_gpu)
    clip = np.zeros((3, 8, 8, 3), np.uint8)
    with pytest.raises(havc.HAVCError, match="not a clip"):
        havc.HAVC_SceneDetectEdges(None)
    with pytest.raises(havc.HAVCError, match="not a clip"):
        havc.HAVC_SceneDetectEdges([[1, 2, 3]])
    with pytest.raises(havc.HAVCError, match="luma_range"):
        havc.HAVC_SceneDetectEdges(clip, luma_range="pc")
    with pytest.raises(havc.HAVCError, match="RGB24"):
        havc.HAVC_SceneDetectEdges(np.zeros((3, 8, 8, 1), np.uint8))
    for offset in (3, 5, 26):                                          # offset >= n_frames: gray[offset:] is empty in the reference as well
        with pytest.raises(havc.HAVCError, match="sc_tht_offset"):
            havc.HAVC_SceneDetectEdges(clip, sc_tht_offset=offset)
    with pytest.raises(ValueError, match="more than 2 frames"):
        SE.edges_offset(2, 2)
    assert SE.edges_offset(0, 3) == 1 and SE.edges_offset(-4, 3) == 1 and SE.edges_offset(2, 3) == 2
    # sc_threshold == 0 is the reference's early return (frequency is 0): no flag, no pixel read, no context
    got = havc.HAVC_SceneDetectEdges(clip, sc_threshold=0)
    assert isinstance(got, SE.EdgeSceneInfo) and not got.scene_change_prev.any() and (got.sc_threshold, got.sc_frequency) == (0, 0)
    assert SE.edges_branch(0, 0) == "none" and SE.edges_branch(0, 5) == SE.edges_branch(0.05, 1) == "frequency" and SE.edges_branch(0.05, 25) == "detect"
    # the reference's argument list and defaults (vsdeoldify/__init__.py:3227-3230)
    sig = inspect.signature(havc.HAVC_SceneDetectEdges)
    assert [(k, v.default) for k, v in sig.parameters.items() if v.kind is v.POSITIONAL_OR_KEYWORD][1:] == [
        ("sc_threshold", 0.035), ("sc_tht_offset", 2), ("sc_tht_ssim", 0.80), ("sc_min_int", 20), ("sc_mult_tht", 15), ("sc_tht_white", 0.70),
        ("sc_tht_black", 0.10), ("sc_debug", False)]
    assert [k for k, v in sig.parameters.items() if v.kind is v.KEYWORD_ONLY] == ["device_index", "luma_range"]
    import vsdeoldify_amd
    assert vsdeoldify_amd.HAVC_SceneDetectEdges is havc.HAVC_SceneDetectEdges
    # the result is a SceneInfo: accepted wherever scenes= is; the sc_algo = 1 refusal of HAVC_extract_reference_frames stays
    with pytest.raises(NotImplementedError, match="sc_algo = 1"):
        havc.HAVC_extract_reference_frames(clip, sc_algo=1)
