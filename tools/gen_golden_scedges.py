#!/usr/bin/env python3
"""Golden vectors for edge-masked scene detection (vsslib/vsscdetect_edge.py) by EXECUTING the reference (build container only).  Writes
tests/golden/scdetect_edges.npz (data only).

  * edges_<i>: the reference's own SceneDetectEdges (:32-102) -> vs_edge_based_scenedetect (:140-286, selector body set_sc_prop included) -> with
    ssim_threshold > 0 its SceneDetectionFiltered.SceneDetectFilter (:354-494, selector body set_scenechange included), on a stand-in clip.  The pixel
    filters (zimg, misc.SCDetect, std.Convolution, akarin.Expr, TCanny, std.MaskedMerge, std.PlaneStats) are native code: their stand-ins hand on WHAT a clip
    is (gray / diff / masked diff, and of which source frames), and the numbers the selectors read of them are INPUTS of the fixture -- the gray planes
    (their mean is sc_luma), misc.SCDetect's flags, PlaneStatsAverage of the difference and of the masked difference (sum / (n_pixels * 255)), and the
    filter's SSIM / histogram scores (recorded tables, as in gen_golden_scfilter.py).  Outputs: the four props of every frame of the clip SceneDetectEdges
    returns, the pairs the filter scored, and the frame `gray[offset:] + gray[-offset]` handed out as frame n (a request beyond a clip's end is answered
    with its last frame: VapourSynth's rule, restated by the stand-in's get()).
    std.CopyFrameProps(props=[...]) copies the named props and drops a name the source does not carry: so the unseparated 'sc_luma' 'sc_reason' of :93-94 is
    one name nobody carries, and the filter reads the constants of :69-70.  The fixture records what the executed reference then does.
  * filter_<i>: SceneDetectionFiltered._scene_detect_filter_task / SceneDetectFilter directly, on frames that carry prescribed props (sc_luma and sc_reason
    vary here, which SceneDetectEdges' routing never lets happen): every branch of the edge file's own filter.

Line tracing asserts that every `if` / `elif` of both selectors went both ways; `elif n < clip.num_frames` (:431) cannot be false (n is a frame number of
that clip), so the else of :454-457 is never reached.
"""
import collections
import importlib
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import refshim  # noqa: E402

refshim.install()
vs = sys.modules["vapoursynth"]
for i, n in enumerate(("DEBUG", "INFORMATION", "WARNING", "CRITICAL", "FATAL")):
    setattr(vs, "MESSAGE_TYPE_" + n, i)
vs.GRAY8, vs.GRAY = "gray8", "gray"
core = vs.core
core.log_message = lambda *a: None

K, A, B = 997, 7, 13
rng = np.random.default_rng(20261020)
ssim_table = np.round(rng.uniform(0.0, 1.0, K), 6)
hist_table = np.round(rng.uniform(0.0, 1.0, K) ** 2, 6)           # compareHist's distance: small = alike


def number(x):
    return int(np.asarray(x).ravel()[0])


def key(t_n, last):
    return (A * t_n + B * last) % K


calls = []


def structural_similarity(im1, im2, full=False):
    calls.append((number(im1), number(im2)))
    return np.float64(ssim_table[key(number(im1), number(im2))])


def compare_hist(H1, H2, method):
    assert method == "hellinger"
    return float(hist_table[key(number(H2), number(H1))])


sk = types.ModuleType("skimage")
sk.metrics = types.ModuleType("skimage.metrics")
sk.metrics.structural_similarity = structural_similarity
sys.modules["skimage"], sys.modules["skimage.metrics"] = sk, sk.metrics
cv2 = sys.modules["cv2"]
cv2.COLOR_RGB2GRAY, cv2.COLOR_RGB2YUV, cv2.HISTCMP_HELLINGER = "gray", "yuv", "hellinger"
cv2.cvtColor = lambda a, code: a[:, :, 0] if code == "gray" else a
cv2.split = lambda a: [a[:, :, k] for k in range(a.shape[2])]
cv2.calcHist = lambda images, channels, mask, size, ranges: np.full((size[0], 1), float(number(images[0])))
cv2.normalize = lambda src, dst: src
cv2.compareHist = compare_hist
plug = types.ModuleType("vsdeoldify.vsslib.vsplugins")
for name in ("load_Retinex_plugin", "load_TCanny_plugin", "load_Akarin_plugin", "load_SCDetect_plugin", "load_MVTool_plugin"):
    setattr(plug, name, lambda *a, **k: None)
sys.modules["vsdeoldify.vsslib.vsplugins"] = plug
rsz = types.ModuleType("vsdeoldify.vsslib.vsresize")
rsz.resize_min_HW = lambda clip: clip                              # zimg: the size does not enter the selectors; the props travel with the clip
sys.modules["vsdeoldify.vsslib.vsresize"] = rsz


class Props(dict):
    __getattr__ = dict.__getitem__


class Frame:
    """what the selectors touch of a vs.VideoFrame: planes, props, copy().  src: the frame of the source clip it was made of."""
    def __init__(self, src, planes, props=None):
        self.src, self.planes, self.props = src, planes, Props(props or {})
        self.format = types.SimpleNamespace(num_planes=len(planes))

    def __getitem__(self, plane):
        return self.planes[plane]

    def copy(self):
        return Frame(self.src, self.planes, self.props)


class Clip:
    """a list of frames + what they are (kind).  std.ModifyFrame evaluates its selector on every frame IN ORDER: both selectors carry state."""
    def __init__(self, frames, kind, case):
        self.frames, self.kind, self.case, self.num_frames = list(frames), kind, case, len(frames)
        self.std = types.SimpleNamespace(SetFrameProp=self._set_prop, ModifyFrame=self._modify, CopyFrameProps=self._copy_props,
                                         Convolution=lambda matrix, saturate: self.like("conv"))
        self.misc = types.SimpleNamespace(SCDetect=self._scdetect)
        self.tcanny = types.SimpleNamespace(TCanny=lambda mode, sigma: self.like("tcanny"))

    def __len__(self):
        return self.num_frames

    def like(self, kind, frames=None):
        return Clip(self.frames if frames is None else frames, kind, self.case)

    def get(self, n):
        return self.frames[min(n, self.num_frames - 1)]               # a request beyond the end: the last frame

    def get_frame(self, n):
        return self.frames[n]

    def __getitem__(self, s):
        return self.like(self.kind, self.frames[s] if isinstance(s, slice) else [self.frames[s]])

    def __add__(self, other):
        return self.like(self.kind, self.frames + other.frames)

    def _set_prop(self, prop, floatval=None, intval=None):
        out = [f.copy() for f in self.frames]
        for f in out:
            f.props[prop] = float(floatval) if floatval is not None else int(intval)
        return self.like(self.kind, out)

    def _copy_props(self, prop_src, props):
        out = [f.copy() for f in self.frames]
        for f, s in zip(out, prop_src.frames):
            for p in props:
                if p in s.props:
                    f.props[p] = s.props[p]
                else:
                    f.props.pop(p, None)
        return self.like(self.kind, out)

    def _modify(self, clips, selector):
        out = []
        for n in range(self.num_frames):
            f = [c.frames[n] for c in clips]
            out.append(selector(n, f[0] if len(clips) == 1 else f))
        return self.like(self.kind, out)

    def _scdetect(self, threshold):
        assert self.kind == "gray" and threshold == 0.10
        out = [f.copy() for f in self.frames]
        for f, p in zip(out, self.case["scd"]):
            f.props["_SceneChangePrev"], f.props["_SceneChangeNext"] = int(p), 0
        return self.like("gray", out)


def to_gray(clip, format, matrix_s):
    assert format == vs.GRAY8 and matrix_s == "709"
    return clip.like("gray", [Frame(f.src, [p], f.props) for f, p in zip(clip.frames, clip.case["planes"])])


def expr(clips, e):
    clips = clips if isinstance(clips, list) else [clips]
    if e == 'x y - abs':                                              # :179: the difference of frame n and the frame clip_next hands out as frame n
        cur, nxt = clips
        assert cur.kind == nxt.kind == "gray"
        cur.case["next_index"] = [nxt.get(n).src for n in range(cur.num_frames)]
        return cur.like("diff")
    return clips[0].like("expr")


def masked_merge(a, b, mask):
    assert a.kind == "blank" and b.kind == "diff" and mask.kind == "expr"
    return b.like("masked")


def plane_stats(clip):
    table = clip.case["avg_masked"] if clip.kind == "masked" else clip.case["avg_diff"]
    assert clip.kind in ("masked", "diff")
    return clip.like(clip.kind, [Frame(f.src, f.planes, {"PlaneStatsAverage": float(table[f.src])}) for f in clip.frames])


core.resize = types.SimpleNamespace(Bicubic=to_gray)
core.akarin = types.SimpleNamespace(Expr=expr)
core.std = types.SimpleNamespace(Expr=expr, MaskedMerge=masked_merge, BlankClip=lambda c: c.like("blank"), PlaneStats=plane_stats,
                                 Splice=lambda clips: clips[0].like(clips[0].kind, [f for c in clips for f in c.frames]))
se = importlib.import_module("vsdeoldify.vsslib.vsscdetect_edge")

hits = {"set_sc_prop": collections.Counter(), "set_scenechange": collections.Counter()}
REF_FILE = se.__file__


def tracer(frame, event, arg):
    name = frame.f_code.co_name
    if name not in hits or frame.f_code.co_filename != REF_FILE:
        return None

    def lines(frame, event, arg):
        if event == "line":
            hits[name][frame.f_lineno] += 1
        return lines
    return lines


NP = 256


def rgb_clip(case, n, props=None):
    """frames whose three 1 x 1 planes hold the frame's number (the filter's pixel stand-ins read it)"""
    return Clip([Frame(i, [np.full((1, 1), i, np.int64)] * 3, props[i] if props else None) for i in range(n)], "rgb", case)


def run_edges(case):
    n = len(case["sum_masked"])
    case["avg_masked"] = [float(int(s)) / (float(NP) * 255.0) for s in case["sum_masked"]]
    case["avg_diff"] = [float(int(s)) / (float(NP) * 255.0) for s in case["sad_next"]]
    sys.settrace(tracer)
    try:
        out = se.SceneDetectEdges(rgb_clip(case, n), **case["kw"])
    finally:
        sys.settrace(None)
    return out.frames


def run_filter(case):
    props = [{"_SceneChangePrev": int(p), "_SceneChangeNext": 0, "sc_luma": float(l), "sc_reason": int(r)}
             for p, l, r in zip(case["prev"], case["luma"], case["reason"])]
    frames = rgb_clip(case, len(props), props)
    det = se.SceneDetectionFiltered(sc_tht_white=case["tht_white"], sc_tht_black=case["tht_black"], sc_frequency=case["frequency"], sc_debug=case["debug"])
    sys.settrace(tracer)
    try:
        if case["chunk"] == 5000:
            out = det.SceneDetectFilter(frames, ssim_threshold=case["ssim_tht"], min_length=case["min_length"]).frames
        else:
            out = []
            for t_start in range(0, len(props), case["chunk"]):
                out += det._scene_detect_filter_task(t_start, frames[t_start:t_start + case["chunk"]], case["ssim_tht"], case["min_length"]).frames
    finally:
        sys.settrace(None)
    return out


def lumas(n, dark=0.2, white=0.12):
    u = rng.uniform(0, 1, n)
    l = np.where(u < dark, rng.uniform(0.03, 0.19, n), np.where(u > 1 - white, rng.uniform(0.66, 0.95, n), rng.uniform(0.19, 0.66, n)))
    return np.round(l, 4)


def planes_for(ls, shape=(16, 16)):
    return [np.clip(l * 255 + 12 * rng.standard_normal(shape), 0, 255).astype(np.uint8) for l in ls]


def edges_case(n, threshold, p_scd, p_big, p_mid, dark=0.2, white=0.12, **kw):
    """statistics around the detector's thresholds: edge_diff = 10 avg_masked against threshold and threshold * sc_mult_tht, ssim_diff = 4 avg_diff against
    1.75 threshold; runs of flagged frames a few frames apart so that both distance rules decide"""
    mult = kw.get("sc_mult_tht", 7) or 7
    u = rng.uniform(0, 1, n)
    edge = np.where(u < p_big, rng.uniform(1.05, 1.6, n) * threshold * mult, np.where(u < p_big + p_mid, rng.uniform(1.05, 3.0, n) * threshold,
                                                                                      rng.uniform(0.1, 0.98, n) * threshold))
    ssim = np.where(rng.uniform(0, 1, n) < 0.7, rng.uniform(1.05, 3.0, n), rng.uniform(0.2, 0.95, n)) * 1.75 * threshold
    planes = planes_for(lumas(n, dark, white))
    return dict(planes=planes, scd=(rng.uniform(0, 1, n) < p_scd).astype(np.int8), sum_masked=np.round(edge / 10 * NP * 255).astype(np.int64),
                sad_next=np.round(ssim / 4 * NP * 255).astype(np.int64), kw=dict(kw, threshold=threshold))


edges = [
    edges_case(96, 0.035, 0.10, 0.10, 0.30, ssim_threshold=0.0, sc_diff_offset=2, sc_min_int=20, sc_mult_tht=15, tht_white=0.70, tht_black=0.10),
    edges_case(96, 0.035, 0.10, 0.10, 0.30, ssim_threshold=0.80, sc_diff_offset=2, sc_min_int=20, sc_mult_tht=15, tht_white=0.70, tht_black=0.10),
    edges_case(80, 0.07, 0.25, 0.25, 0.30, ssim_threshold=0.0, sc_diff_offset=1, sc_min_int=6, sc_mult_tht=4, tht_white=0.70, tht_black=0.12),   # distance max(int(2.0), 3) = 3
    edges_case(80, 0.05, 0.20, 0.20, 0.30, ssim_threshold=0.60, sc_diff_offset=5, sc_min_int=9, sc_mult_tht=0, tht_white=0.88, tht_black=0.12, sc_debug=True),  # 0 -> 7
    edges_case(64, 0.05, 0.15, 0.15, 0.30, ssim_threshold=0.75, frequency=25, sc_diff_offset=0, sc_min_int=1, sc_mult_tht=9, tht_white=0.70, tht_black=0.10),
    edges_case(64, 0.05, 0.15, 0.15, 0.30, ssim_threshold=1.0, sc_diff_offset=25, sc_min_int=12, sc_mult_tht=7, tht_white=0.70, tht_black=0.10),
    edges_case(5040, 0.035, 0.01, 0.01, 0.05, ssim_threshold=0.80, sc_diff_offset=2, sc_min_int=20, sc_mult_tht=15, tht_white=0.70, tht_black=0.10),   # the 5000-frame batch
    edges_case(12, 0.0, 0.5, 0.5, 0.3, ssim_threshold=0.80),                                    # the early return: threshold 0, frequency 0
    edges_case(12, 0.0, 0.5, 0.5, 0.3, frequency=5),                                            # set_scene_change_freq: the modulo rule
    edges_case(12, 0.05, 0.5, 0.5, 0.3, frequency=1),                                           # ... every frame
]
edges[6]["scd"][4990:5012] = (rng.uniform(0, 1, 22) < 0.5).astype(np.int8)                      # candidates on both sides of the batch border


def filter_case(n, density, ssim_tht, min_length, frequency=0, chunk=16, tht_white=0.70, tht_black=0.10, debug=False, dark=0.25):
    prev = (rng.uniform(0, 1, n) < density).astype(np.int8)
    return dict(prev=prev, luma=lumas(n, dark, 0.1), reason=rng.integers(0, 5, n).astype(np.int8), ssim_tht=ssim_tht, min_length=min_length,
                frequency=frequency, chunk=chunk, tht_white=tht_white, tht_black=tht_black, debug=debug)


filters = [
    filter_case(64, 0.6, 0.80, 7),                                  # what SceneDetectEdges' defaults give: min_length = round(20 / 3)
    filter_case(64, 0.7, 0.60, 1, debug=True),
    filter_case(64, 0.6, 0.75, 5, frequency=25, dark=0.45),         # the frequency override: luma alone, no ratio term
    filter_case(64, 0.8, 1.0, 6),
    filter_case(48, 0.9, 0.35, 25, chunk=7, dark=0.5, debug=True),
    filter_case(5040, 0.02, 0.60, 10, chunk=5000),                  # through SceneDetectFilter itself
]
filters[0]["reason"][0] = 1                                        # _sc_prev_reason < 2: the reason override is open for the whole case
filters[1]["reason"][0] = 3                                        # ... and closed
filters[-1]["prev"][4985:5015] = (rng.uniform(0, 1, 30) < 0.7).astype(np.int8)
filters[-1]["luma"][4985:5015] = lumas(30, dark=0.5)
filters[-1]["reason"][0] = 0

fx = {"provenance": np.array("generated by tools/gen_golden_scedges.py executing the reference: vsslib/vsscdetect_edge.py SceneDetectEdges, "
                             "vs_edge_based_scenedetect (selector body set_sc_prop included) and SceneDetectionFiltered (set_scenechange included), on "
                             "prescribed statistics and recorded scores"),
      "ssim_table": ssim_table, "hist_table": hist_table, "key": np.array([K, A, B], np.int64), "n_pixels": np.array(NP),
      "n_edges": np.array(len(edges)), "n_filter": np.array(len(filters))}
for i, c in enumerate(edges):
    calls.clear()
    out = run_edges(c)
    n = len(c["planes"])
    assert [f.src for f in out] == list(range(n))
    fx[f"edges_{i}_params"] = np.array(json.dumps(c["kw"]))
    fx[f"edges_{i}_sum_y"] = np.array([int(p.sum(dtype=np.int64)) for p in c["planes"]], np.int64)
    fx[f"edges_{i}_scd"], fx[f"edges_{i}_sum_masked"], fx[f"edges_{i}_sad_next"] = c["scd"], c["sum_masked"], c["sad_next"]
    fx[f"edges_{i}_prev"] = np.array([f.props.get("_SceneChangePrev", 0) for f in out], np.int8)
    fx[f"edges_{i}_next"] = np.array([f.props.get("_SceneChangeNext", 0) for f in out], np.int8)
    fx[f"edges_{i}_has_props"] = np.array(["_SceneChangePrev" in out[0].props, "sc_luma" in out[0].props, "sc_reason" in out[0].props])
    fx[f"edges_{i}_luma"] = np.array([f.props.get("sc_luma", 0.0) for f in out], np.float64)
    fx[f"edges_{i}_reason"] = np.array([f.props.get("sc_reason", 0) for f in out], np.int8)
    fx[f"edges_{i}_pairs"] = np.array(calls, np.int64).reshape(-1, 2)
    fx[f"edges_{i}_next_index"] = np.array(c.get("next_index", []), np.int64)
    assert all(f.props["sc_threshold"] == c["kw"]["threshold"] and f.props["sc_frequency"] == c["kw"].get("frequency", 0) for f in out)
    print("edges", i, "flags", int(fx[f"edges_{i}_prev"].sum()), "reasons", np.bincount(fx[f"edges_{i}_reason"], minlength=5).tolist(), "scored", len(calls))
for i, c in enumerate(filters):
    calls.clear()
    out = run_filter(c)
    assert [f.src for f in out] == list(range(len(c["prev"])))
    fx[f"filter_{i}_in_prev"], fx[f"filter_{i}_luma"], fx[f"filter_{i}_reason"] = c["prev"], c["luma"], c["reason"]
    fx[f"filter_{i}_params"] = np.array(json.dumps({k: c[k] for k in ("ssim_tht", "min_length", "frequency", "chunk", "tht_white", "tht_black")}))
    fx[f"filter_{i}_prev"] = np.array([f.props["_SceneChangePrev"] for f in out], np.int8)
    fx[f"filter_{i}_next"] = np.array([f.props["_SceneChangeNext"] for f in out], np.int8)
    fx[f"filter_{i}_pairs"] = np.array(calls, np.int64).reshape(-1, 2)
    assert all(f.props["sc_luma"] == l and f.props["sc_reason"] == r for f, l, r in zip(out, c["luma"], c["reason"]))      # the filter leaves both alone
    print("filter", i, "candidates", int(c["prev"].sum()), "kept", int(fx[f"filter_{i}_prev"].sum()), "scored", len(calls))


def both_ways(h, table, what):
    """a line is hit when its statement starts: a branch was taken when the first line of its body was hit, and refused when the test was hit more often"""
    for test, body in table.items():
        assert h[body] > 0, f"{what}: the branch of line {test} was never taken"
        assert h[test] > h[body], f"{what}: the branch of line {test} was never refused"


# line numbers of vsslib/vsscdetect_edge.py
d = hits["set_sc_prop"]
both_ways(d, {191: 192, 220: 221, 221: 222, 222: 223, 225: 226, 234: 235, 235: 236, 244: 245, 255: 256}, "set_sc_prop")
assert d[229] > 0 and d[233] > 0 and d[242] > 0 and d[251] > 0 and d[253] > 0               # every else: reason 3, both "Skipped" forms, the last one, "Rejected"
f = hits["set_scenechange"]
both_ways(f, {384: 385, 393: 394, 401: 402, 407: 408, 412: 413, 413: 414, 414: 415, 426: 427, 435: 437, 438: 439, 441: 442, 444: 446, 448: 449, 459: 460,
              460: 461, 472: 473}, "set_scenechange")
assert f[422] > 0 and f[432] > 0 and f[452] > 0 and f[477] > 0                              # the else of :413, the elif of :431, the final else, the rejection
assert f[455] == 0                                                                          # :431 cannot be false
# what the cases must reach
allr = np.concatenate([fx[f"edges_{i}_reason"][1:] for i in (0, 2)])
assert set(np.unique(allr)) == {0, 1, 2, 3, 4}
lum = np.concatenate([fx[f"edges_{i}_luma"] for i in (0, 2)])
assert (lum < 0.10).any() and (lum > 0.70).any()                                            # "Rejected" for a dark and for a bright frame
assert len(fx["edges_6_pairs"]) and fx["edges_6_pairs"][:, 0].min() < 5000 <= fx["edges_6_pairs"][:, 0].max()       # a chunk boundary
np.savez_compressed(os.path.join(ROOT, "tests", "golden", "scdetect_edges.npz"), **fx)
print("wrote scdetect_edges.npz;", os.path.getsize(os.path.join(ROOT, "tests", "golden", "scdetect_edges.npz")), "bytes")
