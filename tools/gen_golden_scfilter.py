#!/usr/bin/env python3
"""Golden vectors for the scene filter (vsslib/vsscdect.py:352-495) by EXECUTING the reference (build container only).  Writes tests/golden/scfilter.npz
(data only).

Every case drives the reference's own _scene_detect_filter_task -- selector body (set_scenechange, :380-483) included -- frame by frame in order over a
stand-in clip whose frames carry the props stage 1 leaves (_SceneChangePrev / _SceneChangeNext / sc_luma / sc_ratio) and, as their "pixels", nothing but
their own frame number.  The pixel functions are stand-ins that return RECORDED scores, which are inputs of the fixture (as the equalised plane is in
equalize.npz): cv2.cvtColor / split / calcHist / normalize hand the frame number on, and

    skimage.metrics.structural_similarity(frame t_n, frame last)        -> ssim_table[(A * t_n + B * last) % K]         a numpy float64, as skimage's
    cv2.compareHist(hist of frame last, hist of frame t_n, HELLINGER)   -> hist_table[(A * t_n + B * last) % K]         a Python float, as cv2's

so the flags depend on WHICH accepted frame the selector compares with (its carried state), not only on the candidate.  Cases 0..n-2 are cut into chunks of
`chunk` frames, each handed to _scene_detect_filter_task with its t_start as SceneDetectFilter does (:358-363), on one SceneDetection object; the last case
goes through SceneDetectFilter itself with more than its 5000-frame batch.  Line tracing of the selector asserts that every `if` / `elif` of :417-460 went
both ways (the `elif n < clip.num_frames` of :436 cannot be false: n is a frame number of that clip).
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

K, A, B = 997, 7, 13
rng = np.random.default_rng(20261019)
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
plug.load_MVTool_plugin = plug.load_SCDetect_plugin = lambda *a, **k: None
sys.modules["vsdeoldify.vsslib.vsplugins"] = plug
sd = importlib.import_module("vsdeoldify.vsslib.vsscdect")


class Frame:
    """three 1 x 1 planes that hold the frame's number + props: the part of vs.VideoFrame the selector touches"""
    format = types.SimpleNamespace(num_planes=3)

    def __init__(self, number, props):
        self.number, self.props = number, dict(props)

    def __getitem__(self, plane):
        return np.full((1, 1), self.number, np.int64)

    def copy(self):
        return Frame(self.number, self.props)


class Clip:
    """a list of frames; std.ModifyFrame(clips, selector) evaluates the selector on every frame IN ORDER (the filter carries state from frame to frame)"""
    def __init__(self, frames):
        self.frames, self.num_frames = list(frames), len(frames)
        self.std = types.SimpleNamespace(ModifyFrame=self._modify)

    def __getitem__(self, s):
        return Clip(self.frames[s])

    def _modify(self, clips, selector):
        assert len(clips) == 1
        return Clip([selector(n, f) for n, f in enumerate(clips[0].frames)])


vs.core.std = types.SimpleNamespace(Splice=lambda clips: Clip([f for c in clips for f in c.frames]))

hits = collections.Counter()
REF_FILE = sd.__file__


def tracer(frame, event, arg):
    if frame.f_code.co_name != "set_scenechange" or frame.f_code.co_filename != REF_FILE:
        return None

    def lines(frame, event, arg):
        if event == "line":
            hits[frame.f_lineno] += 1
        return lines
    return lines


def run(case):
    frames = [Frame(i, {"_SceneChangePrev": int(p), "_SceneChangeNext": 0, "sc_luma": float(l), "sc_ratio": float(r)})
              for i, (p, l, r) in enumerate(zip(case["prev"], case["luma"], case["ratio"]))]
    det = sd.SceneDetection(sc_frequency=case["frequency"], sc_tht_white=case["tht_white"], sc_tht_black=case["tht_black"])
    sys.settrace(tracer)
    try:
        if case["chunk"] == 5000:
            out = det.SceneDetectFilter(Clip(frames), ssim_threshold=case["ssim_tht"], min_length=case["min_length"]).frames
        else:
            out = []
            for t_start in range(0, len(frames), case["chunk"]):
                cut = Clip(frames[t_start:t_start + case["chunk"]])
                out += det._scene_detect_filter_task(t_start, cut, case["ssim_tht"], case["min_length"]).frames
    finally:
        sys.settrace(None)
    return out


def lumas(n, dark=0.25, white=0.1):
    """4-decimal lumas: mostly mid-gray, some in the dark band (0.05 .. 0.19: both sides of tht_black) and some beyond tht_white"""
    u = rng.uniform(0, 1, n)
    l = np.where(u < dark, rng.uniform(0.05, 0.19, n), np.where(u > 1 - white, rng.uniform(0.66, 0.95, n), rng.uniform(0.19, 0.66, n)))
    return np.round(l, 4)


def case(n, density, ssim_tht, min_length, frequency=0, chunk=16, tht_white=0.70, tht_black=0.10, **kw):
    prev = (rng.uniform(0, 1, n) < density).astype(np.int8)
    ratio = np.round(np.where(rng.uniform(0, 1, n) < 0.5, rng.uniform(0.2, 2.0, n), rng.uniform(2.0, 20.0, n)), 4)
    return dict(prev=prev, luma=lumas(n, **kw), ratio=ratio, ssim_tht=ssim_tht, min_length=min_length, frequency=frequency, chunk=chunk, tht_white=tht_white,
                tht_black=tht_black)


cases = [
    case(64, 0.6, 0.60, 10),                                    # the documented best settings; chunks of 16: candidates at chunk-local n = 0 and 1
    case(64, 0.7, 0.60, 1),                                     # no minimum interval: every candidate is scored
    case(64, 0.6, 0.75, 5, frequency=25, dark=0.45),            # the frequency override on dark frames with small ratios
    case(64, 0.8, 1.0, 6),                                      # ssim threshold 1 with a minimum interval: luma decides, no score is taken
    case(48, 0.9, 0.35, 25, chunk=7, dark=0.5),                 # long interval, short chunks: the chunk-local n rules against the global t_n
    case(64, 0.7, 0.85, 3, tht_white=0.88, tht_black=0.12, dark=0.4),
    case(5040, 0.02, 0.60, 10, chunk=5000),                     # through SceneDetectFilter itself: its own 5000-frame batches
]
cases[-1]["prev"][4985:5015] = (rng.uniform(0, 1, 30) < 0.7).astype(np.int8)            # candidates on both sides of the batch border
cases[-1]["luma"][4985:5015] = lumas(30, dark=0.5)

fx = {"provenance": np.array("generated by tools/gen_golden_scfilter.py executing the reference: vsslib/vsscdect.py SceneDetection._scene_detect_filter_task "
                             "(selector body set_scenechange included) and SceneDetectFilter, on recorded scores"),
      "ssim_table": ssim_table, "hist_table": hist_table, "key": np.array([K, A, B], np.int64), "n_cases": np.array(len(cases))}
for i, c in enumerate(cases):
    calls.clear()
    out = run(c)
    assert [f.number for f in out] == list(range(len(c["prev"])))
    fx[f"case_{i}_in_prev"], fx[f"case_{i}_luma"], fx[f"case_{i}_ratio"] = c["prev"], c["luma"], c["ratio"]
    fx[f"case_{i}_params"] = np.array(json.dumps({k: c[k] for k in ("ssim_tht", "min_length", "frequency", "chunk", "tht_white", "tht_black")}))
    fx[f"case_{i}_prev"] = np.array([f.props["_SceneChangePrev"] for f in out], np.int8)
    fx[f"case_{i}_next"] = np.array([f.props["_SceneChangeNext"] for f in out], np.int8)
    fx[f"case_{i}_pairs"] = np.array(calls, np.int64).reshape(-1, 2)                     # (frame, last accepted frame) of every score the selector took
    print(i, "candidates", int(c["prev"].sum()), "kept", int(fx[f"case_{i}_prev"].sum()), "scored", len(calls))

# every `if` / `elif` of :417-460 went both ways (line numbers of vsslib/vsscdect.py).  A line is hit when its statement starts: a branch was taken when the
# first line of its body was hit, and refused when the test was hit more often than the body.
both = {417: 418, 418: 423, 431: 432, 440: 441, 443: 444, 447: 449, 451: 452}
for test, body in both.items():
    assert hits[body] > 0, f"the branch of line {test} was never taken"
    assert hits[test] > hits[body], f"the branch of line {test} was never refused"
assert hits[427] > 0 and hits[436] > 0 and hits[455] > 0                                  # the else of :418, the elif of :431 and the final else
assert hits[458] == 0                                                                     # :436 cannot be false
assert hits[468] > 0 and hits[480] > 0                                                    # both outcomes of the decision itself
np.savez_compressed(os.path.join(ROOT, "tests", "golden", "scfilter.npz"), **fx)
print("wrote scfilter.npz;", {k: hits[k] for k in sorted(hits) if 415 <= k <= 462})
