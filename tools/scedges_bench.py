#!/usr/bin/env python3
"""HAVC_SceneDetectEdges on a device-resident 1080p clip end to end, the edge-statistics launch alone on the small clip, havc_scene_stats on the same small
clip as the yardstick, and the bytes-read bound.  Needs an MI355X.

    python tools/scedges_bench.py [--frames 48] [--reps 10] [--out profiles/scene_edges.txt]

Method: the clip is scenes of 110 + 60 sin(x / px + f) + 40 cos(y / py - f) + noise (tests/scedges_util.py's recipe) with a cut every 12 frames and a slow
drift inside a scene.  Every figure is the median over `reps` blocking calls on the host clock after 2 warm-up calls.
  * end to end: HAVC_SceneDetectEdges(DeviceImage) with its defaults -- Spline64 to 854 x 480, one havc_scene_edge_stats launch, the detector on the host, then
    the SSIM / histogram filter's launches over the candidates -- to the EdgeSceneInfo in host memory;
  * statistics alone: scdetect_edge.edge_stats on the device-resident 854 x 480 clip = the launch plus the download of 32 bytes per frame;
  * yardstick: scdetect.scene_stats (havc_scene_stats, offset 2) on the same clip, same machine, same clock;
  * bound: a frame's statistics need its own RGB bytes and those of the two frames it is compared with: three RGB frames per output frame at the 8 TB/s HBM3E
    peak profiles/scene_stats.txt uses.  The halo re-reads of the tiles are served by caches or not; they are not in the bound."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import scedges_util as U  # noqa: E402
from vsdeoldify_amd import havc  # noqa: E402
from vsdeoldify_amd import scdetect as SD  # noqa: E402
from vsdeoldify_amd import scdetect_edge as SE  # noqa: E402
from vsdeoldify_amd.device import DeviceImage  # noqa: E402
from vsdeoldify_amd.render import get_context  # noqa: E402

PEAK_GBS = 8000.0


def make_clip(n, h, w, cut=12, seed=1):
    r = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    clip = np.empty((n, h, w, 3), np.uint8)
    for s in range(0, n, cut):
        level, px, py = float(r.integers(70, 160)), float(r.integers(9, 40)), float(r.integers(7, 30))
        for k in range(min(cut, n - s)):
            v = level + 60 * np.sin(x / px + 0.02 * k) + 40 * np.cos(y / py - 0.02 * k) + r.normal(0.0, 2.0, (h, w)).astype(np.float32)
            clip[s + k] = np.clip(np.rint(v[..., None] + np.array([0.0, 3.0, -5.0], np.float32)), 0, 255)
    return clip


def median_ms(call, reps):
    for _ in range(2):
        call()
    v = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        v.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(v), min(v), max(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = get_context(0)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    n, h, w = a.frames, 1080, 1920
    tw, th = SD.resize_min_hw(w, h)
    clip = make_clip(n, h, w)
    dclip = DeviceImage.from_numpy(ctx, clip)
    say(f"HAVC_SceneDetectEdges on a device-resident clip {n} x {h} x {w} ({n * h * w * 3 / 1e6:.0f} MB), small clip {th} x {tw}, device {ctx.device_name()}")
    say(f"median of {a.reps} blocking calls on the host clock after 2 warm-up calls")
    info = havc.HAVC_SceneDetectEdges(dclip)
    ms, lo, hi = median_ms(lambda: havc.HAVC_SceneDetectEdges(dclip), a.reps)
    say(f"end to end (defaults: filter on): {ms:9.3f} ms per call (min {lo:.3f}, max {hi:.3f}) = {n / ms * 1e3:9.0f} frames/s; flags at "
        f"{np.flatnonzero(info.scene_change_prev).tolist()}")
    ms, lo, hi = median_ms(lambda: havc.HAVC_SceneDetectEdges(dclip, sc_tht_ssim=0), a.reps)
    say(f"end to end (sc_tht_ssim = 0):     {ms:9.3f} ms per call (min {lo:.3f}, max {hi:.3f}) = {n / ms * 1e3:9.0f} frames/s")
    small = havc.spline64(ctx, dclip, tw, th)
    del dclip
    small_np = small.numpy()
    rec, tap = SE.edge_stats(ctx, small, 2, mask_tap=True)
    want, mask = U.edge_stats_np(small_np[:4], 2)
    assert tap[:3].tobytes() == mask[:3].tobytes() and all(np.array_equal(rec[k][:2], want[k][:2]) for k in want), "the launch does not equal the definition"
    say(f"mask of the small clip: mean {tap.mean():.1f}, {100 * ((tap == 0) | (tap == 255)).mean():.1f} % of the pixels at 0 or 255; the first frames equal "
        f"the numpy definition byte for byte")
    ms, lo, hi = median_ms(lambda: SE.edge_stats(ctx, small, 2), a.reps)
    must = 3 * n * th * tw * 3
    bound_ms = must / PEAK_GBS / 1e6
    say(f"havc_scene_edge_stats alone, {n} x {th} x {tw}, offset 2, sigma 1.2: {ms:9.3f} ms per call (min {lo:.3f}, max {hi:.3f}) = {n / ms * 1e3:9.0f} frames/s")
    say(f"  bytes-read bound: three RGB frames per frame = {must / 1e6:.0f} MB at {PEAK_GBS / 1000:.0f} TB/s = {bound_ms:.4f} ms; the call takes "
        f"{ms / bound_ms:.1f} x that")
    ms2, lo, hi = median_ms(lambda: SD.scene_stats(ctx, small, 2), a.reps)
    say(f"havc_scene_stats on the same clip (the yardstick: two RGB frames per frame, no stencil): {ms2:9.3f} ms per call (min {lo:.3f}, max {hi:.3f}) = "
        f"{n / ms2 * 1e3:9.0f} frames/s; the edge statistics take {ms / ms2:.2f} x its time")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
