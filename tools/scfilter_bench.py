#!/usr/bin/env python3
"""Scene detection WITH the SSIM / histogram post-filter (scdetect.scene_detect_filtered: Spline64 to the 480-line clip, havc_scene_stats, havc_scene_hist,
havc_scene_ssim, the selector on the host) on a device-resident 1080p clip, at two candidate densities, and the accuracy of havc_scene_ssim against the
numpy restatement over the shapes of tests/test_gpu_scfilter.py.  Needs an MI355X.

    python tools/scfilter_bench.py [--frames 96] [--reps 10] [--out profiles/scene_filter.txt]

Method: the clip is scenes of seeded blocky texture that drift sideways by a pixel per frame, `cut` frames each (every scene start is a candidate of stage
1; a short `cut` = dense candidates).  One call = scene_detect_filtered(sc_tht_filter 0.60, min_length 10) from the DeviceImage to the SceneInfo in host
memory, timed on the host clock after 2 warm-up calls; the figure is the median over `reps` calls.  Next to it the copy bound: the bytes the kernels must
read and write once -- the 1080p clip in and the small clip out (resize), the small clip (statistics), one small frame per candidate (histogram), two
per pair (SSIM; the tile halos and the statistics' compared frame are re-reads that caches may serve) -- at the 8 TB/s HBM3E peak profiles/scene_stats.txt
uses.  The call also holds what no byte count shows: its launches, a blocking download behind the statistics, the histogram and every SSIM call, and
the host selector."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import scfilter_util as U  # noqa: E402
from vsdeoldify_amd import scdetect as SD  # noqa: E402
from vsdeoldify_amd.device import DeviceImage  # noqa: E402
from vsdeoldify_amd.render import get_context  # noqa: E402

PEAK_GBS = 8000.0


def make_clip(n, h, w, cut, seed=1):
    r = np.random.default_rng(seed)
    clip = np.empty((n, h, w, 3), np.uint8)
    for s in range(0, n, cut):
        tex = np.kron(r.integers(-70, 71, (h // 8, w // 8 + 8, 1)), np.ones((8, 8, 1), np.int64)).repeat(3, 2) + int(r.integers(70, 180))
        for k in range(min(cut, n - s)):
            clip[s + k] = np.clip(tex[:, k:k + w], 0, 255)
    return clip


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=96)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = get_context(0)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"havc_scene_ssim against the numpy restatement (integer window sums, float64), device {ctx.device_name()}")
    worst = 0.0
    for h, w in U.SHAPES + [(480, 852)]:
        clip, pairs = U.kernel_clip(h, w)
        g = U.gray(clip)
        err = np.abs(SD.scene_ssim(ctx, clip, pairs) - np.array([U.ssim_np(g[x], g[y]) for x, y in pairs])).max()
        worst = max(worst, float(err))
        say(f"  {h:4d} x {w:4d}: max |gpu - numpy| over {len(pairs)} pairs = {err:.3e}")
    say(f"  maximum over all shapes: {worst:.3e} (tests/test_gpu_scfilter.py bounds it by 1e-9)")
    say()
    n, h, w = a.frames, 1080, 1920
    tw, th = SD.resize_min_hw(w, h)
    say(f"detect + filter on a device-resident clip {n} x {h} x {w} ({n * h * w * 3 / 1e6:.0f} MB), small clip {th} x {tw}; sc_tht_ssim 0.60, sc_min_int 10")
    say(f"median of {a.reps} blocking calls on the host clock after 2 warm-up calls")
    for cut in (24, 3):
        dclip = DeviceImage.from_numpy(ctx, make_clip(n, h, w, cut))
        dbg = {}

        def call():
            return SD.scene_detect_filtered(ctx, dclip, sc_tht_filter=0.60, min_length=10, debug=dbg)

        for _ in range(2):
            info = call()
        v = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            call()
            v.append((time.perf_counter() - t0) * 1e3)
        ms = statistics.median(v)
        k = len(dbg["candidates"])
        pairs = k - 1 + dbg["fallback_launches"]
        small = th * tw * 3
        must = n * h * w * 3 + n * small + n * small + k * small + 2 * pairs * small
        bound_ms = must / PEAK_GBS / 1e6
        say(f"a cut every {cut} frames: {k} candidates of {n} frames, {int(info.scene_change_prev.sum())} kept, {dbg['fallback_launches']} one-pair launches")
        say(f"  {ms:9.3f} ms per call (min {min(v):.3f}, max {max(v):.3f}) = {n / ms * 1e3:9.0f} frames/s")
        say(f"  copy bound: {must / 1e6:.0f} MB at {PEAK_GBS / 1000:.0f} TB/s = {bound_ms:.3f} ms = {n / bound_ms * 1e3:9.0f} frames/s; the call runs at "
            f"{100 * bound_ms / ms:.1f} % of it")
        del dclip
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
