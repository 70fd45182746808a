#!/usr/bin/env python3
"""havc_equalize_clip (csrc/equalize.hip) on a device-resident 1080p clip: rgb_equalizer methods 0-3 and HAVC_bw_tune's default call, in frames/s, next to
the time a plain device-to-device copy needs for the bytes the call must move.  Needs an MI355X.

    python tools/equalize_bench.py [--frames 32] [--reps 20] [--out profiles/equalize.txt]

Method: the clip stays in HBM and the call only enqueues, so `reps` calls are enqueued back to back and the host clock is read around them and a stream
synchronise, after 3 warm-up calls; that is repeated 5 times and the median taken (min and max next to it).  Bytes that must move: the histogram pass
reads the clip, the apply pass reads it again and writes the result -- two reads and one write; with rgb_balance (HAVC_bw_tune) the channel sums read it
once more.  The copy leg moves the clip once (one read, one write) with havc_dev_copy, timed the same way; "copy bound" is the time that copy rate needs
for the call's bytes, and the last column is copy bound / call time.  The comparison points of the reference are its own comments (havc_utils.py:798-803):
41.5 / 54.5 / 37.5 / 34.5 frames/s for methods 0 / 1 / 2 / 3 with cv2 on the CPU, frame size not stated.
The output of every timed method is compared with tests/equalize_util.py's numpy restatement on the first two frames before anything is timed."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import equalize_util as U  # noqa: E402
from vsdeoldify_amd import equalize as EQ  # noqa: E402
from vsdeoldify_amd import havc  # noqa: E402
from vsdeoldify_amd.device import DeviceImage  # noqa: E402
from vsdeoldify_amd.render import get_context  # noqa: E402

REFERENCE_FPS = {0: 41.5, 1: 54.5, 2: 37.5, 3: 34.5}


def make_clip(n, h, w, seed=3):
    """frames inside the gate (levels 90..150), smooth ramps plus noise: every frame does the full work"""
    r = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    clip = np.empty((n, h, w, 3), np.uint8)
    for i in range(n):
        base = 90 + 60 * i / max(n - 1, 1) + 50 * (xx / w - 0.5) + 30 * (yy / h - 0.5)
        clip[i] = np.clip(base[:, :, None] + r.integers(-25, 26, (h, w, 3)), 0, 255)
    return clip


def timed(ctx, fn, reps, rounds=5):
    for _ in range(3):
        fn()
    ctx.synchronize()
    v = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        ctx.synchronize()
        v.append((time.perf_counter() - t0) * 1e3 / reps)
    return v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = get_context(0)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    n, h, w = a.frames, 1080, 1920
    clip = make_clip(n, h, w)
    dclip = DeviceImage.from_numpy(ctx, clip)
    dcopy = DeviceImage(ctx, clip.shape)
    say(f"histogram equalisation of a device-resident clip {n} x {h} x {w} ({clip.nbytes / 1e6:.1f} MB); device {ctx.device_name()}")
    say(f"median of 5 windows of {a.reps} enqueued calls + one synchronise, host clock, after 3 warm-up calls")
    v = timed(ctx, lambda: dcopy.copy_from(dclip), a.reps)
    copy_ms = statistics.median(v)
    copy_gbs = 2 * clip.nbytes / copy_ms / 1e6
    say(f"  device copy of the clip (1 read + 1 write)   {copy_ms:8.3f} ms  (min {min(v):.3f}, max {max(v):.3f})   {copy_gbs:6.0f} GB/s")
    ok = True
    legs = [(f"rgb_equalizer method {m}", m, 3, lambda m=m: EQ.rgb_equalizer_np(ctx, dclip, m, 1.0, 8, 0.98, 0.3, True, True),
             lambda c, m=m: U.rgb_equalizer(c, m, 1.0, 0.98, 0.3, True, True)) for m in range(4)]
    legs.append(("HAVC_bw_tune('Light', 0)", 0, 4, lambda: havc.HAVC_bw_tune(dclip), lambda c: U.bw_tune(c)))
    for name, m, passes, fn, ref in legs:
        same = bool(np.array_equal(fn().numpy()[:2], ref(clip[:2])))
        ok &= same
        v = timed(ctx, fn, a.reps)
        ms = statistics.median(v)
        bound = passes * clip.nbytes / (copy_gbs * 1e6)
        say(f"  {name:28s} {ms:8.3f} ms  (min {min(v):.3f}, max {max(v):.3f})   {n / ms * 1e3:8.0f} frames/s   (reference, cv2 on the CPU: "
            f"{REFERENCE_FPS[m]} frames/s)   {passes} passes = {passes * clip.nbytes / 1e6:.0f} MB: copy bound {bound:.3f} ms = {100 * bound / ms:5.1f} % of the call"
            f"   == numpy: {same}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if not ok:
        raise SystemExit("the kernels and the numpy restatement disagree")


if __name__ == "__main__":
    main()
