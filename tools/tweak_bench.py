#!/usr/bin/env python3
"""HAVC_tweak and HAVC_adjust_rgb on a device-resident 1080p clip, the two halves of the YUV420 round trip on their own, and HAVC_bw_tune on the same clip in
the same run as the existing per-pixel filter to compare against.  Needs an MI355X.

    python tools/tweak_bench.py [--frames 64] [--reps 10] [--out profiles/tweak.txt]

Method: the clip is smooth colour (sines per channel) plus noise, so the error diffusion sees fractions everywhere.  Every operand lives in device memory, so a
call only enqueues: each timed call ends in a device synchronise, and every figure is the median over `reps` such calls on the host clock after 2 warm-up
calls (min and max beside it).  Frames / s = frames of the clip over that time: an end-to-end rate of the call, not a kernel's share of peak.
  * HAVC_tweak(hue, sat, bright, cont, gamma): everything on = forward launch + back launch per chunk (one chunk here);
  * havc_rgb_to_yuv420 / havc_yuv420_to_rgb alone, on device planes;
  * HAVC_adjust_rgb(strength 0.5, gains, biases, gammas): channel sums, tables, one pass; and with strength 0 (no sums);
  * HAVC_bw_tune('Light'): the yardstick, three launches over the clip.
Bytes that must move: forward reads 3 and writes 1.5 bytes per pixel, back reads 1.5 and writes 3, adjust_rgb reads 3 (twice with the sums) and writes 3; the
bound beside each figure is those bytes at the 8 TB/s HBM3E peak the other profiles use.  The first frame of the result is checked against the numpy
definition before anything is timed."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vsdeoldify_amd import _native as nat  # noqa: E402
from vsdeoldify_amd import havc  # noqa: E402
from vsdeoldify_amd.device import DeviceImage  # noqa: E402
from vsdeoldify_amd.render import get_context  # noqa: E402

PEAK_GBS = 8000.0


def make_clip(n, h, w, seed=1):
    r = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    clip = np.empty((n, h, w, 3), np.uint8)
    for k in range(n):
        base = np.stack([120 + 70 * np.sin(x / 61 + 0.1 * k), 110 + 60 * np.cos(y / 43 - 0.07 * k), 100 + 50 * np.sin((x + y) / 97 + 0.05 * k)], -1)
        clip[k] = np.clip(base + r.normal(0.0, 6.0, (h, w, 3)).astype(np.float32), 0, 255)
    return clip


def median_ms(ctx, call, reps):
    def once():
        call()
        ctx.synchronize()
    for _ in range(2):
        once()
    v = []
    for _ in range(reps):
        t0 = time.perf_counter()
        once()
        v.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(v), min(v), max(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = get_context(0)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    n, h, w = a.frames, a.height, a.width
    npix = n * h * w
    clip = make_clip(n, h, w)
    dclip = DeviceImage.from_numpy(ctx, clip)
    say(f"HAVC_tweak / HAVC_adjust_rgb on a device-resident clip {n} x {h} x {w} ({npix * 3 / 1e6:.0f} MB), device {ctx.device_name()}")
    say(f"median of {a.reps} calls, each ended by a device synchronise, on the host clock after 2 warm-up calls")

    def report(name, ms, lo, hi, must):
        bound = must / PEAK_GBS / 1e6
        say(f"{name:<58s} {ms:9.3f} ms per call (min {lo:.3f}, max {hi:.3f}) = {n / ms * 1e3:9.0f} frames/s; bytes bound {must / 1e6:.0f} MB = "
            f"{bound:.3f} ms, the call takes {ms / bound:.1f} x that")

    kw = dict(hue=12.0, sat=1.2, bright=8.0, cont=1.1, gamma=1.1)
    got = havc.HAVC_tweak(dclip, **kw).numpy()
    from tests import tweak_util as U
    rows = 66                                                   # the first 66 rows depend on nothing below row 66 + 4
    want = U.tweak(clip[:1, :rows + 6], **kw)
    assert np.array_equal(got[0, :rows - 2], want[0, :rows - 2]), "HAVC_tweak does not equal the definition"
    say("the first 64 rows of frame 0 equal the numpy definition byte for byte")
    ms, lo, hi = median_ms(ctx, lambda: havc.HAVC_tweak(dclip, **kw), a.reps)
    report("HAVC_tweak (hue, sat, bright, cont, gamma)", ms, lo, hi, npix * 9)
    t_tweak = ms

    planes = [ctx.dev_alloc(npix), ctx.dev_alloc(npix // 4), ctx.dev_alloc(npix // 4)]
    out = DeviceImage(ctx, clip.shape)
    fwd = lambda: nat.check(ctx.lib.havc_rgb_to_yuv420(ctx.h, dclip.ptr, planes[0], planes[1], planes[2], w, h, n), ctx.h)
    back = lambda: nat.check(ctx.lib.havc_yuv420_to_rgb(ctx.h, planes[0], planes[1], planes[2], out.ptr, w, h, n), ctx.h)
    ms_f, lo, hi = median_ms(ctx, fwd, a.reps)
    report("havc_rgb_to_yuv420 alone (tweak_forward_kernel)", ms_f, lo, hi, npix * 4.5)
    ms_b, lo, hi = median_ms(ctx, back, a.reps)
    report("havc_yuv420_to_rgb alone (tweak_back_kernel)", ms_b, lo, hi, npix * 4.5)
    say(f"  back / forward = {ms_b / ms_f:.1f}; forward + back = {ms_f + ms_b:.3f} ms against {t_tweak:.3f} ms for HAVC_tweak")
    for p in planes:
        ctx.dev_free(p)

    adj = dict(factor=(1.1, 0.95, 1.05), bias=(4, -3, 2), gamma=(1.1, 1.0, 0.9))
    ms, lo, hi = median_ms(ctx, lambda: havc.HAVC_adjust_rgb(dclip, 0.5, **adj), a.reps)
    report("HAVC_adjust_rgb (strength 0.5: sums, tables, one pass)", ms, lo, hi, npix * 9)
    ms, lo, hi = median_ms(ctx, lambda: havc.HAVC_adjust_rgb(dclip, 0.0, **adj), a.reps)
    report("HAVC_adjust_rgb (strength 0: tables, one pass)", ms, lo, hi, npix * 6)
    ms, lo, hi = median_ms(ctx, lambda: havc.HAVC_bw_tune(dclip, 'Light'), a.reps)
    report("HAVC_bw_tune('Light') on the same clip (the yardstick)", ms, lo, hi, npix * 12)
    say(f"  HAVC_tweak takes {t_tweak / ms:.2f} x HAVC_bw_tune's time")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
