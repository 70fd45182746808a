#!/usr/bin/env python3
"""HAVC_stabilizer(stab=True) on a device-resident 1080p clip, its temporal stage on its own at the filters' size, and -- in the same run -- what it is made of
and what it sits next to: the dark + smooth + colormap launch and the two YUV420 conversions alone.  Needs an MI355X.

    python tools/chroma_stab_bench.py [--frames 64] [--reps 10] [--out profiles/chroma_stab.txt]

Method: the clip is smooth colour (sines per channel, drifting from frame to frame) plus noise.  Every operand lives in device memory, so a call only
enqueues: each timed call ends in a device synchronise, and every figure is the median over `reps` such calls on the host clock after 2 warm-up calls (min
and max beside it).  Frames / s = frames of the clip over that time: an end-to-end rate of the call, not a kernel's share of peak.  render_factor 24: the
filters run at 384 x 384.
  * HAVC_stabilizer(dark, smooth, colormap, stab) with the default stab_p (5, 'A', 1, 15, 0.2, 0.8), with N = 15, and without stab;
  * the stab stage alone at 384 x 384 (havc_chroma_stab_clip): N = 5 and 15 with tht = 15, N = 5 with tht = 0, each with the flicker pass, and N = 5 without;
  * the dark + smooth + colormap launch alone (havc_stabilizer_chain), havc_rgb_to_yuv420 and havc_yuv420_to_rgb alone on the clip's frames, and the back
    conversion on (N - 1) times as many frames: what the shifted clips of vs_get_clip_frame cost;
  * the flicker pass alone (havc_reduce_flicker_clip).
The kernels' own times come from a separate run under a kernel trace (appended to the profile by hand).  The first frames of the stab stage are checked
against the numpy definition before anything is timed."""
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
from vsdeoldify_amd import chroma_stab as CS  # noqa: E402
from vsdeoldify_amd import havc  # noqa: E402
from vsdeoldify_amd.device import DeviceImage  # noqa: E402
from vsdeoldify_amd.render import get_context  # noqa: E402
from vsdeoldify_amd.stabilizer import stabilize_np  # noqa: E402


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

    n, h, w, fs = a.frames, a.height, a.width, min(24 * 16, a.width)
    clip = make_clip(n, h, w)
    dclip = DeviceImage.from_numpy(ctx, clip)
    say(f"HAVC_stabilizer(stab=True) on a device-resident clip {n} x {h} x {w}, render_factor 24 (filters at {fs} x {fs}), device {ctx.device_name()}")
    say(f"median of {a.reps} calls, each ended by a device synchronise, on the host clock after 2 warm-up calls")

    def report(name, ms, lo, hi, frames=n):
        say(f"{name:<72s} {ms:9.3f} ms per call (min {lo:.3f}, max {hi:.3f}) = {frames / ms * 1e3:9.0f} frames/s")
        return ms

    small = havc.spline64(ctx, dclip, fs, fs)
    from tests import stab_util as SU
    k = 20                                                     # frames 0..15 of the result depend on frames 0..17 (N = 5: two neighbours, two more for flicker)
    got = CS.chroma_stab_np(ctx, small, 5, "A", 1, 15, 0.2, 0.8, flicker=True).numpy()
    want = SU.stab_stage(small.numpy()[:k], 5, "A", 1, 15, 0.2, 0.8)
    assert np.array_equal(got[:k - 4], want[:k - 4]), "havc_chroma_stab_clip does not equal the definition"
    say(f"frames 0..{k - 5} of the stab stage equal the numpy definition byte for byte")

    preset = dict(dark=True, smooth=True, colormap="red->brown")
    t_off = report("HAVC_stabilizer(dark, smooth, colormap), stab off", *median_ms(ctx, lambda: havc.HAVC_stabilizer(dclip, **preset), a.reps))
    t5 = report("HAVC_stabilizer(dark, smooth, colormap, stab), stab_p (5, 'A', 1, 15, 0.2, 0.8)",
                *median_ms(ctx, lambda: havc.HAVC_stabilizer(dclip, stab=True, **preset), a.reps))
    t15 = report("HAVC_stabilizer(dark, smooth, colormap, stab), stab_p (15, 'A', 1, 15, 0.2, 0.8)",
                 *median_ms(ctx, lambda: havc.HAVC_stabilizer(dclip, stab=True, stab_p=(15, 'A', 1, 15, 0.2, 0.8), **preset), a.reps))
    say(f"  stab adds {t5 - t_off:.3f} ms (N = 5) / {t15 - t_off:.3f} ms (N = 15) to {t_off:.3f} ms")
    say()
    say(f"at {fs} x {fs}, {n} frames:")
    stage = {}
    for name, kw in (("N = 5, tht 15, flicker", dict(nframes=5, tht=15, flicker=True)), ("N = 15, tht 15, flicker", dict(nframes=15, tht=15, flicker=True)),
                     ("N = 5, tht 15, no flicker", dict(nframes=5, tht=15, flicker=False)), ("N = 5, tht 0, flicker", dict(nframes=5, tht=0, flicker=True)),
                     ("N = 15, tht 0, flicker", dict(nframes=15, tht=0, flicker=True))):
        stage[name] = report("havc_chroma_stab_clip, " + name,
                             *median_ms(ctx, lambda: CS.chroma_stab_np(ctx, small, mode="A", sat=1, weight=0.2, tht_scen=0.8, **kw), a.reps))
    t_chain = report("havc_stabilizer_chain: dark + smooth + colormap, one launch",
                     *median_ms(ctx, lambda: stabilize_np(ctx, small, (0.2, 0.8, "none"), (0.3, 0.7, 0.9, -0.0, "none"), havc._get_colormap("red->brown")), a.reps))
    t_flick = report("havc_reduce_flicker_clip alone", *median_ms(ctx, lambda: CS.reduce_flicker_np(ctx, small), a.reps))
    npix = n * fs * fs
    t_back = {}
    for mult in (1, 4, 14):
        planes = [ctx.dev_alloc(npix * mult), ctx.dev_alloc(npix * mult // 4), ctx.dev_alloc(npix * mult // 4)]
        src = DeviceImage(ctx, (n * mult, fs, fs, 3))
        out = DeviceImage(ctx, (n * mult, fs, fs, 3))
        for j in range(mult):
            ctx.dev_copy(C.c_void_p(src.ptr.value + j * npix * 3), small.ptr, npix * 3)
        fwd = lambda: nat.check(ctx.lib.havc_rgb_to_yuv420(ctx.h, src.ptr, planes[0], planes[1], planes[2], fs, fs, n * mult), ctx.h)
        back = lambda: nat.check(ctx.lib.havc_yuv420_to_rgb(ctx.h, planes[0], planes[1], planes[2], out.ptr, fs, fs, n * mult), ctx.h)
        report(f"havc_rgb_to_yuv420 alone, {n * mult} frames", *median_ms(ctx, fwd, a.reps), frames=n * mult)
        t_back[mult] = report(f"havc_yuv420_to_rgb alone, {n * mult} frames", *median_ms(ctx, back, a.reps), frames=n * mult)
        for p in planes:
            ctx.dev_free(p)
        del src, out
    say(f"  the N - 1 shifted clips' back conversion alone: {t_back[4]:.3f} ms of {stage['N = 5, tht 15, flicker']:.3f} ms (N = 5), "
        f"{t_back[14]:.3f} ms of {stage['N = 15, tht 15, flicker']:.3f} ms (N = 15)")
    say(f"  stab stage (N = 5) / dark + smooth + colormap launch = {stage['N = 5, tht 15, flicker'] / t_chain:.1f}; flicker alone {t_flick:.3f} ms")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
