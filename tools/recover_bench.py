#!/usr/bin/env python3
"""HAVC_recover_clip_color (csrc/recover.hip: two launches per clip, frame-level decisions on the device) on a device-resident 1080p clip, in frames/s, against
the frame-by-frame composition of the entry points that existed before it: havc.spline64 down on both clips, mcomb.chroma_retention_frame per frame (one luma
launch, one blocking read-back of a double and one restore launch per frame, then a copy into the clip, as havc._per_frame does), havc.spline64 up with the
luma of the clip, mcomb.simple_merge.  Needs an MI355X.

    python tools/recover_bench.py [--frames 64] [--reps 50] [--out profiles/recover_clip.txt]

Cases: the default arguments (chroma_resize=True: 1920 -> 768 x 768 and back) and chroma_resize=False, both at strength 1.0 (the default) and at 0.5 (the closing
blend runs).  Method: both operands stay in HBM.  The clip call only enqueues, so `reps` calls are enqueued back to back and the host clock is read around
them and a stream synchronise; the composition blocks once per frame by construction and is timed the same way with fewer repetitions.  The two sides
ALTERNATE, window by window, in one process on one device, after 2 warm-up calls each; 5 windows each, median with min and max next to it: the spread of
the windows is the run-to-run spread a difference has to exceed.  The result of the clip call is compared with the composition's, byte for byte, on the whole
clip before anything is timed."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vsdeoldify_amd import havc, mcomb  # noqa: E402
from vsdeoldify_amd.device import DeviceImage  # noqa: E402
from vsdeoldify_amd.render import get_context  # noqa: E402


def make_clips(n, h, w, seed=3):
    """the clip to repair: frames from dark to bright (both sides of the luma gate) with gray and coloured regions; the donor: smooth colour + noise"""
    r = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    a = np.empty((n, h, w, 3), np.uint8)
    b = np.empty((n, h, w, 3), np.uint8)
    tint = np.stack([40 * np.sin(xx / 90.0), 40 * np.cos(yy / 70.0), 40 * np.sin((xx + yy) / 110.0)], -1) * (xx[..., None] > w // 2)
    col = np.stack([128 + 100 * np.sin(xx / 37.0 + yy / 53.0), 128 + 100 * np.cos(yy / 29.0 - xx / 71.0), 128 + 100 * np.sin((xx + yy) / 43.0 + 1.0)], -1)
    for i in range(n):
        level = 30 + 200 * i / max(n - 1, 1) + 40 * (xx / w - 0.5)
        a[i] = np.clip(level[:, :, None] + tint + r.integers(-6, 7, (h, w, 3)), 0, 255)
        b[i] = np.clip(col + r.integers(-10, 11, (h, w, 3)), 0, 255)
    return a, b


def composition(ctx, da, db, chroma_resize, strength):
    n, h, w, _ = da.shape
    fs = mcomb.recover_size(w) if chroma_resize else None
    sa, sb = (da, db) if fs is None else (havc.spline64(ctx, da, fs, fs), havc.spline64(ctx, db, fs, fs))
    restored = sa.empty_like()
    for i in range(n):
        restored.frame(i).copy_from(mcomb.chroma_retention_frame(sa.frame(i), sb.frame(i), 0.8, 30, 1.0, 2.0))
    if fs is not None:
        restored = havc.spline64(ctx, restored, w, h, luma_from=da)
    return mcomb.simple_merge(da.as_rows(), restored.as_rows(), strength).reshaped(da.shape)


def window(ctx, fn, reps):
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = get_context(0)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    n, h, w = a.frames, 1080, 1920
    clip, color = make_clips(n, h, w)
    da, db = DeviceImage.from_numpy(ctx, clip), DeviceImage.from_numpy(ctx, color)
    say(f"HAVC_recover_clip_color on a device-resident clip {n} x {h} x {w} ({clip.nbytes / 1e6:.1f} MB a clip, two clips in); device {ctx.device_name()}")
    say(f"clip call: windows of {a.reps} enqueued calls + one synchronise; composition (existing per-frame entry points): windows of {max(a.reps // 5, 1)} calls; "
        "host clock; the two alternate; 5 windows each after 2 warm-up calls each; median (min, max)")
    ok = True
    for chroma_resize in (True, False):
        for strength in (1.0, 0.5):
            new = lambda: havc.HAVC_recover_clip_color(da, db, strength=strength, chroma_resize=chroma_resize)            # noqa: E731
            old = lambda: composition(ctx, da, db, chroma_resize, strength)                                                # noqa: E731
            same = bool(np.array_equal(new().numpy(), old().numpy()))
            ok &= same
            for _ in range(2):
                new()
                old()
            ctx.synchronize()
            vn, vo = [], []
            for _ in range(5):
                vn.append(window(ctx, new, a.reps))
                vo.append(window(ctx, old, max(a.reps // 5, 1)))
            mn, mo = statistics.median(vn), statistics.median(vo)
            say(f"  chroma_resize={chroma_resize!s:5s} strength={strength}:  clip call {mn:8.3f} ms ({min(vn):.3f}, {max(vn):.3f}) = {n / mn * 1e3:8.0f} frames/s"
                f"   composition {mo:8.3f} ms ({min(vo):.3f}, {max(vo):.3f}) = {n / mo * 1e3:8.0f} frames/s   ratio {mo / mn:5.2f}"
                f"   (slowest clip-call window against fastest composition window: {min(vo) / max(vn):5.2f})   same bytes: {same}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if not ok:
        raise SystemExit("the clip call and the composition disagree")


if __name__ == "__main__":
    main()
