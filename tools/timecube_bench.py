#!/usr/bin/env python3
"""havc_lut3d_clip, HAVC_TimeCube and havc_overlay_clip on a device-resident 1080p clip, each next to a device-to-device copy of the same bytes measured in
the same run.  Needs an MI355X.

    python tools/timecube_bench.py [--frames 64] [--reps 10] [--out profiles/timecube.txt]

Method: the clip is smooth colour (sines per channel) plus noise, so neighbouring pixels fall into neighbouring cells of the table as a graded picture's do.
Every operand lives in device memory, so a call only enqueues: each timed call ends in a device synchronise, and every figure is the median over `reps` such
calls on the host clock after 2 warm-up calls (min and max beside it), the cases alternating with the copy.  Frames / s = frames of the clip over that time:
an end-to-end rate of the call, not a kernel's share of peak.
  * havc_lut3d_clip at N = 17, 33, 65 with a random table (every corner a different value) and with an identity table; the table is already in device memory
    (what a caller that grades many clips does), so a call is the pad launch over N^3 points and the pass over the clip;
  * HAVC_TimeCube end to end for effect 2 at strength 0.8 from a generated cube: LUT, havc_tweak_clip (forward + back), merge;
  * havc_overlay_clip: mode `overlay`, a 3-plane mask read plane by plane, opacity 0.8, an overlay of the base's size placed at (0, 0);
  * the copy bound: havc_dev_copy of the clip's bytes, the same 3 bytes read and 3 written per pixel the LUT moves (the overlay call reads 9 and writes 3).
No threshold is asserted anywhere.  The first frame of every LUT result is checked against the numpy definition before anything is timed."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import timecube_util as U  # noqa: E402
from vsdeoldify_amd import _native as nat  # noqa: E402
from vsdeoldify_amd import havc  # noqa: E402
from vsdeoldify_amd import timecube as TC  # noqa: E402
from vsdeoldify_amd.device import DeviceImage  # noqa: E402
from vsdeoldify_amd.render import get_context  # noqa: E402


def make_clip(n, h, w, seed=1):
    r = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    clip = np.empty((n, h, w, 3), np.uint8)
    for k in range(n):
        base = np.stack([120 + 70 * np.sin(x / 61 + 0.1 * k), 110 + 60 * np.cos(y / 43 - 0.07 * k), 100 + 50 * np.sin((x + y) / 97 + 0.05 * k)], -1)
        clip[k] = np.clip(base + r.normal(0.0, 6.0, (h, w, 3)).astype(np.float32), 0, 255)
    return clip


def timed(ctx, call):
    t0 = time.perf_counter()
    call()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternating(ctx, call, copy, reps):
    """the call and the copy in turns -> (median, min, max) of each"""
    for _ in range(2):
        timed(ctx, call)
        timed(ctx, copy)
    a, b = [], []
    for _ in range(reps):
        a.append(timed(ctx, call))
        b.append(timed(ctx, copy))
    return (statistics.median(a), min(a), max(a)), (statistics.median(b), min(b), max(b))


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
    nbytes = n * h * w * 3
    clip = make_clip(n, h, w)
    dclip, dout, dcopy = DeviceImage.from_numpy(ctx, clip), DeviceImage(ctx, clip.shape), DeviceImage(ctx, clip.shape)
    copy = lambda: ctx.dev_copy(dcopy.ptr, dclip.ptr, nbytes)
    say(f"havc_lut3d_clip / HAVC_TimeCube / havc_overlay_clip on a device-resident clip {n} x {h} x {w} ({nbytes / 1e6:.0f} MB), device {ctx.device_name()}")
    say(f"median of {a.reps} calls, each ended by a device synchronise, on the host clock after 2 warm-up calls; every case alternates with a device copy of the clip")

    def report(name, call):
        (ms, lo, hi), (cms, clo, chi) = alternating(ctx, call, copy, a.reps)
        say(f"{name:<52s} {ms:8.3f} ms per call (min {lo:.3f}, max {hi:.3f}) = {n / ms * 1e3:8.0f} frames/s; copy {cms:.3f} ms (min {clo:.3f}, max {chi:.3f}); "
            f"call / copy = {ms / cms:.2f}")
        return ms

    lut_ms = {}
    for size in (17, 33, 65):
        for kind, cube in (("random", U.random_cube(size)), ("identity", U.identity_cube(size))):
            idx, frac = TC.axis_tables(cube)
            d_table = ctx.dev_alloc(cube.table.nbytes)
            ctx.dev_upload(d_table, cube.table.view(np.uint8).reshape(-1))
            p = nat.Lut3dParams(width=w, height=h, n_frames=n, size=size)
            call = lambda: nat.check(ctx.lib.havc_lut3d_clip(ctx.h, dclip.ptr, dout.ptr, d_table, nat.as_ptr(idx), nat.as_ptr(frac), C.byref(p)), ctx.h)
            call()
            assert np.array_equal(dout.frame(0).numpy(), U.lut3d(clip[0], cube)), "havc_lut3d_clip does not equal the definition"
            lut_ms[(size, kind)] = report(f"havc_lut3d_clip N = {size}, {kind} table ({size ** 3 * 16 / 1e6:.2f} MB of points)", call)
            ctx.dev_free(d_table)
    say(f"  random table: N = 65 takes {lut_ms[(65, 'random')] / lut_ms[(17, 'random')]:.2f} x the time of N = 17, N = 33 {lut_ms[(33, 'random')] / lut_ms[(17, 'random')]:.2f} x")

    cube = U.graded_cube(33, seed=2)
    got = havc.HAVC_TimeCube(dclip, 0.8, 2, cube=cube)
    assert isinstance(got, DeviceImage)
    report("HAVC_TimeCube effect 2, strength 0.8, N = 33", lambda: havc.HAVC_TimeCube(dclip, 0.8, 2, cube=cube))

    r = np.random.default_rng(3)
    dov = DeviceImage.from_numpy(ctx, make_clip(n, h, w, seed=2))
    dmask = DeviceImage.from_numpy(ctx, r.integers(0, 256, clip.shape, dtype=np.uint8))
    p = nat.OverlayParams(base_w=w, base_h=h, ov_w=w, ov_h=h, n_frames=n, x=0, y=0, mode=7, plane_mask=7, mask_planes=3, mask_first_plane=0, overlay_frames=n,
                          opacity=0.8)
    report("havc_overlay_clip, mode overlay, 3-plane mask", lambda: nat.check(ctx.lib.havc_overlay_clip(ctx.h, dclip.ptr, dov.ptr, dmask.ptr, dout.ptr, C.byref(p)), ctx.h))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
