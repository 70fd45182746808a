#!/usr/bin/env python3
"""havc_planes_to_rgb24 / havc_rgb24_to_planes on a 1080p clip next to the two tweak conversions they generalise, and the first measurement of planar
transfers against RGB24 transfers.  Needs an MI355X.

    python tools/vformat_bench.py [--frames 64] [--reps 10] [--out profiles/vformat.txt]

Method (tools/tweak_bench.py's): the clip is smooth colour plus noise, so the error diffusion sees fractions everywhere.  A timed call ends in a device
synchronise; every figure is the median over `reps` such calls on the host clock after 2 warm-up calls, min and max beside it: the spread.  Calls that are
compared are ALTERNATED inside one loop (a, b, a, b, ...), so drift of the shared machine hits both alike.  Frames / s = frames of the clip over that time:
an end-to-end rate of the call, not a kernel's share of peak.
  check 1  havc_planes_to_rgb24 (YUV420P8, 709, limited, dither) against havc_yuv420_to_rgb on the same device planes: the same design and per-pixel work
           apart from constants, so the new time should lie within the old one's run-to-run spread.
  check 2  havc_rgb24_to_planes with dither (no predecessor) at 8 and 10 bit, and without dither (its own tiled kernel) next to havc_rgb_to_yuv420.
  check 3  the PCIe argument: host planes -> DeviceImage -> host planes (the planes are what crosses the bus) against the same frames as host RGB24 in and
           out (upload, both conversions on the device, download), for YUV420P8 (1.5 B / pixel each way against 3) and YUV420P10 (3 against 3).  Pageable
           numpy memory on the host, as a caller has it.  No target is set.
The first rows of frame 0 are checked against the numpy definition (tests/vformat_util.py) before anything is timed."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from tweak_bench import make_clip  # noqa: E402
from vsdeoldify_amd import _native as nat  # noqa: E402
from vsdeoldify_amd import vformat as VF  # noqa: E402
from vsdeoldify_amd.device import DeviceImage  # noqa: E402
from vsdeoldify_amd.render import get_context  # noqa: E402

LIMITED = dict(matrix="709", full_range=False, depth_full_range=False, dither=True)


def alternated_ms(ctx, calls, reps):
    """calls: name -> callable; every round runs each once, each ended by a synchronise -> name -> (median, min, max) in ms"""
    def once(fn):
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3
    for _ in range(2):
        for fn in calls.values():
            once(fn)
    v = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            v[k].append(once(fn))
    return {k: (statistics.median(t), min(t), max(t)) for k, t in v.items()}


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
    say(f"havc_planes_to_rgb24 / havc_rgb24_to_planes on a clip {n} x {h} x {w} ({npix * 3 / 1e6:.0f} MB as RGB24), device {ctx.device_name()}")
    say(f"median of {a.reps} calls (min, max = the spread), each ended by a device synchronise, host clock, 2 warm-up calls; compared calls alternate in one loop")

    def report(name, t, note=""):
        ms, lo, hi = t
        say(f"{name:<66s} {ms:9.3f} ms per call (min {lo:.3f}, max {hi:.3f}) = {n / ms * 1e3:8.0f} frames/s{note}")

    # ---- the planes, made by the library itself, and the check against the definition ----
    from tests import vformat_util as U
    p8 = VF.rgb24_to_planes_np(ctx, dclip, "YUV420P8", LIMITED, device=True)
    p10 = VF.rgb24_to_planes_np(ctx, dclip, "YUV420P10", LIMITED, device=True)
    rows = 72
    want = U.rgb_to_planes(clip[:1, :rows], 1, 1, 10, "709", False, True)
    got = [q.numpy() for q in p10]
    assert np.array_equal(got[0][0, :64], want[0][0, :64]) and np.array_equal(got[1][0, :30], want[1][0, :30]) and np.array_equal(got[2][0, :30], want[2][0, :30])
    h8 = [q.numpy() for q in p8]
    rgb8 = VF.planes_to_rgb24_np(ctx, VF.VideoClip(p8, "YUV420P8"), LIMITED, device=True)
    want = U.planes_to_rgb(h8[0][:1, :rows], h8[1][:1, :rows // 2], h8[2][:1, :rows // 2], 1, 1, 8, "709", False, False, True)
    assert np.array_equal(rgb8.numpy()[0, :64], want[0, :64])
    say("the first 64 rows of frame 0 equal the numpy definition byte for byte, both directions")

    def vf(fmt, steps):
        return VF._vformat(VF.FORMATS[fmt], n, h, w, steps, steps["depth_full_range"])

    out = DeviceImage(ctx, clip.shape)
    ptr = lambda planes: [q.ptr for q in planes]

    # ---- check 1 ----
    say()
    say("check 1: planes -> RGB24 with error diffusion, device operands")
    f_lim, f_full = vf("YUV420P8", LIMITED), vf("YUV420P8", dict(LIMITED, full_range=True))
    t = alternated_ms(ctx, {
        "old": lambda: nat.check(ctx.lib.havc_yuv420_to_rgb(ctx.h, *ptr(p8), out.ptr, w, h, n), ctx.h),
        "new": lambda: nat.check(ctx.lib.havc_planes_to_rgb24(ctx.h, *ptr(p8), out.ptr, C.byref(f_lim)), ctx.h),
        "new_full": lambda: nat.check(ctx.lib.havc_planes_to_rgb24(ctx.h, *ptr(p8), out.ptr, C.byref(f_full)), ctx.h),
        "new10": lambda: nat.check(ctx.lib.havc_planes_to_rgb24(ctx.h, *ptr(p10), out.ptr, C.byref(vf("YUV420P10", LIMITED))), ctx.h)}, a.reps)
    report("havc_yuv420_to_rgb (tweak_back_kernel: 709, full, 8 bit)", t["old"])
    report("havc_planes_to_rgb24 YUV420P8 709 limited (vf_back_kernel)", t["new"])
    report("havc_planes_to_rgb24 YUV420P8 709 full (the old call's bytes)", t["new_full"])
    report("havc_planes_to_rgb24 YUV420P10 709 limited", t["new10"])
    old, new = t["old"], t["new"]
    where = "inside" if old[1] <= new[0] <= old[2] else ("BELOW" if new[0] < old[1] else "ABOVE")
    say(f"  new / old = {new[0] / old[0]:.4f}; the old call's spread is {old[1]:.3f} .. {old[2]:.3f} ms: the new median lies {where} it")

    # ---- check 2 ----
    say()
    say("check 2: RGB24 -> planes, device operands")
    o8 = [VF.DevicePlane(ctx, q.shape, q.dtype) for q in p8]
    o10 = [VF.DevicePlane(ctx, q.shape, q.dtype) for q in p10]
    f_nod = vf("YUV420P8", dict(LIMITED, full_range=True, dither=False))
    f_10 = vf("YUV420P10", LIMITED)
    t = alternated_ms(ctx, {
        "old": lambda: nat.check(ctx.lib.havc_rgb_to_yuv420(ctx.h, dclip.ptr, *ptr(o8), w, h, n), ctx.h),
        "nod": lambda: nat.check(ctx.lib.havc_rgb24_to_planes(ctx.h, dclip.ptr, *ptr(o8), C.byref(f_nod)), ctx.h),
        "d8": lambda: nat.check(ctx.lib.havc_rgb24_to_planes(ctx.h, dclip.ptr, *ptr(o8), C.byref(f_lim)), ctx.h),
        "d10": lambda: nat.check(ctx.lib.havc_rgb24_to_planes(ctx.h, dclip.ptr, *ptr(o10), C.byref(f_10)), ctx.h)}, a.reps)
    report("havc_rgb_to_yuv420 (tweak_forward_kernel: tiled, never dithers)", t["old"])
    report("havc_rgb24_to_planes YUV420P8 709 full, dither 0 (vf_fwd_tiled_kernel)", t["nod"], f"; {t['nod'][0] / t['old'][0]:.1f} x the tiled kernel")
    report("havc_rgb24_to_planes YUV420P8 709 limited, dither 1 (vf_fwd_kernel)", t["d8"])
    report("havc_rgb24_to_planes YUV420P10 709 limited, dither 1", t["d10"])

    # ---- check 3 ----
    say()
    say("check 3: what crosses the bus.  Pageable host memory; both paths run the same two conversions on the device")
    for fmt, dplanes in (("YUV420P8", p8), ("YUV420P10", p10)):
        hp = [q.numpy() for q in dplanes]
        hout = [np.empty_like(q) for q in hp]
        rgb_out = np.empty_like(clip)
        mid = DeviceImage(ctx, clip.shape)
        dpl = [VF.DevicePlane(ctx, q.shape, q.dtype) for q in hp]
        f = vf(fmt, LIMITED)
        plane_bytes = sum(q.nbytes for q in hp)

        def planar():
            nat.check(ctx.lib.havc_planes_to_rgb24(ctx.h, *[nat.as_ptr(q) for q in hp], mid.ptr, C.byref(f)), ctx.h)
            nat.check(ctx.lib.havc_rgb24_to_planes(ctx.h, mid.ptr, *[nat.as_ptr(q) for q in hout], C.byref(f)), ctx.h)

        def rgb24():
            ctx.dev_upload(mid.ptr, clip)
            nat.check(ctx.lib.havc_rgb24_to_planes(ctx.h, mid.ptr, *ptr(dpl), C.byref(f)), ctx.h)
            nat.check(ctx.lib.havc_planes_to_rgb24(ctx.h, *ptr(dpl), out.ptr, C.byref(f)), ctx.h)
            ctx.dev_download(rgb_out, out.ptr)

        def resident():
            nat.check(ctx.lib.havc_planes_to_rgb24(ctx.h, *ptr(dplanes), mid.ptr, C.byref(f)), ctx.h)
            nat.check(ctx.lib.havc_rgb24_to_planes(ctx.h, mid.ptr, *ptr(dpl), C.byref(f)), ctx.h)

        t = alternated_ms(ctx, dict(planar=planar, rgb24=rgb24, resident=resident), a.reps)
        report(f"{fmt}: host planes -> DeviceImage -> host planes", t["planar"], f"; {plane_bytes / 1e6:.0f} MB in + {plane_bytes / 1e6:.0f} MB out")
        report(f"{fmt}: host RGB24 -> device, both conversions, -> host RGB24", t["rgb24"], f"; {clip.nbytes / 1e6:.0f} MB in + {clip.nbytes / 1e6:.0f} MB out")
        report(f"{fmt}: the two conversions alone, device-resident", t["resident"])
        say(f"  planar / RGB24 = {t['planar'][0] / t['rgb24'][0]:.3f}; transfers and waiting cost {t['planar'][0] - t['resident'][0]:.2f} ms (planar) and "
            f"{t['rgb24'][0] - t['resident'][0]:.2f} ms (RGB24) over the resident time")
    if a.out:
        with open(a.out, "w") as fo:
            fo.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
