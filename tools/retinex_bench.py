#!/usr/bin/env python3
"""HAVC_retinex (csrc/retinex.hip: seven launches per chunk of frames, float64 recursive Gaussians) on a device-resident 1080p clip.  Needs an MI355X.

    python tools/retinex_bench.py [--frames 64] [--reps 5] [--out profiles/retinex.txt] [--no-kernels]

Reported:
  * frames/s of the default call havc.HAVC_retinex(clip) with the clip in HBM.  The call only enqueues, so `reps` calls are enqueued back to back and the host
    clock is read around them and a stream synchronise; 5 windows after 2 warm-up calls; median with min and max next to it.
  * the copy bound of the same bytes: a device-to-device copy of the clip (what a filter that only reads the input and writes the output would move), timed
    the same way.  There is no earlier implementation to compare with and no threshold: the figures are recorded, not gated.
  * per-kernel times: this script run once more as a child under `rocprofv3 --kernel-trace --stats` (one warm-up call and one timed call; tracing slows the
    host, so the frames/s above come from the untraced run), the ret_* rows of the statistics.
  * accuracy: the planes through the tap bit for bit and the bytes against tests/retinex_util.py's float64 restatement on the GPU test's sizes, and the two
    reference-only measurements of tests/test_retinex_host.py -- (a) float32 against float64, (b) the logarithm moved by one ulp."""
import argparse
import csv
import glob
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import retinex_util as U  # noqa: E402
from vsdeoldify_amd import havc  # noqa: E402
from vsdeoldify_amd import retinex as RX  # noqa: E402
from vsdeoldify_amd.device import DeviceImage  # noqa: E402
from vsdeoldify_amd.render import get_context  # noqa: E402


def make_clip(n, h, w, seed=5):
    """frames from dark to bright (both sides of the gate): a ramp, slow waves and noise"""
    r = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    wave = 50 * np.sin(xx / 130.0 + yy / 170.0) + 30 * np.cos(yy / 60.0 - xx / 95.0)
    clip = np.empty((n, h, w, 3), np.uint8)
    for i in range(n):
        level = 25 + 215 * i / max(n - 1, 1) + 40 * (xx / w - 0.5)
        clip[i] = np.clip((level + wave)[:, :, None] + r.integers(-12, 13, (h, w, 3)), 0, 255)
    return clip


def window(ctx, fn, reps):
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def timed(ctx, fn, reps):
    for _ in range(2):
        fn()
    ctx.synchronize()
    v = [window(ctx, fn, reps) for _ in range(5)]
    return statistics.median(v), min(v), max(v)


def accuracy(ctx, say):
    say("accuracy against the float64 numpy restatement (tests/retinex_util.py), 6-frame clips, default sigmas unless named:")
    total = differ = worst = 0
    for h, w in U.SIZES:
        clip = U.make_clip(h, w)
        exact = True
        for sigmas in U.SIGMA_SETS:
            _, g, p = U.reference(h, w, sigmas, True)
            _, planes = RX.retinex_np(ctx, clip, sigmas, tap=True)
            exact &= bool(np.array_equal(planes[:, :-1].view(np.uint64), g.view(np.uint64)) and np.array_equal(planes[:, -1].view(np.uint64), p.view(np.uint64)))
        n_size = mx_size = 0
        for blend in (False, True):
            for tv_in in (True, False):
                for tv_out in (True, False):
                    want = U.retinex_ref(clip, range_tv_in=tv_in, range_tv_out=tv_out, blend=blend, rtx=U.reference_bytes(h, w, (25, 80, 250), tv_in, tv_out))
                    got = RX.retinex_np(ctx, clip, fulls=tv_in, fulld=tv_out, range_tv=tv_in, blend=blend)
                    n, mx = U.count_diff(got, want)
                    n_size, mx_size, total = n_size + n, max(mx_size, mx), total + want.size
        differ, worst = differ + n_size, max(worst, mx_size)
        say(f"  {h:4d} x {w:4d}: Gaussian planes and P bit for bit (both sigma sets): {exact};  bytes over blend x range_tv_in x range_tv_out: {n_size} differ, "
            f"largest difference {mx_size}")
    say(f"  all sizes: {differ} of {total} bytes differ, largest difference {worst}")
    # the two reference-only measurements (CPU)
    h, w = 33, 257
    want = U.reference_bytes(h, w, (25, 80, 250), True, True)[2:]
    n, mx = U.count_diff(U.msrcp(U.make_clip(h, w)[2:], (25, 80, 250), True, True, dtype=np.float32), want)
    say(f"  measurement (a), CPU: float32 restatement against float64 at {h} x {w}, the frames that pass the gate and the constant one: {n} of {want.size} bytes "
        f"differ ({100.0 * n / want.size:.1f} %), largest difference {mx}")
    tot = dif = wst = 0
    for h, w in U.SIZES:
        clip = U.make_clip(h, w)
        want = U.reference_bytes(h, w, (25, 80, 250), True, True)
        inten, _, p = U.reference(h, w, (25, 80, 250), True)
        for seed in (1, 2, 3):
            r = np.random.default_rng(seed)
            got = np.stack([U.msrcp_frame(clip[f], inten[f], p[f], 3, True, True, log_shift=r.integers(-1, 2, inten[f].shape) * (np.ptp(p[f]) > 0))
                            for f in range(len(clip))])
            n, mx = U.count_diff(got, want)
            tot, dif, wst = tot + want.size, dif + n, max(wst, mx)
    say(f"  measurement (b), CPU: float64 restatement with its logarithm moved by one ulp up / down / not at random (3 seeds, all sizes; the constant frame "
        f"excepted): {dif} of {tot} bytes differ, largest difference {wst}")


def kernel_times(args, say):
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--child", "--frames", str(args.frames)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not files:
            say(f"per-kernel times: not measured (rocprofv3 exit code {r.returncode}, {len(files)} statistics files)")
            return
        rows = [row for row in csv.DictReader(open(files[0])) if row.get("Name", "").startswith("ret_")]
    if not rows or not all(k in rows[0] for k in ("Calls", "TotalDurationNs", "AverageNs")):
        say(f"per-kernel times: not measured (no ret_* rows with the expected columns in {os.path.basename(files[0])})")
        return
    say(f"per-kernel times (rocprofv3 --kernel-trace --stats, a run of its own: 2 default calls on {args.frames} frames, so each kernel ran twice per chunk):")
    total = sum(float(row["TotalDurationNs"]) for row in rows)
    for row in sorted(rows, key=lambda q: -float(q["TotalDurationNs"])):
        t = float(row["TotalDurationNs"])
        say(f"  {row['Name'].split('(')[0]:22s} calls {int(row['Calls']):3d}   total {t / 1e6:9.3f} ms   average {float(row['AverageNs']) / 1e6:9.3f} ms   "
            f"{100.0 * t / max(total, 1.0):5.1f} % of the ret_* time")
    say(f"  ret_* kernels together: {total / 2e6:.3f} ms per call of {args.frames} frames = {args.frames / (total / 2e6) * 1e3:.0f} frames/s of kernel time")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    ctx = get_context(0)
    n, h, w = a.frames, 1080, 1920
    clip = make_clip(n, h, w)
    dclip = DeviceImage.from_numpy(ctx, clip)
    if a.child:                                                  # under the profiler: one warm-up call, one more, nothing else
        for _ in range(2):
            havc.HAVC_retinex(dclip)
        ctx.synchronize()
        return
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"HAVC_retinex on a device-resident clip {n} x {h} x {w} ({clip.nbytes / 1e6:.1f} MB), default arguments (sigmas 25 / 80 / 250, gate 0.20 .. 0.80, "
        f"no blend); device {ctx.device_name()}")
    kinds = U.frame_kinds(clip[:: max(n // 16, 1)], True)
    say(f"  of every {max(n // 16, 1)}th frame {sum(1 for k in kinds if k[1])} of {len(kinds)} pass the gate (a gated-out frame still goes through every kernel)")
    out = havc.HAVC_retinex(dclip)
    first = out.numpy()
    same = bool(np.array_equal(havc.HAVC_retinex(dclip).numpy(), first))
    want = U.retinex_ref(clip[n // 2:n // 2 + 1])
    nd, mx = U.count_diff(first[n // 2:n // 2 + 1], want)
    say(f"  second run bit-identical: {same};  frame {n // 2} against the numpy restatement: {nd} of {want.size} bytes differ, largest difference {mx}")
    med, lo, hi = timed(ctx, lambda: havc.HAVC_retinex(dclip), a.reps)
    say(f"  windows of {a.reps} enqueued calls + one synchronise, host clock, 5 windows after 2 warm-up calls; median (min, max):")
    say(f"  HAVC_retinex: {med:9.3f} ms ({lo:.3f}, {hi:.3f}) a call = {n / med * 1e3:8.1f} frames/s")
    spare = dclip.empty_like()
    cmed, clo, chi = timed(ctx, lambda: spare.copy_from(dclip), a.reps * 4)
    say(f"  copy bound (device-to-device copy of the clip: {clip.nbytes / 1e6:.1f} MB read + as much written): {cmed:9.3f} ms ({clo:.3f}, {chi:.3f}) = "
        f"{n / cmed * 1e3:8.0f} frames/s, {2 * clip.nbytes / cmed / 1e9:.2f} TB/s;  HAVC_retinex takes {med / cmed:.1f} x that")
    del spare, out
    if not a.no_kernels:
        kernel_times(a, say)
    accuracy(ctx, say)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if not same:
        raise SystemExit("two runs of HAVC_retinex disagree")


if __name__ == "__main__":
    main()
