#!/usr/bin/env python3
"""clip_delta_e (havc_delta_e_clip, csrc/metrics.hip) on a device-resident 64-frame 1080p clip, with and without the per-pixel map, next to the CPU oracle
(oracle/imaging.py delta_e00_images) on one frame of the same clip on the same box.  Needs an MI355X.

    python tools/delta_e_bench.py [--frames 64] [--reps 25] [--out profiles/delta_e.txt]

Method: the two clips are a smooth colour clip plus noise and the same clip a few code values off (what a fast render against a precise one looks like), both
in device memory, the map a device buffer: a call stages nothing and brings back only the per-frame records (265 KB for 64 frames), which is what ends it.
Every figure is the median over `reps` calls (at least 25) of the time between two HIP events on the context's stream around ONE call, after 3 warm-up
calls, the two cases alternating; min and max beside it.  Frames / s = frames of the clip over that time: an end-to-end rate of the call.  The oracle is
timed on the host clock, best of 3.  Before anything is timed, frame 0 of the GPU map is compared with the oracle and the largest |difference| is reported
(tests/metrics_util.py: pixels on the hue discontinuity are left out and counted).  No threshold is asserted anywhere."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import metrics_util as mu  # noqa: E402
from vsdeoldify_amd import metrics  # noqa: E402
from vsdeoldify_amd.device import DeviceImage  # noqa: E402
from vsdeoldify_amd.render import get_context  # noqa: E402


def make_pair(n, h, w, seed=1):
    r = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    a = np.empty((n, h, w, 3), np.uint8)
    for k in range(n):
        base = np.stack([120 + 70 * np.sin(x / 61 + 0.1 * k), 110 + 60 * np.cos(y / 43 - 0.07 * k), 100 + 50 * np.sin((x + y) / 97 + 0.05 * k)], -1)
        a[k] = np.clip(base + r.normal(0.0, 6.0, (h, w, 3)).astype(np.float32), 0, 255)
    b = np.clip(a.astype(np.int16) + r.integers(-2, 3, a.shape, dtype=np.int16), 0, 255).astype(np.uint8)
    return a, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    reps = max(a.reps, 25)
    import torch
    ctx = get_context(0)
    stream = torch.cuda.ExternalStream(ctx.stream_ptr())
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    n, h, w = a.frames, a.height, a.width
    ca, cb = make_pair(n, h, w)
    da, db = DeviceImage.from_numpy(ctx, ca), DeviceImage.from_numpy(ctx, cb)
    say(f"clip_delta_e on two device-resident clips {n} x {h} x {w} ({2 * ca.nbytes / 1e6:.0f} MB read, map {n * h * w * 8 / 1e6:.0f} MB), device {ctx.device_name()}")

    rep = metrics.delta_e_np(ctx, da, db, return_map=True)
    frame0 = rep.map.numpy()[0]
    t_cpu = []
    for _ in range(3):
        t0 = time.perf_counter()
        want = mu.oracle_map(ca[0], cb[0])
        t_cpu.append(time.perf_counter() - t0)
    err, share = mu.compare_maps(frame0, ca[0], cb[0], want)
    say(f"frame 0 against the oracle: max |GPU - oracle| {err:.3e} over {frame0.size} pixels, share left out at the hue discontinuity {share:.2e}")
    say(f"the clip: mean {rep.clip_mean:.4f}, max {rep.clip_max:.4f}, below 1.0 {rep.below(1.0):.5f}, p99 {rep.percentile(99):.4f}, PSNR {rep.clip_psnr:.2f} dB")
    del rep

    cases = {"records only": lambda: metrics.delta_e_np(ctx, da, db), "records + float64 map": lambda: metrics.delta_e_np(ctx, da, db, return_map=True)}
    for f in cases.values():
        for _ in range(3):
            f()
    ctx.synchronize()
    ms = {k: [] for k in cases}
    for _ in range(reps):
        for k, f in cases.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            f()
            e1.record(stream)
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    say(f"median of {reps} calls between two HIP events on the context's stream, 3 warm-up calls, the cases alternating")
    for k, v in ms.items():
        med = statistics.median(v)
        say(f"{k:<24s} {med:9.3f} ms per call (min {min(v):.3f}, max {max(v):.3f}) = {n / med * 1e3:9.0f} frames/s = {n * h * w / med / 1e6:8.1f} Gpixel/s")
    cpu = min(t_cpu)
    say(f"CPU oracle (float64 numpy, this box), one frame: {cpu:.3f} s (best of 3) = {1 / cpu:.2f} frames/s; "
        f"records only is {n / statistics.median(ms['records only']) * 1e3 * cpu:.0f} x that")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
