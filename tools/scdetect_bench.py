#!/usr/bin/env python3
"""havc_scene_stats (csrc/scdetect.hip) on device-resident clips: 64 x 480 x 854 (what HAVC_SceneDetect looks at after resize_min_HW) and 16 x 1080 x 1920,
each without and with normalisation, next to the same statistics taken with torch ops on the SAME device memory -- what a user would write today.
Needs an MI355X.

    python tools/scdetect_bench.py [--reps 30] [--out profiles/scene_stats.txt]

Method: both legs end with the per-frame records in host memory (the entry point blocks until they are there; the torch leg ends in .cpu()), so each call
is timed on the host clock around the whole call, after 5 warm-up calls; the figure is the median over `reps` calls, min and max next to it.  The two
legs are compared for equality first.  Bytes that must move = the clip read once (the compared frame is re-read, but it was read by the blocks of the
frame before it at about the same time); with normalisation the clip is read by both passes: twice.  GB/s = those bytes / time, next to the 8 TB/s
HBM3E peak of the MI355X (the peak profiles/stabilizer_chain.txt uses).  The time includes the launch, the 32-byte-per-frame download and the stream
synchronisation: for the smaller clip that fixed part is not negligible."""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vsdeoldify_amd import scdetect as SD  # noqa: E402
from vsdeoldify_amd.device import DeviceImage  # noqa: E402
from vsdeoldify_amd.render import get_context  # noqa: E402

PEAK_GBS = 8000.0


def torch_stats(t, offset, normalize, coeffs, tb=SD.DEF_THT_BLACK_MIN, tw=SD.DEF_THT_WHITE_MIN):
    import torch
    cr, cg, cb, bias = coeffs
    c = t.to(torch.int32)
    y = (cr * c[..., 0] + cg * c[..., 1] + cb * c[..., 2] + bias) >> 16
    mn, mx = y.amin((1, 2)), y.amax((1, 2))
    raw = y.sum((1, 2), dtype=torch.int64)
    if normalize:
        luma = raw.double() / (y.shape[1] * y.shape[2]) / 255.0
        inside = ~((luma <= tb) | (luma >= tw))
        d = (mx - mn).clamp(min=1).double()[:, None, None]
        yn = (255.0 * ((y - mn[:, None, None]).double() / d)).to(torch.int32)
        y = torch.where(inside[:, None, None], yn, y)
    prev = torch.cat([y[:1].expand(min(offset, y.shape[0]), -1, -1), y[:-offset]])[:y.shape[0]]
    out = torch.stack([y.sum((1, 2), dtype=torch.int64), (y - prev).abs().sum((1, 2), dtype=torch.int64), raw, mn.long(), mx.long()])
    return out.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    ctx = get_context(0)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"scene statistics of a device-resident clip, offset 1, limited-range BT.709; device {torch.cuda.get_device_name(0)}")
    say(f"median of {a.reps} blocking calls on the host clock after 5 warm-up calls, records in host memory at the end of both legs")
    ok = True
    for n, h, w in ((64, 480, 854), (16, 1080, 1920)):
        r = np.random.default_rng(n)
        level = r.integers(30, 200, (n, 1, 1, 1))
        clip = np.clip(level + r.integers(-40, 41, (n, h, w, 3)), 0, 255).astype(np.uint8)
        t = torch.from_numpy(clip).cuda()
        torch.cuda.synchronize()
        dclip = DeviceImage(ctx, clip.shape, ptr=ctypes.c_void_p(t.data_ptr()), owner=t)          # the very memory torch reads
        for normalize in (False, True):
            legs = {"havc_scene_stats": lambda: SD.scene_stats(ctx, dclip, 1, normalize),
                    "torch ops": lambda: torch_stats(t, 1, normalize, SD.LUMA_LIMITED)}
            rec, tor = legs["havc_scene_stats"](), legs["torch ops"]()
            same = all(np.array_equal(rec[k].astype(np.int64), tor[i]) for i, k in enumerate(("sum_y", "sad", "sum_raw", "min_y", "max_y")))
            ok &= same
            ms = {}
            for k, f in legs.items():
                for _ in range(5):
                    f()
                v = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    f()
                    v.append((time.perf_counter() - t0) * 1e3)
                ms[k] = v
            must = clip.nbytes * (2 if normalize else 1)
            say(f"{n} x {h} x {w} ({clip.nbytes / 1e6:.1f} MB), normalize {'on (2 launches)' if normalize else 'off (1 launch)'}; kernel == torch: {same}")
            for k, v in ms.items():
                m = statistics.median(v)
                say(f"  {k:18s} {m:9.4f} ms   (min {min(v):.4f}, max {max(v):.4f})   {must / 1e6:.1f} MB that must move: {must / m / 1e6:7.0f} GB/s = "
                    f"{100 * must / m / 1e6 / PEAK_GBS:5.1f} % of the {PEAK_GBS / 1000:.0f} TB/s peak")
            say(f"  torch / kernel: {statistics.median(ms['torch ops']) / statistics.median(ms['havc_scene_stats']):.1f}x")
        del dclip, t
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if not ok:
        raise SystemExit("the kernel and the torch statement disagree")


if __name__ == "__main__":
    main()
