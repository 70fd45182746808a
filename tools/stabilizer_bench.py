#!/usr/bin/env python3
"""HAVC_stabilizer's filter chain on device-resident clips: the five existing launches (image_tweak + luma merge, image_chroma_tweak + luma merge,
image_chroma_tweak) against the one fused launch (csrc/stabilizer.hip, stabilizer.stabilize_np), plus the whole HAVC_stabilizer call, with the parameters
of HAVC_main's `medium` preset (dark [0.2, 0.8], smooth [0.3, 0.7, 0.9, 0.0, "none"], colormap "red->brown").  Needs an MI355X.

    python tools/stabilizer_bench.py [--reps 20] [--inner 10] [--out profiles/stabilizer_chain.txt]

Method: every item is warmed up, then timed `reps` times by HIP events on the context's stream, `inner` calls back to back between the two events (the
stream stays fed; a single call would time the enqueue), the items alternating inside a repetition; the figure is the median over the repetitions, per
call.  The outputs of the two chains are compared byte for byte first.  GB/s of the fused launch = (one read + one write of the clip) / time, next to
the 8 TB/s HBM3E peak of the MI355X."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vsdeoldify_amd import havc, imfilters as F, stabilizer as S  # noqa: E402
from vsdeoldify_amd.device import DeviceImage  # noqa: E402
from vsdeoldify_amd.render import get_context  # noqa: E402

DARK, SMOOTH, COLORMAP = (0.2, 0.8, "none"), (0.3, 0.7, 0.9, -0.0, "none"), havc._get_colormap("red->brown")
PEAK_GBS = 8000.0


def clip(seed, n, h, w):
    """seeded colourful frames, dark on the left and bright on the right: every luma mask and hue range of the preset selects part of the picture"""
    r = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    level = (0.04 + 0.96 * xx / (w - 1))[..., None] ** 1.5
    out = np.empty((n, h, w, 3), np.uint8)
    for i in range(n):
        col = np.stack([128 + 110 * np.sin(xx / (37.0 + i) + yy / 230.0), 128 + 110 * np.cos(yy / (25.0 + i) - xx / 310.0),
                        128 + 110 * np.sin((xx + yy) / 90.0 + 1.0 + i)], -1)
        out[i] = np.clip(col * level + 6 * r.standard_normal((h, w, 3), dtype=np.float32), 0, 255).astype(np.uint8)
    return out


def unfused(ctx, d):
    """the chain through the five existing entry points, the clip as one tall image (what dark_tweak_frame -> chroma_bright_tweak_frame ->
    colormap_frame launch per frame)"""
    white = min(max(DARK[0], 0.1), 0.50)
    t = F.image_tweak_np(ctx, d, sat=min(max(1.1 - DARK[1], 0.10), 0.80), bright=-min(max(DARK[1], 0.20), 0.90), hue_range=DARK[2])
    x = F.luma_merge_np(ctx, t, d, *S._luma_merge_mode(0.1, white))
    t = F.image_chroma_tweak_np(ctx, x, sat=SMOOTH[2], bright=SMOOTH[3], hue_adjust=SMOOTH[4])
    x = F.luma_merge_np(ctx, t, x, *S._luma_merge_mode(SMOOTH[0], SMOOTH[1]))
    return F.image_chroma_tweak_np(ctx, x, hue_adjust=COLORMAP)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    ctx = get_context(0)
    stream = torch.cuda.ExternalStream(ctx.stream_ptr())
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"stabilizer chain, preset medium: dark {DARK}, smooth {SMOOTH}, colormap {COLORMAP!r}; device {torch.cuda.get_device_name(0)}")
    say(f"median of {a.reps} repetitions by HIP events, {a.inner} calls per repetition, per call; items alternate inside a repetition")
    for n, h, w in ((64, 384, 384), (16, 1080, 1920)):
        d = DeviceImage.from_numpy(ctx, clip(1, n, h, w))
        rows = d.as_rows()
        same = np.array_equal(unfused(ctx, rows).numpy().reshape(d.shape), S.stabilize_np(ctx, d, DARK, SMOOTH, COLORMAP).numpy())
        items = {
            "unfused chain (5 launches)": lambda: unfused(ctx, rows),
            "fused chain (1 launch)": lambda: S.stabilize_np(ctx, d, DARK, SMOOTH, COLORMAP),
            "HAVC_stabilizer (squash + chain + back)": lambda: havc.HAVC_stabilizer(d, True, DARK[:2], True, (0.3, 0.7, 0.9, 0.0, "none"), colormap="red->brown"),
        }
        for f in items.values():
            for _ in range(3):
                f()
        ctx.synchronize()
        ms = {k: [] for k in items}
        for _ in range(a.reps):
            for k, f in items.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(a.inner):
                    f()
                e1.record(stream)
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1) / a.inner)
        med = {k: statistics.median(v) for k, v in ms.items()}
        nbytes = n * h * w * 3
        gbs = 2 * nbytes / (med["fused chain (1 launch)"] * 1e-3) / 1e9
        say()
        say(f"clip {n} x {h} x {w} x 3 u8 ({nbytes / 1e6:.1f} MB), device-resident; fused bytes == unfused bytes: {same}")
        for k in items:
            say(f"  {k:42s} {med[k]:9.4f} ms   (min {min(ms[k]):.4f}, max {max(ms[k]):.4f})")
        say(f"  fused / unfused: {med['unfused chain (5 launches)'] / med['fused chain (1 launch)']:.2f} x faster; fused launch moves "
            f"{gbs:.0f} GB/s = {100 * gbs / PEAK_GBS:.1f} % of the {PEAK_GBS / 1000:.0f} TB/s peak")
        if not same:
            raise SystemExit("the fused chain does not reproduce the unfused chain")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
