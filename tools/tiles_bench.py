#!/usr/bin/env python3
"""HAVC_clip_reconstruct's fused launch (csrc/tiles.hip, havc_tile_reconstruct) on a device-resident clip: 16 x 1080 x 1920, 4 tiles, the overlaps of
HAVC_main's Placebo preset (havc.tiled_preset_params: 192 x 108), the linear ramp (blend_weight 0) and the luma re-attach on -- what the preset runs
behind the four HAVC_colorizer calls.  HAVC_clip_slice is timed next to it.  Needs an MI355X.

    python tools/tiles_bench.py [--reps 20] [--inner 10] [--out profiles/tile_reconstruct.txt]

Method: each item is warmed up, then timed `reps` times by HIP events on the context's stream, `inner` calls back to back between the two events (the
stream stays fed; a single call would time the enqueue); the figure is the median over the repetitions, per call.  The output is compared byte for byte
with a numpy statement of the blend on one frame first.  Bytes that must move = every tile read once + clip_orig read once + the output written once;
GB/s = those bytes / time, next to the 8 TB/s HBM3E peak of the MI355X (the peak profiles/stabilizer_chain.txt uses).  The kernel reads a tile pixel only
where its mask is not at the other end, so the bytes it touches are fewer: that count is printed too."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import tiles_util as U  # noqa: E402
from vsdeoldify_amd import havc  # noqa: E402
from vsdeoldify_amd.device import DeviceImage  # noqa: E402
from vsdeoldify_amd.render import get_context  # noqa: E402

PEAK_GBS = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    ctx = get_context(0)
    stream = torch.cuda.ExternalStream(ctx.stream_ptr())
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    n, h, w, slices = a.frames, 1080, 1920, 4
    ox, oy, _ = havc.tiled_preset_params(w, h, slices)
    r = np.random.default_rng(1)
    clip = r.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    dclip = DeviceImage.from_numpy(ctx, clip)
    ct = havc.HAVC_clip_slice(dclip, slices, ox, oy)
    shape = ct.tiles[0].shape
    tiles = [r.integers(0, 256, shape, dtype=np.uint8) for _ in range(slices)]                   # independent bytes: every seam is a real blend
    ct.tiles = [DeviceImage.from_numpy(ctx, t) for t in tiles]
    got = havc.HAVC_clip_reconstruct(ct, 0, True).numpy()
    want = U.reconstruct_np([t[:1] for t in tiles], clip[:1], ct.base_tile_w, ct.base_tile_h, ox, oy, 0, True)
    same = np.array_equal(got[:1], want)
    items = {
        "HAVC_clip_slice (1 launch)": lambda: havc.HAVC_clip_slice(dclip, slices, ox, oy),
        "HAVC_clip_reconstruct (1 launch)": lambda: havc.HAVC_clip_reconstruct(ct, 0, True),
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
    tile_bytes, clip_bytes = slices * int(np.prod(shape)), n * h * w * 3
    mx, my = U.blend_mask(w, ox, ct.base_tile_w, 0), U.blend_mask(h, oy, ct.base_tile_h, 0)
    touched = int(((1 + ((mx > 0) & (mx < 255)))[None, :] * (1 + ((my > 0) & (my < 255)))[:, None]).sum()) * 3 * n
    say(f"tile reconstruct, Placebo geometry: clip {n} x {h} x {w} x 3 u8 ({clip_bytes / 1e6:.1f} MB), {slices} tiles {shape[1]} x {shape[2]} "
        f"(base {ct.base_tile_h} x {ct.base_tile_w}, overlap {oy} x {ox}), linear ramp, luma re-attach on; device {torch.cuda.get_device_name(0)}")
    say(f"median of {a.reps} repetitions by HIP events, {a.inner} calls per repetition, per call; frame 0 == the numpy statement of the blend: {same}")
    for k in items:
        say(f"  {k:36s} {med[k]:9.4f} ms   (min {min(ms[k]):.4f}, max {max(ms[k]):.4f})")
    t = med["HAVC_clip_reconstruct (1 launch)"] * 1e-3
    must = tile_bytes + 2 * clip_bytes
    say(f"  reconstruct, bytes that must move (tiles {tile_bytes / 1e6:.1f} MB + clip_orig {clip_bytes / 1e6:.1f} MB + output {clip_bytes / 1e6:.1f} MB = "
        f"{must / 1e6:.1f} MB): {must / t / 1e9:.0f} GB/s = {100 * must / t / 1e9 / PEAK_GBS:.1f} % of the {PEAK_GBS / 1000:.0f} TB/s peak")
    act = touched + 2 * clip_bytes
    say(f"  reconstruct, bytes the kernel touches (tile pixels read where their mask is not at the other end: {touched / 1e6:.1f} MB; {act / 1e6:.1f} MB in "
        f"all): {act / t / 1e9:.0f} GB/s = {100 * act / t / 1e9 / PEAK_GBS:.1f} % of the peak")
    ts = med["HAVC_clip_slice (1 launch)"] * 1e-3
    say(f"  slice moves {clip_bytes / 1e6:.1f} MB in + {tile_bytes / 1e6:.1f} MB out: {(clip_bytes + tile_bytes) / ts / 1e9:.0f} GB/s = "
        f"{100 * (clip_bytes + tile_bytes) / ts / 1e9 / PEAK_GBS:.1f} % of the peak")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if not same:
        raise SystemExit("the fused launch does not reproduce the numpy statement of the blend")


if __name__ == "__main__":
    main()
