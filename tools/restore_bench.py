#!/usr/bin/env python3
"""HAVC_restore_video on a device-resident 1080p clip with a 720 x 540 reference video, in frames/s, for both exemplar models, and the two resize kernels
it adds next to their existing siblings at the same shapes.  Needs an MI355X.

    python tools/restore_bench.py [--reps 25] [--out profiles/restore_video.txt]

Method: everything stays in HBM; HIP events on the context's stream around each call (the routes block on the host between frames, so the events span the
whole call; the last event is synchronised); 2 warm-up calls per item, then `reps` repetitions with the items of a group alternating inside a repetition;
median with min and max.  Weights are seeded (vsdeoldify_amd.synth): the arithmetic, not the colours, is what is timed.  The routes:

  ex_model 0  ColorMNet, method 6, render_speed 'medium': Spline36 of clip_ref to 1080p, scene detection on it, DeepExColorMNet frame by frame
  ex_model 2  DeepRemaster, method 6 (references = scenes of clip_ref, ref_freq 10) and method 5 with ref_merge 2 (every frame blended with its LANCZOS-
              resized clip_ref frame): Spline36, scene detection, Spline64 to 576 x 320, batches of 2 frames (one LANCZOS call per batch), Spline64 back with luma, luma recovery; the
              packed weights are uploaded by every call

The kernels: Spline36 / Spline64 on the clip_ref -> clip resize (720 x 540 -> 1920 x 1080, the whole clip in one call) and the clip -> inference-size resize
(1920 x 1080 -> 576 x 320).  Pillow LANCZOS / BICUBIC on 1, 2 and all frames 1920 x 1080 -> 576 x 320 are CALL times of havc_pil_resize_n (two launches, the
coefficient tables built on the host and uploaded per call, one stream synchronise), not bare kernel times; the whole-clip call amortises the set-up and
is the nearest to the kernels' own time."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vsdeoldify_amd import _native as nat  # noqa: E402
from vsdeoldify_amd import havc  # noqa: E402
from vsdeoldify_amd.device import DeviceImage  # noqa: E402


def make_clips(n, h, w, hr, wr, cut_every=12, seed=5):
    """a gray master with a cut every `cut_every` frames and a tinted reference video of it at another size"""
    r = np.random.default_rng(seed)

    def frames(hh, ww):
        yy, xx = np.mgrid[0:hh, 0:ww] * (h / hh)
        tex = [95 + 50 * np.sin(xx / 39.0 + yy / 25.0), 150 + 40 * np.cos(xx / 24.0 - yy / 51.0), 120 + 60 * np.sin((xx + yy) / 33.0)]
        return np.stack([np.clip(tex[(i // cut_every) % 3] + (i % cut_every) + r.integers(-3, 4, (hh, ww)), 0, 255) for i in range(n)]).astype(np.uint8)

    clip = np.repeat(frames(h, w)[..., None], 3, -1)
    g = np.repeat(frames(hr, wr)[..., None], 3, -1).astype(np.float32)
    tint = np.array([[1.10, 0.92, 0.70], [0.75, 1.0, 1.15], [0.95, 1.1, 0.8]], np.float32)
    ref = np.stack([np.clip(g[i] * tint[(i // cut_every) % 3] + np.float32([12, 0, 8]), 0, 255) for i in range(n)]).astype(np.uint8)
    return clip, ref


def pil_resize_dev(ctx, src, dw, dh, resample):
    out = DeviceImage(ctx, (src.shape[0], dh, dw, 3))
    nat.check(ctx.lib.havc_pil_resize_n(ctx.h, src.ptr, src.shape[2], src.shape[1], out.ptr, dw, dh, resample, src.shape[0]), ctx.h)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from vsdeoldify_amd.colormnet_net import ColorMNetNetwork
    from vsdeoldify_amd.remaster_net import RemasterColorNet
    from vsdeoldify_amd.synth import synth_colormnet_state_dict, synth_remaster_state_dict
    net = ColorMNetNetwork(synth_colormnet_state_dict(7), device_index=0)
    ctx = net.ctx                                                # one context for everything: the clips live in its pool
    stream = torch.cuda.ExternalStream(ctx.stream_ptr())
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def measure(items, reps, per=1.0):
        for f in items.values():
            for _ in range(2):
                f()
        ctx.synchronize()
        ms = {k: [] for k in items}
        for _ in range(reps):
            for k, f in items.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                f()
                e1.record(stream)
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1) / per)
        return ms

    n, h, w, hr, wr = a.frames, 1080, 1920, 540, 720
    clip, ref = make_clips(n, h, w, hr, wr)
    dclip, dref = DeviceImage.from_numpy(ctx, clip), DeviceImage.from_numpy(ctx, ref)
    say(f"HAVC_restore_video: device-resident clip {n} x {h} x {w}, reference video {n} x {hr} x {wr}; device {torch.cuda.get_device_name(0)}")
    say(f"HIP events on the context stream around each call, median of {a.reps} repetitions (min, max) after 2 warm-up calls; items of a group alternate")
    say()
    model = RemasterColorNet(synth_remaster_state_dict(5))
    n0 = min(n, 16)
    routes = {
        f"ex_model 0 ColorMNet, method 6, {n0} frames": (n0, lambda: havc.HAVC_restore_video(dclip.frames(0, n0), dref.frames(0, n0), network=net)),
        f"ex_model 2 DeepRemaster, method 6, {n} frames": (n, lambda: havc.HAVC_restore_video(dclip, dref, ex_model=2, render_vivid=False, model=model)),
        f"ex_model 2 DeepRemaster, method 5 ref_merge 2, {n} frames": (n, lambda: havc.HAVC_restore_video(dclip, dref, method=5, ex_model=2, ref_merge=2,
                                                                                                      render_vivid=False, model=model)),
    }
    ms = measure({k: v[1] for k, v in routes.items()}, a.reps)
    for k, (frames, _) in routes.items():
        med = statistics.median(ms[k])
        say(f"  {k:58s} {med:10.2f} ms a call ({min(ms[k]):.2f}, {max(ms[k]):.2f}) = {frames / med * 1e3:8.1f} frames/s")
    say()
    fw, fh = 576, 320
    for label, src, dw, dh in ((f"{n} x {hr} x {wr} -> {w} x {h}", dref, w, h), (f"{n} x {h} x {w} -> {fw} x {fh}", dclip, fw, fh)):
        ms = measure({"Spline36": lambda: havc.spline36(ctx, src, dw, dh), "Spline64": lambda: havc.spline64(ctx, src, dw, dh)}, a.reps)
        for k, v in ms.items():
            say(f"  {k} {label:34s} {statistics.median(v):9.4f} ms a call ({min(v):.4f}, {max(v):.4f}) = {statistics.median(v) / n * 1e3:8.2f} us a frame")
    say()
    say("havc_pil_resize_n CALL times, not kernel times: each call builds its two coefficient tables on the host, uploads them, launches the two passes and")
    say("synchronises the stream once")
    for nf in (1, 2, n):
        src = dclip.frames(0, nf)
        ms = measure({"LANCZOS": lambda: pil_resize_dev(ctx, src, fw, fh, 1), "BICUBIC": lambda: pil_resize_dev(ctx, src, fw, fh, 3)}, a.reps)
        for k, v in ms.items():
            say(f"  Pillow {k} call {nf:3d} x {h} x {w} -> {fw} x {fh}   {statistics.median(v):9.4f} ms a call ({min(v):.4f}, {max(v):.4f})"
                f" = {statistics.median(v) / nf * 1e3:8.2f} us a frame")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
