#!/usr/bin/env python3
"""DeepRemaster on a device-resident clip at the reference's operating point: frames of 320 x 576 (what resize_for_inference makes of 1920 x 1080 at
frame_mindim 320), 20 reference stills of 256 x 455 in the ring, `length` 2 and 5.  Reports, from HIP events around the enqueued ops (the library's own
timer, havc_stats.last_ms), the median of REPEATS runs after WARMUP warm-up runs:

  colorize      one call on `length` frames (the `colorize` slice: everything but the stills' encoders) -> frames/s
  stattn1       the first source-reference attention alone (N_q = length x 40 x 72 queries against 20 x 32 x 57 keys, d 64, d_v 512), with the
                share of the fp16 MFMA peak its algorithmic FLOPs (2 N_q N_k (d + d_v)) reach
  encode        one reference still through reffeatnet1 / reffeatnet2 and the key / value convs (once per still, when it enters the window)

Weights are the seeded synthetic ones (timing does not depend on their values).  Usage: python tools/remaster_bench.py [--out FILE]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP, REPEATS = 5, 25
MFMA_F16_PEAK = 2.5e15          # dense fp16 MFMA peak of the MI355X, FLOP/s (spec)
H, W, REF_HW, SLOTS = 320, 576, (256, 455), 20


def median_ms(ctx, fn):
    for _ in range(WARMUP):
        fn()
    t = []
    for _ in range(REPEATS):
        fn()
        t.append(ctx.stats().last_ms)
    return float(np.median(t)), float(np.min(t)), float(np.max(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from vsdeoldify_amd import _native as nat
    from vsdeoldify_amd.device import DeviceImage
    from vsdeoldify_amd.remaster_net import RemasterColorNet, RemasterSession
    from vsdeoldify_amd.render import get_context
    from vsdeoldify_amd.synth import synth_remaster_state_dict
    ctx = get_context(0)
    model = RemasterColorNet(synth_remaster_state_dict(5))
    weights = nat.Weights(ctx, model.blob)
    r = np.random.default_rng(0)
    lines = [f"DeepRemaster, {ctx.device_name()}: frames {H} x {W}, {SLOTS} stills of {REF_HW[0]} x {REF_HW[1]}; HIP-event times, median of {REPEATS} after {WARMUP} warm-up runs (min - max)"]
    for length in (2, 5):
        s = RemasterSession(ctx, model, length, H, W, REF_HW, SLOTS, weights=weights)
        P = s.plan
        ref = np.ascontiguousarray(r.integers(0, 256, REF_HW + (3,), dtype=np.uint8))
        for slot in range(SLOTS):
            s.encode_reference(slot, ref)
        if length == 2:
            ms = median_ms(ctx, lambda: s.encode_reference(0, ref))
            lines.append(f"encode_reference (one still, {P.encode[1]} ops): {ms[0]:.3f} ms ({ms[1]:.3f} - {ms[2]:.3f})")
        clip = DeviceImage.from_numpy(ctx, r.integers(0, 256, (length, H, W, 3), dtype=np.uint8))
        out = DeviceImage(ctx, clip.shape)
        ms = median_ms(ctx, lambda: s.colorize(clip.ptr, out.ptr))
        lines.append(f"length {length}: colorize {ms[0]:.3f} ms ({ms[1]:.3f} - {ms[2]:.3f}) = {length / ms[0] * 1e3:.1f} frames/s")
        i = P.names.index("stattn1")
        op = P.ops[i]
        flops = float(op["flops"]) * length
        s._bind(None)
        ms = median_ms(ctx, lambda: s.net.run_ops(i, 1, length))
        nq, nk = length * int(op["Hi"]) * int(op["Wi"]), int(op["kw"]) * int(op["Ho"]) * int(op["Wo"])
        lines.append(f"length {length}: stattn1 alone ({nq} queries x {nk} keys, {flops / 1e9:.1f} GFLOP) {ms[0]:.3f} ms ({ms[1]:.3f} - {ms[2]:.3f}) = "
                     f"{flops / ms[0] / 1e9:.1f} TFLOP/s = {100 * flops / (ms[0] * 1e-3) / MFMA_F16_PEAK:.2f} % of the fp16 MFMA peak ({MFMA_F16_PEAK / 1e15:.1f} PFLOP/s)")
        prof = s.net.profile(length)[P.colorize[0]:P.colorize[0] + P.colorize[1]]
        top = np.argsort(prof)[::-1][:6]
        lines.append(f"length {length}: per-op profile of colorize, sum {prof.sum():.3f} ms; largest: " +
                     ", ".join(f"{P.names[P.colorize[0] + j]} {prof[j]:.3f}" for j in top))
        s.close()
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
