#!/usr/bin/env python3
"""How far apart are precision="fast" and precision="precise" on this footage?  Colours a clip with one DeOldify model in both arithmetics and prints
clip_delta_e of the two results: per frame and for the clip, mean, max, the share of pixels below the contract's 1.0, p99 and PSNR.  Needs an MI355X.

    python tools/precision_report.py [--model stable] [--render-factor 24] [--frames 8] [--size 480x270] [--clip frames.npy] [--package-dir DIR]

The clip is the synthetic gray clip of the benchmark (vsdeoldify_amd.clip.synthetic_gray_frame) unless --clip names a .npy of uint8 [n, h, w, 3].  The weights
are the checkpoints under --package-dir (<dir>/models/*.pth, as the reference lays them out) or, without it, the seeded synthetic weights the test-suite
uses.  Both renders and the metric run on device-resident clips: only the per-frame records come back."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vsdeoldify_amd import clip_delta_e  # noqa: E402
from vsdeoldify_amd.clip import ClipColorizer, synthetic_gray_frame  # noqa: E402
from vsdeoldify_amd.device import DeviceImage  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="stable", choices=["video", "stable", "artistic"])
    ap.add_argument("--render-factor", type=int, default=24)
    ap.add_argument("--video-weight", type=float, default=0.5)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", default="480x270", help="WxH of the synthetic clip")
    ap.add_argument("--clip", default=None, help=".npy of uint8 [n, h, w, 3]")
    ap.add_argument("--package-dir", default=None)
    ap.add_argument("--device-index", type=int, default=0)
    a = ap.parse_args()
    if a.clip:
        frames = np.load(a.clip)
        if frames.ndim != 4 or frames.shape[-1] != 3 or frames.dtype != np.uint8:
            sys.exit(f"{a.clip}: uint8 [n, h, w, 3] expected, got {frames.dtype} {frames.shape}")
    else:
        w, h = (int(x) for x in a.size.lower().split("x"))
        frames = np.stack([synthetic_gray_frame(i, w, h) for i in range(a.frames)])
    n, h, w, _ = frames.shape
    sds = None
    if a.package_dir is None:
        from vsdeoldify_amd.synth import synth_state_dict
        sds = {"video": synth_state_dict("wide", 1), "stable": synth_state_dict("wide", 2), "artistic": synth_state_dict("deep", 3)}
    out = {}
    for mode in ("fast", "precise"):
        cc = ClipColorizer(a.model, a.render_factor, a.video_weight, a.device_index, sds, a.package_dir, max_batch=min(8, n), precision=mode)
        src = DeviceImage.from_numpy(cc.ctx, frames)
        out[mode] = DeviceImage(cc.ctx, frames.shape)
        cc.colorize_device(src.ptr, out[mode].ptr, n, w, h)
    rep = clip_delta_e(out["fast"], out["precise"], device_index=a.device_index)
    print(f"{a.model}, render_factor {a.render_factor}, {n} frames of {w} x {h}, {'seeded synthetic weights' if sds else a.package_dir}: "
          f"CIEDE2000 of precision='fast' against precision='precise'")
    print(rep.table())


if __name__ == "__main__":
    main()
