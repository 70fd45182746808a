"""-m gpu: the BENCHMARKED entry points at BASELINE.json's full sizes, and the generators against the golden vectors of
the executed reference.

  * havc_colorize_clip on 1080p frames (stable, rf=35, net 560x560) vs oracle.pipeline.colorize_frame_fullsize
  * havc_spline64_resize (1920x1080 -> 560x560, and back up with the fused luma re-attach) vs oracle.resample
  * wide / deep generators at 560x560 vs the oracle
  * the conv frame-chunking path (operands beyond one buffer descriptor) forced at a small size
  * HIP generators directly against tests/golden/unet_*_S80.npz and ModelImageRender against tests/golden/render_*.npz
    (vectors produced by EXECUTING the reference, tools/gen_golden.py) -- no oracle in between

Tolerances (fp16 storage + fp32 MFMA accumulation vs fp32): see tests/test_gpu_deoldify.py and profiles/r2_precision_study.txt.
At 1080p after the two-model blend and the Spline64 up-pass the measured figures are mean dE00 0.11-0.12, p99 1.2,
97 % of pixels below 1.0; the CPU simulation of the same rounding points (tests/precision_study.py) gives 0.113 / 1.19 / 97.3 %.
"""
import json
import os

import numpy as np
import pytest

from oracle import imaging, pipeline, resample
from tests import gpu_util as gu
from tests.conftest import GOLDEN
from tests.test_gpu_deoldify import FINAL_TOL, RAW_TOL, make_frame, raw_gpu, summarize
from vsdeoldify_amd import _native as nat
from vsdeoldify_amd.clip import ClipColorizer, synthetic_gray_frame
from vsdeoldify_amd.render import GeneratorRuntime, ModelImageRender
from vsdeoldify_amd.synth import synth_state_dict

pytestmark = pytest.mark.gpu

CLIP_TOL = dict(mean=0.2, p99=1.35, frac_lt1=0.965)      # 1080p output of BASELINE configs[1]


@pytest.fixture(scope="module")
def stable_sds():
    return {"video": synth_state_dict("wide", 1), "stable": synth_state_dict("wide", 2)}


def test_colorize_clip_1080p_matches_oracle(ctx, stable_sds):
    """the entry point bench.py times (havc_colorize_clip): 2 frames of the synthetic 1080p clip, DeOldify stable rf=35."""
    idx = (0, 7)                                            # (frames the precise clip test checks too: the oracle evaluates them once per session)
    frames = np.stack([synthetic_gray_frame(i, 1920, 1080) for i in idx])
    cc = ClipColorizer("stable", 35, 0.5, device_index=0, state_dicts=stable_sds, max_batch=2)
    got = cc.colorize(frames)
    assert got.shape == frames.shape and got.dtype == np.uint8
    for i, g in zip(idx, got):
        ref = gu.oracle_fullsize_stable(1, 2, i)
        de = imaging.delta_e00_images(g, ref)
        s = summarize(g, ref)
        print(f"1080p stable rf=35: mean dE00 {de.mean():.4f} p99 {np.percentile(de, 99):.3f} max {de.max():.2f} "
              f"dE<1 {float((de < 1).mean()):.5f} {s}")
        assert de.mean() < CLIP_TOL["mean"] and np.percentile(de, 99) < CLIP_TOL["p99"] and (de < 1.0).mean() > CLIP_TOL["frac_lt1"], \
            (de.mean(), np.percentile(de, 99), float((de < 1.0).mean()), s)
    # one frame alone == the same frame inside the batch (frames are independent)
    assert np.array_equal(cc.colorize(frames[1:2])[0], got[1])


def _spline(ctx, src, dw, dh, luma_from=None):
    out = np.empty((dh, dw, 3), np.uint8)
    src = np.ascontiguousarray(src)
    nat.check(ctx.lib.havc_spline64_resize(ctx.h, nat.as_ptr(src), src.shape[1], src.shape[0], nat.as_ptr(out), dw, dh,
                                           nat.as_ptr(np.ascontiguousarray(luma_from)) if luma_from is not None else None), ctx.h)
    return out


def test_spline64_resize_matches_oracle(ctx):
    """down 1920x1080 -> 560x560 and up 560x560 -> 1920x1080 with the fused chroma_post_process (vs_recover_clip_luma)."""
    frame = synthetic_gray_frame(3, 1920, 1080)
    r = np.random.default_rng(5)
    colour = np.clip(frame.astype(np.int32) + r.integers(-40, 40, frame.shape), 0, 255).astype(np.uint8)      # not gray: exercises U, V
    down = _spline(ctx, colour, 560, 560)
    ref_down = resample.resize_rgb8(colour, 560, 560)
    d = np.abs(down.astype(int) - ref_down.astype(int))
    # same taps, same accumulation order, fp32: identical up to the rare value that sits on a .5 rounding boundary
    assert d.max() <= 1 and (d > 0).mean() < 1e-4, (int(d.max()), float((d > 0).mean()))
    up = _spline(ctx, ref_down, 1920, 1080, luma_from=frame)
    ref_up = pipeline.post_process(resample.resize_rgb8(ref_down, 1920, 1080), frame)
    d = np.abs(up.astype(int) - ref_up.astype(int))
    assert d.max() <= 2 and (d > 0).mean() < 1e-4, (int(d.max()), float((d > 0).mean()))
    # odd sizes, plain copy, up-scaling without luma
    small = colour[:97, :131]
    for dw, dh in ((131, 97), (64, 64), (263, 195), (50, 200)):
        got, want = _spline(ctx, small, dw, dh), resample.resize_rgb8(small, dw, dh)
        d = np.abs(got.astype(int) - want.astype(int))
        assert d.max() <= 1 and (d > 0).mean() < 1e-3, (dw, dh, int(d.max()), float((d > 0).mean()))


@pytest.mark.parametrize("arch,seed", [("wide", 1), ("deep", 3)])
def test_generator_raw_color_560(ctx, arch, seed):
    """the net size of BASELINE configs[1] (render_factor 35): one frame, raw colour and final image."""
    sd = synth_state_dict(arch, seed)
    rt = GeneratorRuntime(ctx, sd, arch)
    try:
        f = make_frame(560, 560)
        got = raw_gpu(ctx, rt, f[None])[0]
        ref = pipeline.raw_color_square(sd, arch, f)
        s, de = summarize(got, ref), imaging.delta_e00_images(got, ref)
        de2 = imaging.delta_e00_images(pipeline.post_process(got, f), pipeline.post_process(ref, f))
        print(f"{arch} 560: raw {s} mean {de.mean():.4f} p99 {np.percentile(de, 99):.3f} | final mean {de2.mean():.4f} p99 {np.percentile(de2, 99):.3f}")
        assert s["within1"] >= RAW_TOL["within1"] and s["within2"] >= RAW_TOL["within2"] and de.mean() < RAW_TOL["mean"] and \
            np.percentile(de, 99) < RAW_TOL["p99"], (s, de.mean(), np.percentile(de, 99))
        assert de2.mean() < FINAL_TOL["mean"] and np.percentile(de2, 99) < FINAL_TOL["p99"], (de2.mean(), np.percentile(de2, 99))
    finally:
        rt.close()


def test_conv_frame_chunking_is_bit_identical():
    """Convs whose operands exceed one buffer descriptor run as several frame chunks (rt_net.cpp run_op; batch >= 23 at
    560x560).  HAVC_DESC_LIMIT_BYTES lowers the limit of a NEW context so that a 3-frame batch at 96x96 is issued frame by frame
    for the big layers; the bytes must equal the single-launch result."""
    _conv_frame_chunking(str(96 * 96 * 320 * 2 + 4096), None)    # one frame of the 320-pitch tail buffer (+ slack) per launch


def test_conv_frame_chunking_is_bit_identical_precise(ctx):
    """the same in the default mode: precise pixel rows are twice as wide (hi | lo), so chunking sets in at half the batch; the lowered limit is one
    frame of the PRECISE plan's own tail buffer (+ slack), read from the plan"""
    rt = gu.generator_runtime(ctx, synth_state_dict("wide", 1), "wide", "precise")      # the session's packed precise generator; only its plan is needed here
    gen = rt.gen
    rt.close()
    ops, _, _, _, names = gen.plan(96)
    tail_pitch = int(ops[names.index("layers.10.layers.0.0")]["dst_cpitch"])
    assert gen.precise and tail_pitch == 2 * 320
    _conv_frame_chunking(str(96 * 96 * tail_pitch * 2 + 4096), gen)


def _conv_frame_chunking(limit_bytes, generator):
    sd = synth_state_dict("wide", 1)
    frames = np.stack([make_frame(96, s) for s in (21, 22, 23)])
    outs = []
    for limit in (None, limit_bytes):
        if limit:
            os.environ["HAVC_DESC_LIMIT_BYTES"] = limit
        try:
            c = nat.Context(0)
        finally:
            os.environ.pop("HAVC_DESC_LIMIT_BYTES", None)
        rt = GeneratorRuntime(c, sd, "wide") if generator is None else GeneratorRuntime(c, None, "wide", generator=generator, precision="precise")
        try:
            assert generator is None or all(int(o["flags"]) & nat.F_PRECISE for o in rt.net(96, 3).ops)
            c.reset_stats()
            outs.append((raw_gpu(c, rt, frames), c.stats().launches))
        finally:
            rt.close()
            c.close()
    assert np.array_equal(outs[0][0], outs[1][0])
    assert outs[1][1] > outs[0][1], "the lowered limit did not split any launch"


@pytest.mark.parametrize("arch", ["wide", "deep"])
def test_generator_matches_reference_golden_S80(ctx, arch):
    """HIP generator vs DynamicUnetWide/Deep.forward EXECUTED from the reference tree (tests/golden/unet_*_S80.npz, incl. the
    odd-size nearest branch): the golden normalised input goes straight into the plan's activation buffers (the prep op
    is skipped), the u8 output is compared with image2np(denorm(y) * 255) of the golden output."""
    g = np.load(os.path.join(GOLDEN, f"unet_{arch}_S80.npz"))
    sd = synth_state_dict(arch, int(g["seed"]))
    rt = GeneratorRuntime(ctx, sd, arch)
    try:
        S = 80
        net = rt.net(S, 1)
        prep = net.ops[0]
        assert prep["type"] == nat.OP_PREP_RGB8
        x = np.transpose(g["x"][0], (1, 2, 0))                                     # [S,S,3] normalised fp32
        x0 = np.zeros((S, S, int(prep["dst_cpitch"])), np.float16)
        x0[..., int(prep["dst_coff"]):int(prep["dst_coff"]) + 3] = x
        net.upload(int(prep["dst"]), x0)
        tail = np.zeros((S, S, int(prep["res_cpitch"])), np.float16)
        tail[..., int(prep["res_coff"]):int(prep["res_coff"]) + 3] = x
        net.upload(int(prep["src2"]), tail)
        net.run_ops(1, len(net.ops) - 1, 1)
        got = net.download(net.out_buf, (S, S, 3), np.uint8)
        ref = imaging.model_output_u8(g["y"][0])
        s, de = summarize(got, ref), imaging.delta_e00_images(got, ref)
        # The golden input is white noise in all three channels (not a gray image): measured within1 0.986-0.989, mean dE00
        # 0.09-0.17, p99 0.6-1.8; the CPU simulation of the HIP rounding points (tests/precision_study.py forward()) gives
        # 0.986-0.991 / 0.11-0.13 / 0.6-1.2 on the same vectors.
        assert s["within1"] >= 0.98 and s["within2"] >= 0.993 and de.mean() < RAW_TOL["mean"] and np.percentile(de, 99) < 2.0, \
            (s, de.mean(), np.percentile(de, 99))
    finally:
        rt.close()


@pytest.mark.parametrize("modelname", ["video", "stable", "artistic"])
def test_model_image_render_matches_reference_golden(ctx, modelname):
    """ModelImageRender drop-in vs the reference's OWN ModelImageRender.get_transformed_image (weights through Learner.load from
    .pth files; tests/golden/render_*.npz), post-process on and off."""
    from PIL import Image
    g = np.load(os.path.join(GOLDEN, f"render_{modelname}.npz"))
    seeds = json.loads(str(g["seeds"]))
    sds = {"video": synth_state_dict("wide", seeds["video"])}
    if modelname == "stable":
        sds["stable"] = synth_state_dict("wide", seeds["stable"])
    if modelname == "artistic":
        sds["artistic"] = synth_state_dict("deep", seeds["artistic"])
    r = ModelImageRender(None, modelname, int(g["render_factor"]), float(g["video_weight"]), state_dicts=sds)
    for post, ref in ((True, g["out"]), (False, g["out_nopp"])):
        got = np.asarray(r.get_transformed_image(Image.fromarray(g["img"]), post_process=post))
        de = imaging.delta_e00_images(got, ref)
        tol = FINAL_TOL if post else dict(mean=RAW_TOL["mean"], p99=RAW_TOL["p99"])
        assert got.shape == ref.shape and de.mean() < tol["mean"] and np.percentile(de, 99) < tol["p99"], \
            (post, de.mean(), np.percentile(de, 99), summarize(got, ref))
