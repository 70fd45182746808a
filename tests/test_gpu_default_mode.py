"""-m gpu: the package DEFAULT arithmetic ("precise", vsdeoldify_amd/precision.py) through the public entry points and against the vectors of the
EXECUTED reference (tests/golden/unet_*_S80.npz, render_*.npz) -- no oracle in between.

tests/conftest.py pins HAVC_PRECISION=fast for the session, so everything here selects the mode with the explicit precision="precise" argument (or clears
the variable where the entry point only reads the environment) and asserts that the nets it ran really are precise.  Thresholds are the two the precise
mode is specified by (tests/test_gpu_precise.py), nothing new:

  PRECISE_RAW   raw colour of a generator: >= 99.9 % of the bytes EQUAL, none off by more than 1.  The reference alone, evaluated twice in fp32 (its own
                execution vs oracle.unet on the CPU), gives 100 % / 0 LSB (wide) and 99.990 % / 1 LSB (deep) on these fixtures: a 10x margin.
  PRECISE_CLIP  final images: CIEDE2000 p99 < 1.0 and >= 99 % of the pixels below 1.0 (BASELINE.json north_star).

Every threshold test prints its figures before it asserts.  Weight seeds are the ones the suite already packs in precise form (wide 1, 2, 11, 12, 21, 22;
deep 3, 13, 23): with HAVC_SHARE_WEIGHTS the blobs are packed once per session."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import imaging, pipeline, resample
from tests.conftest import GOLDEN
from tests.test_gpu_deoldify import make_frame
from tests.test_gpu_precise import PRECISE_CLIP, PRECISE_RAW
from tests import gpu_util as gu
from vsdeoldify_amd import _native as nat
from vsdeoldify_amd.render import ModelImageRender
from vsdeoldify_amd.synth import synth_ddcolor_state_dict, synth_state_dict, synth_zhang_state_dict

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def check_raw(got, ref, what):
    d = np.abs(got.astype(int) - ref.astype(int))
    eq, mx = float((d == 0).mean()), int(d.max())
    print(f"{what}: bytes equal {eq:.6f}, max |d| {mx} LSB")
    assert got.shape == ref.shape and eq >= PRECISE_RAW["equal"] and mx <= PRECISE_RAW["max_lsb"], (what, eq, mx)


def check_clip(got, ref, what):
    de = imaging.delta_e00_images(got, ref)
    p99, frac = float(np.percentile(de, 99)), float((de < 1.0).mean())
    print(f"{what}: mean dE00 {de.mean():.5f} p99 {p99:.4f} below 1.0 {frac:.5f} max {de.max():.2f}")
    assert got.shape == ref.shape and p99 < PRECISE_CLIP["p99"] and frac >= PRECISE_CLIP["frac_lt1"], (what, p99, frac)


def precise_nets(render):
    return all(rt.gen.precise for rt in (render._video, render._second) if rt is not None)


# ---- 1. executed-reference fixtures ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", ["wide", "deep"])
def test_precise_generator_matches_reference_golden_S80(ctx, arch):
    """tests/test_gpu_fullsize.py test_generator_matches_reference_golden_S80 in the default mode: the golden normalised fp32 input goes into the prep
    op's two destinations as hi / lo pairs (the prep op is skipped), the u8 output is compared with image2np(denorm(y) * 255) of the golden output"""
    g = np.load(os.path.join(GOLDEN, f"unet_{arch}_S80.npz"))
    rt = gu.generator_runtime(ctx, synth_state_dict(arch, int(g["seed"])), arch, "precise")
    try:
        assert rt.gen.precise
        S = 80
        net = rt.net(S, 1)
        prep = net.ops[0]
        assert prep["type"] == nat.OP_PREP_RGB8 and int(prep["flags"]) & nat.F_PRECISE
        hi, lo = gu.hl_split(np.transpose(g["x"][0], (1, 2, 0)))                    # [S,S,3] normalised fp32 -> pair
        for buf, pitch, coff in ((prep["dst"], prep["dst_cpitch"], prep["dst_coff"]), (prep["src2"], prep["res_cpitch"], prep["res_coff"])):
            pitch, coff = int(pitch), int(coff)
            img = np.zeros((S, S, pitch), np.float16)                               # pixel row = [hi: pitch / 2 | lo: pitch / 2]
            img[..., coff:coff + 3] = hi
            img[..., pitch // 2 + coff:pitch // 2 + coff + 3] = lo
            net.upload(int(buf), img)
        net.run_ops(1, len(net.ops) - 1, 1)
        got = net.download(net.out_buf, (S, S, 3), np.uint8)
        check_raw(got, imaging.model_output_u8(g["y"][0]), f"precise {arch} generator vs executed reference, S = 80")
    finally:
        rt.close()


def _golden_render(modelname):
    g = np.load(os.path.join(GOLDEN, f"render_{modelname}.npz"))
    seeds = json.loads(str(g["seeds"]))
    sds = {"video": synth_state_dict("wide", seeds["video"])}
    if modelname == "stable":
        sds["stable"] = synth_state_dict("wide", seeds["stable"])
    if modelname == "artistic":
        sds["artistic"] = synth_state_dict("deep", seeds["artistic"])
    return g, sds


@pytest.mark.parametrize("modelname", ["video", "stable", "artistic"])
def test_precise_model_image_render_matches_reference_golden(ctx, modelname):
    """ModelImageRender(precision="precise") vs the reference's OWN ModelImageRender.get_transformed_image (tests/golden/render_*.npz): raw colour at
    PRECISE_RAW (the CPU oracle is 100 % equal on all three), the final image at PRECISE_CLIP, and the integer stages exactly: post_process of the GPU's own
    per-model raw colours, blended like get_transformed_image composes them (visualize.py:118-137), is the GPU's final image byte for byte."""
    from PIL import Image
    g, sds = _golden_render(modelname)
    w = float(g["video_weight"])
    r = ModelImageRender(None, modelname, int(g["render_factor"]), w, state_dicts=sds, precision="precise")
    assert precise_nets(r) and r._precision == "precise"
    img = g["img"]
    nopp = np.asarray(r.get_transformed_image(Image.fromarray(img), post_process=False))
    check_raw(nopp, g["out_nopp"], f"precise render {modelname}, post_process=False, vs executed reference")
    post = np.asarray(r.get_transformed_image(Image.fromarray(img), post_process=True))
    check_clip(post, g["out"], f"precise render {modelname}, post_process=True, vs executed reference")
    raw_v, raw_s = r._raw_colors(img)                                                # each model alone, no post-process
    if raw_s is None:
        assert np.array_equal(raw_v, nopp)
        want = pipeline.post_process(nopp, img)
    else:
        assert np.array_equal(imaging.pil_blend(raw_s, raw_v, w), nopp)
        want = imaging.pil_blend(pipeline.post_process(raw_s, img), pipeline.post_process(raw_v, img), w)
    assert np.array_equal(post, want), int(np.abs(post.astype(int) - want.astype(int)).max())


# ---- 2. low latency in the default mode ----------------------------------------------------------------------------------------------------
def test_precise_low_latency_is_the_batched_plan(ctx, monkeypatch):
    """No split-K plan exists in precise form (deoldify_net.DeoldifyGenerator.plan, render.GeneratorRuntime.net): low_latency=True must not change a byte,
    and no op of its nets carries a split-K count."""
    from PIL import Image
    sds = {"video": synth_state_dict("wide", 1), "stable": synth_state_dict("wide", 2)}
    rf = 6
    img = make_frame(rf * 16, 9)
    monkeypatch.delenv("HAVC_LOW_LATENCY", raising=False)
    base = ModelImageRender(None, "stable", rf, 0.5, state_dicts=sds, precision="precise")
    low = ModelImageRender(None, "stable", rf, 0.5, state_dicts=sds, precision="precise", low_latency=True)
    assert low._low_latency and not base._low_latency and precise_nets(base) and precise_nets(low)
    try:
        a = np.asarray(base.get_transformed_image(Image.fromarray(img)))
        b = np.asarray(low.get_transformed_image(Image.fromarray(img)))
        assert np.array_equal(a, b)
        for rt in (low._video, low._second):
            assert set(rt.nets) == {(rf * 16, 1)}, list(rt.nets)                    # the ordinary net key: no (S, max_batch, True) low-latency net was built
            net = rt.net(rf * 16, 1, True)
            assert not any((int(o["flags"]) >> 16) & 15 for o in net.ops if o["type"] == nat.OP_CONV)
            assert all(int(o["flags"]) & nat.F_PRECISE for o in net.ops)
            assert not any("split" in n.lower() for n in net.names)
        check_clip(b, pipeline.model_image_render(sds, "stable", img, rf, 0.5), "precise low_latency render vs oracle")
    finally:
        for r in (base, low):
            for rt in (r._video, r._second):
                rt.close()


# ---- 3. weight files in the default mode ---------------------------------------------------------------------------------------------------
def test_precise_model_image_render_reads_pth_and_havc_files(ctx, tmp_path):
    """tests/test_gpu_configs.py test_model_image_render_reads_pth_and_havc_files with precision="precise": both Learner.save layouts, then a deployment that
    ships only the converted blob -- which has to be a PRECISE blob (tools/convert_weights.py --precision); a fast blob alone is refused with a message that
    names both modes; a fast and a precise render on the same files in one process never share a blob."""
    from PIL import Image
    from tests.test_gpu_configs import _save_pth
    sds = {"video": synth_state_dict("wide", 1), "stable": synth_state_dict("wide", 2)}
    models = tmp_path / "models"
    models.mkdir()
    _save_pth(str(models / "ColorizeVideo_gen.pth"), sds["video"], "learner")
    _save_pth(str(models / "ColorizeStable_gen.pth"), sds["stable"], "bare")
    rf = 6
    r = np.random.default_rng(5)
    img = np.clip(128 + 45 * r.standard_normal((rf * 16, rf * 16, 1)), 0, 255).astype(np.uint8).repeat(3, -1)
    pil = Image.fromarray(img)

    def colour(package_dir, precision, **kw):
        mir = ModelImageRender(package_dir, "stable", rf, 0.5, precision=precision, **kw)
        assert precise_nets(mir) == (precision == "precise") and mir._video.gen.precise == (precision == "precise")
        return np.asarray(mir.get_transformed_image(pil)), mir
    want = {p: colour(None, p, state_dicts=sds)[0] for p in ("precise", "fast")}
    assert not np.array_equal(want["precise"], want["fast"])
    from_pth, _ = colour(str(tmp_path), "precise")
    assert np.array_equal(from_pth, want["precise"])
    check_clip(from_pth, pipeline.model_image_render(sds, "stable", img, rf, 0.5), "precise render from .pth files vs oracle")
    # the same files, the other mode, the same process: the cache key carries the precision
    assert np.array_equal(colour(str(tmp_path), "fast")[0], want["fast"])
    assert np.array_equal(colour(str(tmp_path), "precise")[0], want["precise"])
    conv = [sys.executable, os.path.join(ROOT, "tools", "convert_weights.py"), str(models / "ColorizeStable_gen.pth")]
    subprocess.check_call(conv + [str(tmp_path / "fast.havc"), "--precision", "fast"])
    subprocess.check_call(conv + ["--precision", "precise"])
    packed = models / "ColorizeStable_gen.havc"
    assert packed.is_file()
    os.remove(models / "ColorizeStable_gen.pth")                              # a deployment that ships only the converted blob
    only_havc, mir = colour(str(tmp_path), "precise")
    assert mir._second.gen.pack is None, "the stable model was not read from the packed file"
    assert np.array_equal(only_havc, want["precise"])
    with pytest.raises(FileNotFoundError) as e:                                # a precise blob alone cannot serve the fast mode ...
        colour(str(tmp_path), "fast")
    assert "'precise'" in str(e.value) and "'fast'" in str(e.value)
    os.replace(tmp_path / "fast.havc", packed)
    with pytest.raises(FileNotFoundError) as e:                                # ... nor a fast blob alone the default mode
        colour(str(tmp_path), "precise")
    assert "holds a 'fast' blob" in str(e.value) and "precision='precise'" in str(e.value), str(e.value)
    only_fast, mir = colour(str(tmp_path), "fast")
    assert mir._second.gen.pack is None and np.array_equal(only_fast, want["fast"])


def test_precise_ddcolor_render_reads_the_checkpoint_file(ctx, tmp_path):
    """DDColorRender(model_dir=..., precision="precise") == the same render from the state dict"""
    import torch
    from vsdeoldify_amd.ddcolor import DDColorRender
    small = dict(depths=(1, 1, 2, 1), dec_layers=2)
    sd = synth_ddcolor_state_dict(2, **small)
    torch.save({"params": {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}}, str(tmp_path / "ddcolor_artistic.pth"))
    r = np.random.default_rng(6)
    frame = np.clip(128 + 45 * r.standard_normal((96, 96, 1)), 0, 255).astype(np.uint8).repeat(3, -1)
    a = DDColorRender(model=1, input_size=96, state_dict=sd, precision="precise", **small)
    b = DDColorRender(model=1, input_size=96, model_dir=str(tmp_path), precision="precise", **small)
    try:
        assert a.rt.gen.precise and b.rt.gen.precise
        assert np.array_equal(a.colorize_frame(frame), b.colorize_frame(frame))
    finally:
        a.rt.close(); b.rt.close()


# ---- 4. HAVC_colorizer / HAVC_merge in the default mode ------------------------------------------------------------------------------------
def _havc_case():
    from tests.test_havc_harness import oracle_method_case
    return oracle_method_case()


def _precise_colorizer(method, w_merge, c):
    from tests.test_havc_harness import HUE_ADJ, SMALL_DD
    from vsdeoldify_amd import havc
    col = havc.HAVCFrameColorizer(method=method, mweight=w_merge, deoldify_p=(0, c["rf"], 1.0, 0.0), ddcolor_p=(1, c["rf"], 1.0, 0.0, True), state_dicts=c["sds"],
                                  ddcolor_state_dict=c["dsd"], ddcolor_kwargs=SMALL_DD, ddtweak_p=(havc.DEF_TWEAK_p, HUE_ADJ), precision="precise")
    assert col.precision == "precise"
    return col


@pytest.mark.parametrize("method", [0, 1, 2, 3, 4, 5, 6, 7])
def test_precise_gpu_frame_matches_oracle_graph(ctx, method):
    """HAVCFrameColorizer(precision="precise"), methods 0 - 7: (a) the oracle graph fed with the GPU's own model outputs reproduces the frame (<= 1 LSB on
    < 2e-4 of the bytes: Spline64 .5 ties), (b) end to end against the all-oracle graph at PRECISE_CLIP.  The merge rules do not amplify the model noise the
    precise mode may have (tests/test_havc_harness.py test_merge_rules_do_not_amplify_admissible_model_noise, CPU: every method passes), so (b) is asserted on
    every pixel."""
    from oracle import tweaks
    from tests.test_havc_harness import HUE_ADJ
    c = _havc_case()
    w_merge, frame, sq, rf = 0.4, c["frame"], c["sq"], c["rf"]
    col = _precise_colorizer(method, w_merge, c)
    got = col.colorize(frame)
    assert got.shape == frame.shape and got.dtype == np.uint8
    if method != 1:
        assert precise_nets(col._deoldify_render())
    if method != 0:
        assert col._ddcolor.rt.gen.precise and col._ddcolor.precision == "precise"

    def graph(a, b):
        m = pipeline.combine_models(a, b, method, w_merge)
        return pipeline.post_process(resample.resize_rgb8(m, frame.shape[1], frame.shape[0]), frame)
    a_gpu = col._deoldify_render().render_square_batch(sq[None])[0] if method != 1 else None
    b_gpu = tweaks.adjust_hue_range(col._ddcolor_clip(sq[None], (rf // 2) * 32)[0], HUE_ADJ) if method != 0 else None
    d = np.abs(got.astype(int) - graph(a_gpu, b_gpu).astype(int))
    assert d.max() <= 1 and (d > 0).mean() < 2e-4, (method, int(d.max()), float((d > 0).mean()))
    check_clip(got, graph(c["a"] if method != 1 else None, c["b"] if method != 0 else None), f"precise HAVC method {method} vs all-oracle graph")


@pytest.mark.parametrize("with_luma", [False, True])
def test_havc_merge_of_precise_model_outputs(ctx, with_luma):
    """HAVC_merge (method 5) on the two PRECISE model outputs of the frame, with and without a hi-res luma source, against the same merge of the oracle's two
    model outputs: PRECISE_CLIP; and exactly the oracle's merge of the GPU's own two outputs (Spline64 .5 ties excepted)."""
    import math
    from oracle import tweaks
    from tests.test_havc_harness import HUE_ADJ
    from vsdeoldify_amd import havc
    c = _havc_case()
    col = _precise_colorizer(5, 0.6, c)
    sq, rf = c["sq"], c["rf"]
    a_gpu = col._deoldify_render().render_square_batch(sq[None])[0]
    b_gpu = tweaks.adjust_hue_range(col._ddcolor_clip(sq[None], (rf // 2) * 32)[0], HUE_ADJ)
    assert precise_nets(col._deoldify_render()) and col._ddcolor.rt.gen.precise
    luma = resample.resize_rgb8(c["frame"], 400, 300) if with_luma else None
    got = np.asarray(havc.HAVC_merge(a_gpu, b_gpu, clip_luma=luma, weight=0.6, method=5))

    def merge(a, b):
        if luma is None:
            return pipeline.combine_models(a, b, 5, 0.6)
        fs = min(min(max(math.trunc(0.4 * luma.shape[1] / 16), 16), 32) * 16, luma.shape[1])
        m = pipeline.combine_models(resample.resize_rgb8(a, fs, fs), resample.resize_rgb8(b, fs, fs), 5, 0.6)
        return pipeline.post_process(resample.resize_rgb8(m, luma.shape[1], luma.shape[0]), luma)
    d = np.abs(got.astype(int) - merge(a_gpu, b_gpu).astype(int))
    assert d.max() <= 2 and (d > 0).mean() < 1e-3 and (luma is not None or d.max() == 0), (with_luma, int(d.max()), float((d > 0).mean()))
    check_clip(got, merge(c["a"], c["b"]), f"HAVC_merge method 5 of precise model outputs, luma source: {with_luma}")


def test_havc_colorizer_function_resolves_to_precise_without_a_switch(ctx, monkeypatch):
    """HAVC_colorizer(**harness) reads only the environment when no precision is given (havc.py): with HAVC_PRECISION unset, a call on an EMPTY colorizer
    cache builds its graph through the no-argument path of HAVCFrameColorizer -- the package default, precise nets -- and a graph built afterwards with
    precision="precise" (another object: the cache is cleared in between) returns the same bytes"""
    from tests.test_havc_harness import SMALL_DD, _frame, _weights
    from vsdeoldify_amd import havc
    sds, dsd = _weights()
    frame = _frame(9, 80, 120)
    kw = dict(method=2, mweight=0.5, deoldify_p=(0, 5, 1.0, 0.0), ddcolor_p=(1, 10, 1.0, 0.0, True), state_dicts=sds, ddcolor_state_dict=dsd, ddcolor_kwargs=SMALL_DD)
    built = []
    init = havc.HAVCFrameColorizer.__init__

    def recording_init(self, *a, **k):
        built.append((self, k.get("precision")))
        return init(self, *a, **k)
    monkeypatch.setattr(havc.HAVCFrameColorizer, "__init__", recording_init)
    havc._colorizers.clear()
    try:
        monkeypatch.delenv("HAVC_PRECISION", raising=False)
        default = havc.HAVC_colorizer(frame, **kw)                                   # first call, empty cache, no switch anywhere
        (col_default,) = havc._colorizers.values()
        assert len(built) == 1 and built[0] == (col_default, None), "the call without a switch did not build its own graph without a precision argument"
        assert col_default.precision == "precise" and precise_nets(col_default._deoldify_render()) and col_default._ddcolor.rt.gen.precise
        assert col_default._ddcolor.precision == "precise"
        assert np.array_equal(havc.HAVC_colorizer(frame, **kw), default) and len(built) == 1          # the same call again is served by that graph
        havc._colorizers.clear()
        monkeypatch.setenv("HAVC_PRECISION", "fast")                                 # the explicit argument wins over the environment
        explicit = havc.HAVC_colorizer(frame, precision="precise", **kw)
        (col_explicit,) = havc._colorizers.values()
        assert len(built) == 2 and built[1] == (col_explicit, "precise") and col_explicit is not col_default
        assert col_explicit.precision == "precise" and precise_nets(col_explicit._deoldify_render()) and col_explicit._ddcolor.rt.gen.precise
        assert np.array_equal(default, explicit)
        fast = havc.HAVC_colorizer(frame, **kw)                                      # and the environment alone selects the speed mode: a third graph
        (col_fast,) = havc._colorizers.values()
        assert len(built) == 3 and col_fast is built[2][0] and col_fast.precision == "fast"
        assert not precise_nets(col_fast._deoldify_render()) and not np.array_equal(fast, explicit)
    finally:
        havc._colorizers.clear()


# ---- 5. Zhang and DDColor entry shapes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["eccv16", "siggraph17"])
@pytest.mark.parametrize("hw", [(135, 240), (300, 200)])
def test_precise_model_colorization_frame_sizes(ctx, model, hw):
    """ModelColorization(precision="precise").colorize_frame on frames that are not 256 x 256 (BICUBIC squash of L, BILINEAR stretch of ab inside the
    library) vs oracle/zhang.colorize_frame at PRECISE_CLIP"""
    import torch
    from oracle import zhang
    from tests.test_zhang import frame
    from vsdeoldify_amd.colorization import ModelColorization
    sd = synth_zhang_state_dict(model, 7)
    mc = ModelColorization(model, True, state_dict=sd, precision="precise")
    try:
        assert mc.precision == "precise" and mc.gen.precise
        img = frame(hw[0], hw[1], 77)
        got = mc.colorize_frame(img)
        check_clip(got, zhang.colorize_frame({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, model, img), f"precise zhang {model} {hw}")
    finally:
        mc.close()


def test_precise_ddcolor_rgbs_rgbh_call_shape(ctx):
    from tests.test_gpu_boundary import ddcolor_rgbs_rgbh_call_shape
    ddcolor_rgbs_rgbh_call_shape("precise")
