"""-m gpu: the fused epilogue of the second tail conv (HAVC_F_FUSE_RGB8: 259 -> 259 3x3 conv + ReLU + residual + layers.11 1x1 -> 3 + SigmoidRange -> u8),
op by op.

Its residual reaches the accumulator fragments through the wave-private LDS image (16-byte loads, eight lanes per 128-byte line, read back in fragment
layout): a routing change only, so every check here is about bytes.

  * fused op against the unfused two-op chain (conv + ReLU + residual -> fp16 r2, then the 1x1 conv with the RGB8 epilogue): the tolerance of
    tests/test_gpu_deoldify.py::test_fused_final_conv_matches_unfused -- max 1 LSB, > 99.9 % of the bytes equal (same rounding points: fp16 r2, fp16
    weights, fp32 accumulation; only the summation order of the 259-term dot differs);
  * fused op against a float64 evaluation with the documented rounding points (conv result -> fp16, + residual -> fp16, layers.11 weights -> fp16,
    truncation to u8).  What may differ is the fp32 accumulation of the 2 331-term conv dot: it is ~3e-6 away from the exact sum (sqrt(2331) x 2^-24 x the
    O(1) partial sums), so an r2 value of magnitude ~1 (fp16 ulp 2^-10) rounds the other way with probability ~6e-3; of a pixel's 259 channels ~1.5 do,
    each moving the logit by ulp x |w11| ~ 1e-3 x 0.06.  A logit error of ~1e-4 times the steepest slope of the output map (255 x 0.229 x 6 / 4 = 88 LSB
    per unit logit) flips the truncation of < 1 % of the bytes, by one LSB.  Bound: max 1 LSB, >= 97 % of the bytes equal (3 x that estimate).
  * a batch of 3 equals three single-frame calls byte for byte; a whole generator at S = 32 fused against unfused.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import gpu_util as gu
from vsdeoldify_amd import _native as nat
from vsdeoldify_amd.deoldify_net import Y_RANGE
from vsdeoldify_amd.plan import PlanBuilder, View, WeightPack, pack_conv, pad_to, pitch_for

pytestmark = pytest.mark.gpu

C = 259
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def h16(a):
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


def make_case(B, H, W, seed):
    r = np.random.default_rng(seed)
    return dict(x=h16(0.5 * r.standard_normal((B, C, H, W))), res=h16(0.5 * r.standard_normal((B, C, H, W))),
                w=h16(r.standard_normal((C, C, 3, 3)) / np.sqrt(C * 9)), bias=(0.3 * r.standard_normal(C)).astype(np.float32),
                w11=(r.standard_normal((3, C)) / np.sqrt(C)).astype(np.float32), b11=(0.2 * r.standard_normal(3)).astype(np.float32))


def run_tail(ctx, case, fused, res_coff=0):
    """the op (fused) or the two-op chain (unfused) on `case` -> uint8 [B, H, W, 3].  res_coff: the residual is a view at this channel offset of a wider buffer"""
    x, res = case["x"], case["res"]
    B, _, H, W = x.shape
    pack, b = WeightPack(), PlanBuilder()
    xv = b.tensor(H, W, C)
    span = pad_to(C, 8)
    rpitch = pitch_for(res_coff + span)
    rv = View(b.buf(H * W * rpitch), res_coff, rpitch, H, W, C, span)
    rgb = b.buf(H * W * 3, 1)
    pc = pack_conv(pack, case["w"], xv.cmap, xv.span, bias=case["bias"])
    assert pc.Npad == 272
    if fused:
        fw = np.zeros((3, pc.Npad), np.float32)
        fw[:, :C] = case["w11"]
        fw_off, fb_off = pack.add(fw), pack.add(case["b11"])
        oi = b.conv("tail+11", pc, xv, b.tensor(H, W, C), pad=1, flags=nat.F_RELU_PRE | nat.F_RESIDUAL | nat.F_FUSE_RGB8, res=rv,
                    f=(Y_RANGE[0], Y_RANGE[1], 0, 0), aux0=rgb)
        b.ops[oi]["scale_off"], b.ops[oi]["shift_off"] = fw_off, fb_off
    else:
        r2 = b.tensor(H, W, C)
        b.conv("tail", pc, xv, r2, pad=1, flags=nat.F_RELU_PRE | nat.F_RESIDUAL, res=rv)
        pc11 = pack_conv(pack, case["w11"][:, :, None, None], r2.cmap, r2.span, bias=case["b11"])
        b.conv("11", pc11, r2, rgb, flags=nat.F_OUT_RGB8, f=(Y_RANGE[0], Y_RANGE[1], 0, 0), Co=3)
    rbuf = np.zeros((B, H, W, rpitch), np.float16)
    rbuf[..., res_coff:res_coff + C] = res.transpose(0, 2, 3, 1)
    rbuf[..., :res_coff] = 7.0                                    # what lies in front of the view must not be read
    ups = {xv.buf: gu.nhwc_pad(x, xv.cpitch), rv.buf: rbuf}
    return gu.run_plan(ctx, pack, b, ups, {rgb: ((B, H, W, 3), np.uint8)}, B)[rgb]


def reference_f64(case):
    """float64 with the rounding points of the fused epilogue: fp16(ReLU(conv + bias)), fp16(. + residual), fp16 layers.11 weights, truncation"""
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    v = F.relu(F.conv2d(t(case["x"]), t(case["w"]), t(case["bias"]), 1, 1)).numpy()
    r2 = h16(h16(v).astype(np.float64) + case["res"]).astype(np.float64)
    logit = np.einsum("bchw,jc->bhwj", r2, h16(case["w11"]).astype(np.float64)) + case["b11"].astype(np.float64)
    s = 1.0 / (1.0 + np.exp(-logit))
    s = s * (Y_RANGE[1] - Y_RANGE[0]) + Y_RANGE[0]
    s = np.clip(s * np.asarray(STD) + np.asarray(MEAN), 0.0, 1.0)
    return (s * 255.0).astype(np.int32).astype(np.uint8)


# 16 x 16, batch 1: one full 256-pixel tile; 24 x 20, batch 3: M = 1440 = 5 tiles + 160 rows (ragged last tile, tiles that straddle frames);
# 16 x 16, batch 2 with the residual a view at channel offset 8 of a wider buffer
SHAPES = [(1, 16, 16, 0), (3, 24, 20, 0), (2, 16, 16, 8)]
_cache = {}


def outputs(ctx, shape):
    """(case, fused bytes, unfused bytes, float64 bytes) of a shape: computed once, shared by the tests, never modified"""
    if shape not in _cache:
        B, H, W, coff = shape
        case = make_case(B, H, W, 100 + H + B)
        _cache[shape] = (case, run_tail(ctx, case, True, coff), run_tail(ctx, case, False, coff), reference_f64(case))
    return _cache[shape]


def diff_stats(a, b):
    d = np.abs(a.astype(np.int32) - b.astype(np.int32))
    return int(d.max()), float((d == 0).mean())


@pytest.mark.parametrize("shape", SHAPES, ids=[str(s) for s in SHAPES])
def test_fused_tail_op_matches_the_two_op_chain(ctx, shape):
    _, fused, unfused, _ = outputs(ctx, shape)
    mx, eq = diff_stats(fused, unfused)
    print(f"fused vs two-op chain {shape}: max {mx} LSB, {eq:.5f} of the bytes equal")
    assert fused.std() > 10, "degenerate output"
    assert mx <= 1 and eq > 0.999, (mx, eq)


@pytest.mark.parametrize("shape", SHAPES, ids=[str(s) for s in SHAPES])
def test_fused_tail_op_matches_float64_with_its_rounding_points(ctx, shape):
    _, fused, _, ref = outputs(ctx, shape)
    mx, eq = diff_stats(fused, ref)
    print(f"fused vs float64 {shape}: max {mx} LSB, {eq:.5f} of the bytes equal")
    assert mx <= 1 and eq >= 0.97, (mx, eq)


def test_fused_tail_op_is_batch_independent(ctx):
    case, fused, _, _ = outputs(ctx, SHAPES[1])
    for i in range(3):
        one = {k: (v[i:i + 1] if k in ("x", "res") else v) for k, v in case.items()}
        assert np.array_equal(run_tail(ctx, one, True), fused[i:i + 1]), f"frame {i} differs between a batch of 3 and a single-frame call"


def test_generator_with_fused_tail_matches_unfused_at_32(ctx):
    from tests.test_gpu_deoldify import make_frame, raw_gpu
    from vsdeoldify_amd.render import GeneratorRuntime
    from vsdeoldify_amd.synth import synth_state_dict
    frames = np.stack([make_frame(32, 5), make_frame(32, 6)])
    outs = []
    for fuse in (True, False):
        rt = GeneratorRuntime(ctx, synth_state_dict("wide", 1), "wide", fuse_final=fuse)
        try:
            names = rt.net(32, 2).names
            assert ("layers.11.0" in names) != fuse and ("layers.10.layers.1.0+11" in names) == fuse
            outs.append(raw_gpu(ctx, rt, frames))
        finally:
            rt.close()
    mx, eq = diff_stats(outs[0], outs[1])
    print(f"generator at 32, fused vs unfused: max {mx} LSB, {eq:.5f} of the bytes equal")
    assert mx <= 1 and eq > 0.999, (mx, eq)
