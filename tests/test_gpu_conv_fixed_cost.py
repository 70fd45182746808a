"""-m gpu: the per-tile fixed work of conv_pipe_kernel that is not its main loop, byte for byte.

A. Division-free pixel index math (csrc/conv_common.h fast_div): the prologue turns a GEMM row into (frame, row, column) with a multiplier and a shift
   per launch-constant divisor; so do the pixel-shuffle stores and the shuffle + blur tile walk.  A wrong quotient is a wrong pixel, so the shapes here make
   pixel tiles cross row ends and frame ends, and include the divisor 1 (H x 1 and 1 x W maps).
B. The last K stage of a conv whose K table ends in four or more pad chunks runs its first K half only (ConvArgs::k_half_empty).  The accumulators start
   at +0 and the dropped MFMAs would add +0 products, so the bytes are those of a kernel that runs them: the register-staged kernel (configuration 1).

Reference everywhere: the register-staged conv_igemm_kernel (configuration 1), which has neither change in its main loop and divides with `/` in its own
prologue, compared BYTE FOR BYTE; the fused shuffle + blur conv against its unfused chain, as tests/test_gpu_deoldify.py does for whole generators.  On the
parent commit every shape below is byte-equal between configuration 1 and the pipelined configurations (measured with this file against the parent
library), the split-K conv among its pipelined configurations; none needed the fall-back tolerance.  The split-K conv has no register-staged form
(launch_conv sends every configuration to a pipelined tile), so it is held to tests/test_gpu_kernels.py's assert_close bound against torch's fp32
conv in addition.
"""
import numpy as np
import pytest

from tests import gpu_util as gu
from tests.test_gpu_kernels import assert_close, h16, torch_conv
from vsdeoldify_amd import _native as nat
from vsdeoldify_amd.plan import PlanBuilder, WeightPack, pack_conv

pytestmark = pytest.mark.gpu

PIPE_CFGS = (60, 61, 70, 71, 72)
COUT = 259            # Npad 272: the one width every pipelined configuration runs, the 256 x (256 + 16) tile (61) included


def case(B, Cin, k, H, W, seed, cout=COUT):
    r = np.random.default_rng(seed)
    return (h16(0.5 * r.standard_normal((B, Cin, H, W))), h16(r.standard_normal((cout, Cin, k, k)) / np.sqrt(Cin * k * k)),
            (0.3 * r.standard_normal(cout)).astype(np.float32))


def same_bytes(ctx, x, w, bias, cfgs, **kw):
    ref = gu.conv_op(ctx, x, w, bias=bias, cfg=1, **kw)[1]
    assert np.isfinite(ref).all() and ref.astype(np.float32).std() > 0.05, "degenerate reference"
    for cfg in cfgs:
        got = gu.conv_op(ctx, x, w, bias=bias, cfg=cfg, **kw)[1]
        assert np.array_equal(got.view(np.uint16), ref.view(np.uint16)), f"configuration {cfg} differs from the register-staged kernel"
    return ref


# ---- A: pixel tiles that cross row ends and frame ends ----
# (B, Cin, k, stride, pad, H, W)
A_SHAPES = [
    (3, 24, 3, 1, 1, 9, 11),        # 297 pixels: a 256-pixel tile ends inside frame 2, the 64- and 128-pixel tiles inside rows
    (3, 24, 3, 1, 1, 35, 35),       # 3 675 pixels, Ho * Wo = 1 225, Wo = 35: no tile boundary falls on a row or a frame end
    (2, 24, 3, 2, 1, 37, 21),       # stride 2: 19 x 11 outputs from a 37 x 21 map
    (2, 16, 3, 1, 1, 1, 75),        # 1 x W map: Ho * Wo == Wo
    (2, 16, 3, 1, 1, 75, 1),        # H x 1 map: divisor 1
]


@pytest.mark.parametrize("shape", A_SHAPES, ids=[str(s) for s in A_SHAPES])
def test_pixel_index_math_across_row_and_frame_ends(ctx, shape):
    B, Cin, k, stride, pad, H, W = shape
    x, w, bias = case(B, Cin, k, H, W, 7 * H + W)
    same_bytes(ctx, x, w, bias, PIPE_CFGS, stride=stride, pad=pad, flags=nat.F_RELU_PRE)


def test_pixel_shuffle_stores_on_an_odd_map(ctx):
    """1x1 conv with pixel-shuffle output, 2 frames of 17 x 20: every 16-byte store computes its own (frame, row, column)"""
    x, w, bias = case(2, 64, 1, 17, 20, 5, cout=256)
    same_bytes(ctx, x, w, bias, (60, 70, 71, 72), flags=nat.F_RELU_PRE, pixshuf=True)


def shuffle_blur(ctx, x, w, bias, fused):
    """1x1 conv + ReLU + PixelShuffle(2) + blur: the fused op (HAVC_F_PS_BLUR) or the unfused chain conv -> shuffled tensor -> blur_resize"""
    B, Cin, H, W = x.shape
    up_c = w.shape[0] // 4
    pack, b = WeightPack(), PlanBuilder()
    xv = b.tensor(H, W, Cin)
    yv = b.tensor(2 * H, 2 * W, up_c)
    pc = pack_conv(pack, w, xv.cmap, xv.span, bias=bias, pixshuf="blur" if fused else True)
    if fused:
        b.conv("shuf+blur", pc, xv, yv, flags=nat.F_RELU_PRE | nat.F_OUT_PIXSHUF | nat.F_PS_BLUR)
    else:
        ps = b.tensor(2 * H, 2 * W, up_c)
        b.conv("shuf", pc, xv, ps, flags=nat.F_RELU_PRE | nat.F_OUT_PIXSHUF)
        b.blur_resize("blur", ps, yv)
    return gu.run_plan(ctx, pack, b, {xv.buf: gu.nhwc_pad(x, xv.cpitch)}, {yv.buf: ((B, yv.H, yv.W, yv.cpitch), np.float16)}, B)[yv.buf]


# 16 x 16: two tiles per side, the second one clamped to a single fresh row; 17 x 20 and 31 x 15: several clamped tiles, tiles_x != tiles_y
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("hw", [(16, 16), (17, 20), (31, 15)], ids=str)
def test_fused_shuffle_blur_tile_walk(ctx, hw, B):
    r = np.random.default_rng(hw[0] * 100 + hw[1] + B)
    x = h16(0.5 * r.standard_normal((B, 64, hw[0], hw[1])))
    w = h16(r.standard_normal((256, 64, 1, 1)) / 8)
    bias = (0.3 * r.standard_normal(256)).astype(np.float32)
    fused, chain = shuffle_blur(ctx, x, w, bias, True), shuffle_blur(ctx, x, w, bias, False)
    assert np.isfinite(chain).all() and chain.astype(np.float32).std() > 0.05
    assert np.array_equal(fused.view(np.uint16), chain.view(np.uint16))


# ---- B: the last K stage with an empty second half ----
# (Cin, k): chunks of 8 channels in the last stage -> skipped or not
B_SHAPES = [
    (8, 1),       # a single stage, one real chunk: half empty
    (32, 1),      # a single stage, four chunks: exactly half
    (40, 1),      # five chunks: must NOT skip
    (64, 1),      # a full stage
    (24, 3),      # 27 chunks: the last stage holds three
]


@pytest.mark.parametrize("shape", B_SHAPES, ids=[str(s) for s in B_SHAPES])
def test_last_stage_with_an_empty_k_half(ctx, shape):
    Cin, k = shape
    x, w, bias = case(3, Cin, k, 9, 11, 31 * Cin + k)
    same_bytes(ctx, x, w, bias, PIPE_CFGS, pad=k // 2, flags=nat.F_RELU_PRE)


def test_tail_conv_259_to_259_under_the_extra_column_tile(ctx):
    """the shape the skip is for: 32 main chunks x 9 taps, then a remainder segment of 9 chunks padded to 16 -- the last stage holds one real chunk"""
    x, w, bias = case(3, 259, 3, 9, 11, 259)
    r = np.random.default_rng(3)
    res = h16(0.5 * r.standard_normal((3, COUT, 9, 11)))
    same_bytes(ctx, x, w, bias, (61, 60, 70), pad=1, flags=nat.F_RELU_PRE, res=res)


def test_split_k_only_the_part_with_the_last_stage_skips(ctx):
    """Cin = 1 032: 128 main chunks + a remainder chunk padded to 8 = 17 stages in 3 parts; the part that owns stage 16 skips its second half"""
    x, w, bias = case(1, 1032, 1, 9, 11, 1032, cout=256)
    outs = {cfg: gu.conv_op(ctx, x, w, bias=bias, flags=nat.F_SPLITK(3), cfg=cfg) for cfg in (1, 60, 70, 71, 72)}
    ref = torch_conv(x, w, bias, 0)
    for cfg, (got, raw) in outs.items():
        assert_close(got, ref, f"split-K conv, configuration {cfg}")
        assert np.array_equal(raw.view(np.uint16), outs[1][1].view(np.uint16)), f"configuration {cfg} differs"
