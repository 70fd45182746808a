"""-m gpu: the fused tail epilogue (HAVC_F_FUSE_RGB8) on pixel counts that leave tiles and fragments partly or wholly empty, byte for byte.

tests/test_gpu_fused_tail_epilogue.py holds the op to a tolerance against the two-op chain on three shapes; on those shapes, and on the ones added here,
the kernel in fact gives the chain's bytes (conv + ReLU + residual -> fp16 r2, then the 1x1 conv with the RGB8 epilogue: same operands, same order of
additions).  That equality is what a change of how the residual reaches the epilogue has to keep -- profiles/conv_fixed_cost.txt section 4 records one that
was built against these cases (the first residual batch by LDS-DMA under the last K stage; no gain, dropped) -- and what the last K stage without its
empty second half (conv_pipe_kernel.inc, skip2) must not disturb on this kernel.

Shapes beside the three of that file: pixel counts that are no multiple of the 256-pixel tile or of the 16-pixel fragment, so that single residual rows past
M occur (M = 255, 297, 37), whole empty fragments (M = 37, 60 < 64: fragments 3 - 7 of wave row 0 and all of wave row 1), a tile whose rows straddle three
frames, and the residual as a view at a channel offset of a wider buffer.
"""
import numpy as np
import pytest

from tests.test_gpu_fused_tail_epilogue import SHAPES as BASE_SHAPES
from tests.test_gpu_fused_tail_epilogue import make_case, run_tail

pytestmark = pytest.mark.gpu

# (B, H, W, res_coff)
SHAPES = list(BASE_SHAPES) + [
    (1, 15, 17, 0),       # M = 255: one row short of a tile
    (3, 9, 11, 0),        # M = 297: a tile over three frames + a 41-row tile (2 full fragments, 9 rows of a third, the rest empty)
    (1, 1, 37, 0),        # M = 37 < 64: fragments 0, 1, 5 rows of fragment 2; nothing for the second wave row
    (2, 5, 6, 16),        # M = 60 < 64, residual view at channel offset 16
]
_cache = {}


def outputs(ctx, shape):
    """(case, fused bytes, two-op chain bytes): computed once, shared, never modified"""
    if shape not in _cache:
        B, H, W, coff = shape
        case = make_case(B, H, W, 900 + 31 * H + W + B)
        _cache[shape] = (case, run_tail(ctx, case, True, coff), run_tail(ctx, case, False, coff))
    return _cache[shape]


@pytest.mark.parametrize("shape", SHAPES, ids=[str(s) for s in SHAPES])
def test_fused_tail_every_byte_equals_the_two_op_chain(ctx, shape):
    _, fused, chain = outputs(ctx, shape)
    assert chain.astype(np.float32).std() > 10, "degenerate output"
    d = fused.astype(np.int32) - chain.astype(np.int32)
    assert np.array_equal(fused, chain), f"{int((d != 0).sum())} of {d.size} bytes differ, max {int(np.abs(d).max())} LSB"


@pytest.mark.parametrize("shape", [(3, 9, 11, 0), (3, 24, 20, 0)], ids=str)
def test_fused_tail_batch_of_three_equals_three_single_frame_calls(ctx, shape):
    case, fused, _ = outputs(ctx, shape)
    for i in range(3):
        one = {k: (v[i:i + 1] if k in ("x", "res") else v) for k, v in case.items()}
        assert np.array_equal(run_tail(ctx, one, True, shape[3]), fused[i:i + 1]), f"frame {i} differs between a batch of 3 and a single-frame call"
