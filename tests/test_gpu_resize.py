"""-m gpu: the Spline64 resize on EVERY horizontal kernel variant against a float64 reference (tests/resize_util.py), through vsdeoldify_amd.havc.spline64
on 4-D host clips.

The suite's other resize tests pass one to six frames, which launch_resize_passes (csrc/colorfilters.hip) gives to the one-block-per-row resize_h_kernel;
the benchmark's clips run the batched resize_h_rows_kernel<TMAX>, chosen only from 2048 blocks (16-row chunks x 256-column tiles) on.  Each case below first
asserts with havc_resize_plan that it lands on the variant it is named for, so a later change of the thresholds cannot silently take the coverage away.
The sizes are the smallest that reach 2048 blocks (32 753 rows for one tile, 16 369 for two).  Every byte of every frame is compared: exact outside
near-ties of the float64 value, either neighbour inside them (resize_util: eps is derived from the fp32 passes, the near-tie share is capped at 1 %).

Inputs: random uint8, seed = case index; frame 0 is random 0 / 255 so that overshoot saturates (cases a, b, c and g1; the stronger down-sampling of
the others averages the noise back into range).

| case | n x sh x sw -> dw x dh          | variant | what it adds                                                                                           |
| a    | 65 x 513 x 40 -> 130 x 200      | 9       | one partial tile; dw % 4 != 0 (scalar stores, resize_v_kernel); sh % 16 = 1: chunks straddle frames,   |
|      |                                 |         | the last chunk has one row                                                                             |
| b    | 33 x 500 x 96 -> 260 x 124 luma | 9       | two tiles, ragged second (4 columns); 16-byte stores; resize_v4_kernel; fused luma                     |
| c    | 33 x 500 x 520 -> 260 x 500     | 17      | taps = 17 exactly; identity vertical                                                                   |
| d    | 65 x 513 x 42 -> 12 x 100       | 29      | taps = 29 exactly; 12 active lanes                                                                     |
| e    | 65 x 513 x 93 -> 24 x 100       | 32      | taps = 32 exactly                                                                                      |
| f    | 33 x 500 x 1326 -> 260 x 60     | 48      | 42 taps, staged span 4048 of 4096 bytes                                                                |
| g1   | 1 x 97 x 1400 -> 260 x 97       | 0       | fallback beyond the LDS limit                                                                          |
| g2   | 3 x 50 x 600 -> 96 x 31         | 0       | fallback beyond 48 taps; three frames through the vertical pass                                        |
| h    | 1 x 61 x 83 -> 83 x 61 luma     | 0       | same size with luma: no copy shortcut                                                                  |
"""
import collections

import numpy as np
import pytest

from tests import resize_util as RU
from vsdeoldify_amd import havc
from vsdeoldify_amd.device import DeviceImage

pytestmark = pytest.mark.gpu

Case = collections.namedtuple("Case", "seed n sh sw dw dh variant taps luma")
CASES = {
    "a": Case(0, 65, 513, 40, 130, 200, 9, 9, False),
    "b": Case(1, 33, 500, 96, 260, 124, 9, 9, True),
    "c": Case(2, 33, 500, 520, 260, 500, 17, 17, False),
    "d": Case(3, 65, 513, 42, 12, 100, 29, 29, False),
    "e": Case(4, 65, 513, 93, 24, 100, 32, 32, False),
    "f": Case(5, 33, 500, 1326, 260, 60, 48, 42, False),
    "g1": Case(6, 1, 97, 1400, 260, 97, 0, 45, False),
    "g2": Case(6, 3, 50, 600, 96, 31, 0, 51, False),
    "h": Case(7, 1, 61, 83, 83, 61, 0, 9, True),
}

_kept = {}


def operands(name):
    """(clip, luma or None, Ref64) of a case; the reference is computed once and left unchanged (case b serves three tests)"""
    if name in _kept:
        return _kept[name]
    c = CASES[name]
    r = np.random.default_rng(c.seed)
    clip = r.integers(0, 256, (c.n, c.sh, c.sw, 3), dtype=np.uint8)
    clip[0] = r.integers(0, 2, clip[0].shape, dtype=np.uint8) * 255
    luma = r.integers(0, 256, (c.n, c.dh, c.dw, 3), dtype=np.uint8) if c.luma else None
    ref = RU.ref64(clip, c.dw, c.dh)
    ref.v.setflags(write=False)
    out = (clip, luma, ref)
    if name == "b":
        _kept[name] = out
    return out


def assert_plan(ctx, name):
    c = CASES[name]
    taps, variant, span_lds = RU.plan(ctx.lib, c.sw, c.dw, c.n * c.sh)
    assert (taps, variant) == (c.taps, c.variant), (name, taps, variant, span_lds)
    return span_lds


@pytest.mark.parametrize("name", list(CASES))
def test_spline64_every_variant_against_float64(ctx, name):
    c = CASES[name]
    span_lds = assert_plan(ctx, name)
    if name == "f":
        assert span_lds == 4048
    if name == "g1":
        assert span_lds > 4096
    clip, luma, ref = operands(name)
    sat = int(((ref.v > 255.5) | (ref.v < -0.5)).sum())
    print(f"case {name}: variant {c.variant}, {c.taps} taps, span {span_lds} bytes of LDS, {sat} values saturate")
    if name in ("a", "b", "c", "g1"):          # up-sampled or merely halved, the 0 / 255 frame overshoots; the stronger down-sampling averages it back into range
        assert sat > 500 and ref.v[0].max() > 280 and ref.v[0].min() < -25
    label = f"case {name}"
    # the condition of the rule, from the reference alone, before the GPU output exists
    tie = RU.assert_near_tie_share(ref, label, per_pixel=c.luma)
    got = havc.spline64(ctx, clip, c.dw, c.dh, luma_from=luma)
    if c.luma:
        RU.check_fused(got, ref, tie, luma, label)
    else:
        RU.check_bytes(got, ref, tie, label)


def test_spline64_batched_twice_gives_the_same_bytes(ctx):
    assert_plan(ctx, "b")
    c = CASES["b"]
    clip, luma, _ = operands("b")
    assert np.array_equal(havc.spline64(ctx, clip, c.dw, c.dh, luma_from=luma), havc.spline64(ctx, clip, c.dw, c.dh, luma_from=luma))


def test_spline64_batched_device_operands_equal_host_operands(ctx):
    assert_plan(ctx, "b")
    c = CASES["b"]
    clip, luma, _ = operands("b")
    dev = havc.spline64(ctx, DeviceImage.from_numpy(ctx, clip), c.dw, c.dh, luma_from=DeviceImage.from_numpy(ctx, luma))
    assert isinstance(dev, DeviceImage) and np.array_equal(dev.numpy(), havc.spline64(ctx, clip, c.dw, c.dh, luma_from=luma))
