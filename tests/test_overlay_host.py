"""CPU: the host half of HAVC_clip_overlay (vsdeoldify_amd/overlay.py) -- the crop / pad arithmetic of vsdeoldify/__init__.py:3102-3109 as offsets, the
normalisation and the refusals -- and properties of the numpy definition (tests/overlay_util.py)."""
import numpy as np
import pytest

from tests import overlay_util as U
from vsdeoldify_amd import havc
from vsdeoldify_amd import overlay as OV


@pytest.mark.parametrize("x,y,crop,pad,rect", [
    (0, 0, (0, 0, 0, 0), (0, 36, 0, 14), (0, 0, 30, 20)),
    (5, 7, (0, 0, 0, 0), (5, 31, 7, 7), (5, 7, 35, 27)),
    (-6, -4, (6, 0, 4, 0), (0, 42, 0, 18), (0, 0, 24, 16)),
    (50, 25, (0, 14, 0, 11), (50, 0, 25, 0), (50, 25, 66, 34)),
    (36, 14, (0, 0, 0, 0), (36, 0, 14, 0), (36, 14, 66, 34)),
    (-29, -19, (29, 0, 19, 0), (0, 65, 0, 33), (0, 0, 1, 1)),
    (100, 100, (0, 64, 0, 86), (100, 0, 100, 0), None),
    (-30, 0, (30, 0, 0, 0), (0, 66, 0, 14), None),
    (0, 34, (0, 0, 0, 20), (0, 36, 34, 0), None),
    (66, -100, (0, 30, 100, 0), (66, 0, 0, 114), None),
])
def test_placement_is_the_reference_crop_and_pad_arithmetic(x, y, crop, pad, rect):
    p = OV.placement(66, 34, 30, 20, x, y)
    assert p == dict(crop=crop, pad=pad, rect=rect)
    if rect is not None:                                                                          # what is left of the overlay fills the rectangle between the borders
        assert rect[2] - rect[0] == 30 - crop[0] - crop[1] and rect[3] - rect[1] == 20 - crop[2] - crop[3]


def test_placement_of_an_overlay_larger_than_the_base():
    assert OV.placement(20, 10, 30, 40, -4, -8) == dict(crop=(4, 6, 8, 22), pad=(0, 0, 0, 0), rect=(0, 0, 20, 10))


def test_plan_normalises_like_the_reference():
    plan = OV.overlay_plan((3, 34, 66, 3), (20, 30, 3), None, 5, 7, 1.5, "OverLay", 1, False)
    assert plan["n"] == 3 and plan["base"] == (66, 34) and plan["overlay"] == (30, 20) and plan["overlay_frames"] == 1
    assert plan["opacity"] == 1.0 and plan["mode"] == U.MODES.index("overlay") == 7 and plan["plane_mask"] == 2 and plan["mask_planes"] == 0
    assert OV.overlay_plan((3, 34, 66, 3), (3, 20, 30, 3), (3, 20, 30), opacity=-2)["opacity"] == 0.0
    assert OV.overlay_plan((3, 34, 66, 3), (3, 20, 30, 3), (3, 20, 30))["mask_planes"] == 1
    assert OV.overlay_plan((3, 34, 66, 3), (3, 20, 30, 3), (3, 20, 30, 3))["mask_planes"] == 3
    assert OV.overlay_plan((3, 34, 66, 3), (20, 30, 3), (20, 30))["mask_planes"] == 1
    assert OV.overlay_plan((3, 34, 66, 3), (3, 20, 30, 3), planes=[0, 2])["plane_mask"] == 5
    assert OV.overlay_plan((3, 34, 66, 3), (3, 20, 30, 3))["plane_mask"] == 7
    assert OV.MODES == U.MODES


def test_refusals():
    base, ov = np.zeros((2, 8, 10, 3), np.uint8), np.zeros((2, 4, 6, 3), np.uint8)
    cases = [(dict(base="x"), "mask_overlay: this is not a clip"), (dict(overlay=None), "mask_overlay: this is not a clip"),
             (dict(mask="m"), "mask_overlay: mask is not a clip"),
             (dict(mask=np.zeros((2, 4, 5), np.uint8)), "mask_overlay: mask must have the same dimensions and bit depth as overlay"),
             (dict(mask=np.zeros((2, 8, 10, 3), np.uint8)), "mask_overlay: mask must have the same dimensions and bit depth as overlay"),
             (dict(mask=np.zeros((1, 4, 6), np.uint8)), "as many frames"),
             (dict(mask=np.zeros((2, 4, 6), np.uint16)), "uint8"),
             (dict(mode="screen"), "mask_overlay: invalid mode specified"), (dict(mode=3), "mask_overlay: invalid mode specified"),
             (dict(planes=[0, 3]), "plane 3"), (dict(planes=-1), "plane -1"),
             (dict(overlay=np.zeros((3, 4, 6, 3), np.uint8)), "number of frames"), (dict(base=np.zeros((8, 10, 3), np.uint8)), "[n, h, w, 3]"),
             (dict(overlay=np.zeros((2, 4, 6), np.uint8)), "RGB24"), (dict(x=1 << 30), "2^30")]
    for kw, text in cases:
        args = dict(base=base, overlay=ov)
        args.update(kw)
        with pytest.raises(havc.HAVCError) as e:
            havc.HAVC_clip_overlay(**args)
        assert text in str(e.value), (kw, str(e.value))


# ---- the definition ----------------------------------------------------------------------------------------------------------------------------------------
def test_normal_at_full_opacity_pastes_the_overlay():
    base, ov = U.make_clip(2, 34, 66, 1), U.make_clip(2, 20, 30, 2)
    for x, y in ((0, 0), (5, 7), (-6, -4), (50, 25)):
        out = U.clip_overlay(base, ov, x, y)
        want = base.copy()
        x0, y0, x1, y1 = max(x, 0), max(y, 0), min(x + 30, 66), min(y + 20, 34)
        want[:, y0:y1, x0:x1] = ov[:, y0 - y:y1 - y, x0 - x:x1 - x]
        assert np.array_equal(out, want), (x, y)
    assert np.array_equal(U.clip_overlay(base, ov, 100, 100), base)
    assert np.array_equal(U.clip_overlay(base, ov[0], 5, 7), U.clip_overlay(base, np.stack([ov[0], ov[0]]), 5, 7))       # one frame is repeated


def test_opacity_zero_and_a_black_mask_return_the_base():
    base, ov = U.make_clip(2, 34, 66, 3), U.make_clip(2, 20, 30, 4)
    for mode in U.MODES:
        assert np.array_equal(U.clip_overlay(base, ov, 5, 7, None, 0.0, mode), base), mode
        assert np.array_equal(U.clip_overlay(base, ov, 5, 7, np.zeros((2, 20, 30), np.uint8), 1.0, mode), base), mode


def test_planes_and_mask_planes():
    base, ov = U.make_clip(2, 34, 66, 5), U.make_clip(2, 20, 30, 6)
    full = U.clip_overlay(base, ov, 5, 7, None, 0.5, "multiply")
    out = U.clip_overlay(base, ov, 5, 7, None, 0.5, "multiply", planes=[1])
    assert np.array_equal(out[..., 0], base[..., 0]) and np.array_equal(out[..., 2], base[..., 2]) and np.array_equal(out[..., 1], full[..., 1])
    assert np.array_equal(U.clip_overlay(base, ov, 5, 7, planes=1), U.clip_overlay(base, ov, 5, 7, planes=[1]))
    mask = U.make_clip(2, 20, 30, 7)
    first = U.clip_overlay(base, ov, 5, 7, mask, mask_first_plane=True)
    assert np.array_equal(first, U.clip_overlay(base, ov, 5, 7, mask[..., 0]))                  # plane 0 of three = the gray mask
    each = U.clip_overlay(base, ov, 5, 7, mask, mask_first_plane=False)
    assert np.array_equal(each[..., 0], first[..., 0]) and not np.array_equal(each[..., 1], first[..., 1])
    for k in range(3):
        assert np.array_equal(each[..., k], U.clip_overlay(base, ov, 5, 7, mask[..., k])[..., k])


def test_blend_values_by_hand():
    x, y = np.array([200, 100, 0, 255, 10, 128, 127], np.uint8), np.array([100, 200, 0, 255, 0, 64, 64], np.uint8)
    assert U.blend("addition", x, y).tolist() == [255, 255, 0, 255, 10, 192, 191]
    assert U.blend("average", x, y).tolist() == [150, 150, 0, 255, 5, 96, 96]                    # 95.5 + 0.5 truncates to 96
    assert U.blend("difference", x, y).tolist() == [100, 100, 0, 0, 10, 64, 63]
    assert U.blend("divide", x, y).tolist() == [255, 128, 255, 255, 255, 255, 255]               # y = 0: peak
    assert U.blend("multiply", x, y).tolist() == [78, 78, 0, 255, 0, 32, 32]
    assert U.blend("subtract", x, y).tolist() == [100, 0, 0, 0, 10, 64, 63]
    assert U.blend("exclusion", x, y).tolist() == [143, 143, 0, 0, 10, 128, 127]
    assert U.blend("overlay", x, y).tolist() == [188, 157, 0, 255, 0, 65, 64]
    assert U.expr8(np.array([-3.0, 0.49, 0.5, 254.5, 300.0], np.float32)).tolist() == [0, 0, 1, 255, 255]
