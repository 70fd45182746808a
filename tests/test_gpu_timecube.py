"""-m gpu: havc_lut3d_clip (csrc/lut3d.hip) and HAVC_TimeCube against the numpy definition of tests/timecube_util.py: every comparison is byte-equal.

Table sizes N:  2   one cell, every sample in it            3   two cells, the clamp idx = N - 2 at the top sample
                17, 33   odd sizes as .cube files ship them   65  4.4 MB of points: more than one XCD's 4 MiB of L2
Frames, h x w:  1 x 1 and 3 x 5 (fewer than four pixels; a ragged last group of a thread's four), 34 x 66, 70 x 130 (more than one block); clips of 1 and 3
frames with different content per frame.  Random tables in [-0.2, 1.2]: the output clamp is hit on both sides.
HAVC_TimeCube is compared with the composition of the three definitions: timecube_util.lut3d -> tweak_util.tweak -> the oracle's merge (pil_blend, or
ChromaBoundAdaptiveMerge for effect 8)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from oracle import pipeline
from tests import timecube_util as U
from tests import tweak_util as TU
from vsdeoldify_amd import havc
from vsdeoldify_amd import timecube as TC
from vsdeoldify_amd.device import DeviceImage

pytestmark = pytest.mark.gpu

SIZES = [2, 3, 17, 33, 65]
FRAMES = [(1, 1), (3, 5), (34, 66), (70, 130)]


def _same(got, want, what):
    bad = np.argwhere(got != want)
    assert got.shape == want.shape and len(bad) == 0, (what, len(bad), bad[0].tolist(), int(got[tuple(bad[0])]), int(want[tuple(bad[0])]))


@pytest.mark.parametrize("size", SIZES)
def test_lut_alone_on_random_tables(ctx, size):
    cube = U.random_cube(size)
    for h, w in FRAMES:
        for n in (1, 3):
            clip = U.make_clip(h, w, n)
            _same(TC.lut3d_np(ctx, clip, cube), U.lut3d(clip, cube), (size, h, w, n))
    frame = U.make_clip(34, 66, 1)[0]
    _same(TC.lut3d_np(ctx, frame, cube), U.lut3d(frame, cube), (size, "a frame"))
    clip = U.make_clip(70, 130, 2)
    _same(TC.lut3d_np(ctx, clip, U.identity_cube(size)), clip, (size, "identity"))


def test_a_frame_of_a_clip_equals_the_frame_alone(ctx):
    cube, clip = U.random_cube(17, seed=3), U.make_clip(3, 5, 3)
    whole = TC.lut3d_np(ctx, clip, cube)
    for k in range(3):
        _same(TC.lut3d_np(ctx, clip[k], cube), whole[k], k)


@pytest.mark.parametrize("size", [3, 17])
def test_lut_with_a_shifted_domain(ctx, size):
    cube = U.random_cube(size, seed=1, domain_min=(0.1, 0.0, 0.25), domain_max=(0.9, 0.5, 2.0))      # samples below, inside and above the domain
    clip = U.make_clip(70, 130, 3)
    _same(TC.lut3d_np(ctx, clip, cube), U.lut3d(clip, cube), size)
    ident = U.identity_cube(size, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    _same(TC.lut3d_np(ctx, clip, ident), clip, (size, "identity"))


@functools.lru_cache(maxsize=None)
def _sweep_cube():
    return U.random_cube(33, seed=5)


@pytest.mark.parametrize("rotation", [0, 1, 2])
def test_sweep_of_2_36_million_inputs(ctx, rotation):
    frame = U.sweep_frame(rotation)
    _same(TC.lut3d_np(ctx, frame, _sweep_cube()), U.lut3d(frame, _sweep_cube()), rotation)
    if rotation == 0:
        _same(TC.lut3d_np(ctx, frame, U.identity_cube(33)), frame, "identity")


def test_table_host_or_device_and_clip_host_or_device(ctx):
    cube, clip = U.random_cube(33, seed=2), U.make_clip(34, 66, 3)
    want = U.lut3d(clip, cube)
    nb = cube.table.nbytes
    d_table = ctx.dev_alloc(nb)
    try:
        ctx.dev_upload(d_table, cube.table.view(np.uint8).reshape(-1))
        _same(TC.lut3d_np(ctx, clip, cube, table_ptr=d_table), want, "device table, host clip")
        dev = TC.lut3d_np(ctx, DeviceImage.from_numpy(ctx, clip), cube, table_ptr=d_table)
        assert isinstance(dev, DeviceImage)
        _same(dev.numpy(), want, "device table, device clip")
    finally:
        ctx.dev_free(d_table)
    dev = TC.lut3d_np(ctx, DeviceImage.from_numpy(ctx, clip), cube)
    assert isinstance(dev, DeviceImage)
    _same(dev.numpy(), want, "host table, device clip")
    odd = U.make_clip(3, 5, 3)
    dclip = DeviceImage.from_numpy(ctx, odd)
    _same(TC.lut3d_np(ctx, dclip.frame(1), cube).numpy(), U.lut3d(odd[1], cube), "a frame view at an odd byte offset")


def test_c_abi_refusals(ctx):
    from vsdeoldify_amd import _native as nat
    cube, clip = U.identity_cube(2), U.make_clip(3, 5, 1)
    idx, frac = TC.axis_tables(cube)
    out = np.empty_like(clip)

    def call(src, dst, size=2, w=5, h=3, n=1):
        p = nat.Lut3dParams(width=w, height=h, n_frames=n, size=size)
        return ctx.lib.havc_lut3d_clip(ctx.h, nat.as_ptr(src), nat.as_ptr(dst), nat.as_ptr(cube.table), nat.as_ptr(idx), nat.as_ptr(frac), C.byref(p))

    assert call(clip, out) == 0
    for kw in (dict(size=1), dict(size=257), dict(w=0), dict(h=-1), dict(n=0), dict(w=1 << 16, h=(1 << 14) + 1)):
        assert call(clip, out, **kw) == nat.HAVC_E_INVALID, kw
    assert call(clip, clip) == nat.HAVC_E_INVALID


# ---- HAVC_TimeCube -----------------------------------------------------------------------------------------------------------------------------------------
EFFECTS = [0, 2, 8]


@pytest.fixture(scope="module")
def lut_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("luts")
    os.makedirs(d / "color")
    for e in EFFECTS:
        U.write_cube(d / "color" / TC.LUT_FILES[e], U.graded_cube(17, seed=e))
    return str(d)


@functools.lru_cache(maxsize=None)
def _graded(h, w, effect):
    """the clip, and the definition's LUT -> tweak of it"""
    clip = U.make_clip(h, w, 3, seed=effect)
    cube = TC.parse_cube(U.cube_text(U.graded_cube(17, seed=effect)))
    return clip, TU.tweak(U.lut3d(clip, cube), **TC.timecube_plan(1.0, effect, None, "d")["tweak"])


def _merged(clip, new, effect, strength):
    if strength == 1:
        return new
    method, cmc = (7, TC.AMBER_CMC_P) if effect == 8 else (2, (0.15, True, 20, 24))
    return np.stack([pipeline.combine_models(a, b, method, strength, cmc_p=cmc) for a, b in zip(clip, new)])


@pytest.mark.parametrize("effect", EFFECTS)
@pytest.mark.parametrize("h,w", [(34, 66), (70, 130)])
def test_timecube_against_the_composition(ctx, lut_dir, h, w, effect):
    clip, new = _graded(h, w, effect)
    for strength in (0.6, 1):
        _same(havc.HAVC_TimeCube(clip, strength, effect, lut_dir=lut_dir), _merged(clip, new, effect, strength), (h, w, effect, strength))
    assert havc.HAVC_TimeCube(clip, 0, effect, lut_dir=lut_dir) is clip


def test_timecube_factors_cube_argument_environment_and_device(ctx, lut_dir, monkeypatch, tmp_path):
    odd = U.make_clip(3, 5, 2)
    cube = U.graded_cube(9, seed=4)
    neutral = [0, 1, 0, 1, 1]
    _same(havc.HAVC_TimeCube(odd, 1.0, 2, neutral, cube=cube), U.lut3d(odd, cube), "neutral factors on 3 x 5")
    _same(havc.HAVC_TimeCube(odd[0], 1.0, 2, neutral, cube=cube), U.lut3d(odd[0], cube), "neutral factors on one frame")
    want = np.stack([pipeline.combine_models(a, b, 2, 0.25) for a, b in zip(odd, U.lut3d(odd, cube))])
    _same(havc.HAVC_TimeCube(odd, 0.25, 2, neutral, cube=cube), want, "neutral factors, merged")
    path = U.write_cube(tmp_path / "mine.cube", cube, line_end="\r\n")
    clip = U.make_clip(34, 66, 3, seed=9)
    factors = [12.0, 0.8, -12.0, 1.1, 1.2]
    new = TU.tweak(U.lut3d(clip, TC.parse_cube(path)), hue=12.0, sat=0.8, bright=-12.0, cont=1.1, gamma=1.2)
    want = _merged(clip, new, 5, 0.6)
    _same(havc.HAVC_TimeCube(clip, 0.6, 5, factors, cube=path), want, "cube= as a path")
    _same(havc.HAVC_TimeCube(clip, 0.6, 5, factors, cube=TC.parse_cube(path)), want, "cube= as an object")
    dev = havc.HAVC_TimeCube(DeviceImage.from_numpy(ctx, clip), 0.6, 5, factors, cube=path)
    assert isinstance(dev, DeviceImage)
    _same(dev.numpy(), want, "DeviceImage in, DeviceImage out")
    clip8, new8 = _graded(34, 66, 8)
    dev = havc.HAVC_TimeCube(DeviceImage.from_numpy(ctx, clip8), 0.6, 8, lut_dir=lut_dir)
    assert isinstance(dev, DeviceImage)
    _same(dev.numpy(), _merged(clip8, new8, 8, 0.6), "effect 8 on the device")
    monkeypatch.setenv("HAVC_LUT_DIR", lut_dir)
    clip2, new2 = _graded(34, 66, 2)
    _same(havc.HAVC_TimeCube(clip2, 1.0, 2), new2, "HAVC_LUT_DIR")
    dclip = DeviceImage.from_numpy(ctx, clip)
    assert havc.HAVC_TimeCube(dclip, 0, 2) is dclip
