"""-m gpu: HAVC_stabilizer (vsdeoldify/__init__.py:2748-2873) -- the fused filter chain (csrc/stabilizer.hip) against the chain of the existing entry
points and against the oracle's chain (pinned to the executed reference by tests/test_stabilizer_host.py), and the whole function against its
decomposition into the library's separately tested Spline64 entry point and the oracle chain.  Byte equality unless said otherwise."""
import itertools
import os

import numpy as np
import pytest

from oracle import tweaks
from tests import stabilizer_util as U
from tests.conftest import GOLDEN
from vsdeoldify_amd import _native as nat
from vsdeoldify_amd import havc, stabilizer
from vsdeoldify_amd.device import DeviceImage
from vsdeoldify_amd.stabilizer import stabilize_np

pytestmark = pytest.mark.gpu


def _parameter_sets():
    """every (dark, smooth, colormap) of the fixture's chain cases, each stage also on its own and in pairs: all 8 on / off combinations per case"""
    _, cases, table = U.fixture()
    out = []
    for c in cases:
        kw = dict(c)
        # a case that leaves a stage off lends it the preset's parameters, so that all 8 combinations exist for every case
        full = dict(U.MEDIUM, **{k: v for k, v in kw.items() if k.endswith("_p") or k == "colormap"})
        d, s, m = U.parsed(table, **dict(full, dark=True, smooth=True))
        for on in itertools.product((False, True), repeat=3):
            p = (d if on[0] else None, s if on[1] else None, m if on[2] else None)
            if p not in out:
                out.append(p)
    return out


def test_fused_chain_equals_the_existing_entry_points_and_the_oracle(ctx):
    g, cases, _ = U.fixture()
    frame = g["img"]
    sets = _parameter_sets()
    assert len(sets) >= 8 * 4 and (None, None, None) in sets
    for p in sets:
        got = stabilize_np(ctx, frame, *p)
        assert got.dtype == np.uint8 and got.shape == frame.shape
        assert np.array_equal(got, U.chain(stabilizer, frame, *p)), p                       # the five existing launches
        assert np.array_equal(got, U.oracle_chain(frame, *p)), p
    # a stack whose pixel count is no multiple of the four pixels a thread takes, host and device; a device frame view at an odd byte offset
    stack = U.colourful(5, 5, 53, 97)                                                      # 25 705 pixels
    assert (stack.shape[0] * stack.shape[1] * stack.shape[2]) % 4 == 1
    full = U.colourful(6, 5, 54, 96)
    assert full.shape == (5, 54, 96, 3)
    for clip in (full, stack):
        dclip = DeviceImage.from_numpy(ctx, clip)
        for p in sets[::3] + [sets[-1]]:
            want = U.oracle_chain(clip, *p)
            assert np.array_equal(stabilize_np(ctx, clip, *p), want), p
            dev = stabilize_np(ctx, dclip, *p)
            assert isinstance(dev, DeviceImage) and dev.shape == clip.shape
            assert np.array_equal(dev.numpy(), want), p
            assert np.array_equal(stabilize_np(ctx, dclip.frame(1), *p).numpy(), want[1]), p   # 53 * 97 * 3 bytes into the stack: not dword-aligned
        assert np.array_equal(dclip.numpy(), clip)                                          # the input is left alone


def test_single_stage_chains_reproduce_the_reference_vectors(ctx):
    """dark_tweak_0/1 and bright_tweak_0/1 of tests/golden/tweaks.npz (the reference's selector bodies, executed) as one-stage chains"""
    G = np.load(os.path.join(GOLDEN, "tweaks.npz"))
    base = G["base"]
    assert np.array_equal(stabilize_np(ctx, base, smooth=(0.3, 0.6, 0.8, -0.10, "none")), G["bright_tweak_0"])
    assert np.array_equal(stabilize_np(ctx, base, smooth=(0.4, 0.4, 0.6, -0.25, "red|0.5,0.0")), G["bright_tweak_1"])
    assert np.array_equal(stabilize_np(ctx, base, dark=(0.3, 0.8, "none")), G["dark_tweak_0"])
    assert np.array_equal(stabilize_np(ctx, base, dark=(0.45, 0.5, "280:360,0:30")), G["dark_tweak_1"])
    assert np.array_equal(stabilize_np(ctx, base, colormap="blue|+40,0.2"), tweaks.colormap_frame(base, "blue|+40,0.2"))
    d = stabilize_np(ctx, DeviceImage.from_numpy(ctx, base), dark=(0.45, 0.5, "280:360,0:30"))
    assert np.array_equal(d.numpy(), G["dark_tweak_1"])


def test_no_stage_is_a_copy_and_a_bad_stage_launches_nothing(ctx):
    clip = U.colourful(7, 2, 31, 45)
    out = stabilize_np(ctx, clip)
    assert out is not clip and np.array_equal(out, clip)
    dclip = DeviceImage.from_numpy(ctx, clip)
    dout = stabilize_np(ctx, dclip)
    assert dout.ptr.value != dclip.ptr.value and np.array_equal(dout.numpy(), clip)
    good = stabilizer._chroma_stage(0.9, -0.1, "red|0.5,0.0", (0.3, 0.7))
    for field, value in (("kind", 2), ("kind", -1), ("merge_mode", 4), ("merge_mode", -2), ("n_ranges", 9), ("n_ranges", -1), ("n_ranges", 0),
                         ("has_adjust", 2)):
        bad = nat.StabStage.from_buffer_copy(good)
        setattr(bad, field, value)
        res = np.full_like(clip, 7)
        ctx.synchronize()
        before = ctx.stats().launches
        arr = (nat.StabStage * 2)(good, bad)
        rc = ctx.lib.havc_stabilizer_chain(ctx.h, nat.as_ptr(clip), nat.as_ptr(res), clip.shape[2], clip.shape[0] * clip.shape[1], arr, 2)
        assert rc == nat.HAVC_E_INVALID == -1, (field, value, rc)
        assert b"stabilizer_chain" in ctx.lib.havc_last_error(ctx.h)
        assert ctx.stats().launches == before and (res == 7).all(), (field, value)
        with pytest.raises(Exception):
            nat.check(rc, ctx.h)
    for n in (-1, 4):
        arr = (nat.StabStage * 4)(good, good, good, good)
        assert ctx.lib.havc_stabilizer_chain(ctx.h, nat.as_ptr(clip), nat.as_ptr(np.empty_like(clip)), clip.shape[2], clip.shape[0] * clip.shape[1], arr, n) == -1
    assert ctx.lib.havc_stabilizer_chain(ctx.h, nat.as_ptr(clip), nat.as_ptr(np.empty_like(clip)), clip.shape[2], clip.shape[0] * clip.shape[1], None, 1) == -1
    # in place on a device buffer: out may be img
    want = U.chain(tweaks, clip[0], None, (0.3, 0.7, 0.9, -0.1, "red|0.5,0.0"), None)
    d0 = DeviceImage.from_numpy(ctx, clip[0])
    arr = (nat.StabStage * 1)(good)
    nat.check(ctx.lib.havc_stabilizer_chain(ctx.h, d0.ptr, d0.ptr, clip.shape[2], clip.shape[1], arr, 1), ctx.h)
    assert np.array_equal(d0.numpy(), want)


PARAMS = [U.MEDIUM, dict(colormap="red->brown"), dict()]


@pytest.mark.parametrize("size", [(400, 300), (1920, 1080)])
def test_whole_function_equals_its_decomposition(ctx, size):
    """HAVC_stabilizer == spline64(oracle chain(spline64(clip, fs, fs)), w, h, luma_from=clip): the two resamples are the library's own entry point
    (tested on its own against oracle.resample), the chain is the oracle's"""
    _, _, table = U.fixture()
    w, h = size
    clip = U.colourful(11, 3, h, w)
    fs = min(24 * 16, w)
    sq = havc.spline64(ctx, clip, fs, fs)
    assert sq.shape == (3, fs, fs, 3)
    for kw in PARAMS:
        want = havc.spline64(ctx, U.oracle_chain(sq, *U.parsed(table, **kw)), w, h, luma_from=clip)
        got = havc.HAVC_stabilizer(clip, **kw)
        assert isinstance(got, np.ndarray) and got.shape == clip.shape and got.dtype == np.uint8
        assert np.array_equal(got, want), kw
        if kw:
            assert (got != clip).any()
    # one frame in, one frame out; the auto render factor (__init__.py:2798-2799)
    rf0 = min(max(int(0.4 * w / 16), 16), 32)
    fs0 = min(rf0 * 16, w)
    want = havc.spline64(ctx, U.oracle_chain(havc.spline64(ctx, clip[1], fs0, fs0), *U.parsed(table, **U.MEDIUM)), w, h, luma_from=clip[1])
    got = havc.HAVC_stabilizer(clip[1], render_factor=0, **U.MEDIUM)
    assert got.shape == clip[1].shape and np.array_equal(got, want)


def test_everything_off_against_the_all_oracle_graph(ctx):
    """no filter: Spline64 down, Spline64 back, the source's luma -- against oracle.resample / oracle.pipeline end to end, under the condition
    tests/test_havc_harness.py uses for the Spline64 .5-boundary ties (max <= 1, fewer than 2e-4 of the bytes differ)"""
    from oracle import pipeline, resample
    from tests.test_havc_harness import _frame
    f = _frame(3)
    h, w = f.shape[:2]
    fs = min(24 * 16, w)
    want = pipeline.post_process(resample.resize_rgb8(resample.resize_rgb8(f, fs, fs), w, h), f)
    got = havc.HAVC_stabilizer(f)
    d = np.abs(got.astype(int) - want.astype(int))
    print("everything off vs all-oracle graph: max", int(d.max()), "share", float((d > 0).mean()))
    assert d.max() <= 1 and (d > 0).mean() < 2e-4, (int(d.max()), float((d > 0).mean()))


def test_device_clip_chains_behind_the_colorizer(ctx):
    """HAVC_stabilizer(HAVC_colorizer(DeviceImage)) stays a DeviceImage and carries the bytes of the host-array path of the same two calls"""
    from tests.test_havc_harness import _frame, _weights
    sds, _ = _weights()
    clip = np.stack([_frame(21), _frame(22)])
    kw = dict(method=0, deoldify_p=(0, 10, 1.0, 0.0), state_dicts=sds)
    host = havc.HAVC_stabilizer(havc.HAVC_colorizer(clip, **kw), colormap="blue->brown")
    dcol = havc.HAVC_colorizer(DeviceImage.from_numpy(ctx, clip), **kw)
    assert isinstance(dcol, DeviceImage)
    dev = havc.HAVC_stabilizer(dcol, colormap="blue->brown")
    assert isinstance(dev, DeviceImage) and dev.shape == clip.shape
    assert np.array_equal(dev.numpy(), host)
    one = havc.HAVC_stabilizer(dcol.frame(1), colormap="blue->brown")
    assert isinstance(one, DeviceImage) and one.shape == clip.shape[1:] and np.array_equal(one.numpy(), host[1])
