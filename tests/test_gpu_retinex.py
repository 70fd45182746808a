"""-m gpu: havc_retinex_clip (csrc/retinex.hip), retinex.retinex_np and HAVC_retinex against the numpy restatement of tests/retinex_util.py (the definition).

Clips of 6 frames (retinex_util.make_clip: gated dark, gated bright, blend zone, ordinary, constant, black runs + saturated channel) at
    7 x 5       below any tile            64 x 64     one exact horizontal tile column block (64 rows), two 32-column tiles
    65 x 130    tile + 1 and tiles + 2    33 x 257    odd; frames start at odd byte offsets
    96 x 200    ordinary                  3 x 1100    a row longer than any plausible staging width
  * the Gaussian planes and the MSR product, through the tap, bit for bit: there is no transcendental before that point, so there is no tolerance;
  * the bytes: no byte off by more than 1 LSB and at most 1 byte in 10 000 of a clip different.  The only step that is not bit-defined is the logarithm; a
    last-place difference between the device's and numpy's moves 7 bytes of 2.35 million by 1 (test_retinex_host.py, measurement (b)): the cap leaves more
    than ten times that and lies two to three orders of magnitude below what a wrong coefficient, a wrong initial state or float32 planes cause
    (measurement (a): 66 %)."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import retinex_util as U
from vsdeoldify_amd import _native as nat
from vsdeoldify_amd import havc
from vsdeoldify_amd import retinex as RX
from vsdeoldify_amd.device import DeviceImage

pytestmark = pytest.mark.gpu

DEFAULT = (25, 80, 250)


def _close(got, want, what):
    n, mx = U.count_diff(got, want)
    print(f"retinex bytes {what}: {n} of {want.size} differ, largest difference {mx}")
    assert mx <= 1, (what, n, mx)
    assert n * 10000 <= want.size, (what, n, want.size)


@pytest.mark.parametrize("h,w", U.SIZES)
@pytest.mark.parametrize("sigmas", U.SIGMA_SETS)
def test_planes_bit_for_bit(ctx, h, w, sigmas):
    clip = U.make_clip(h, w)
    for fulls in ((True, False) if sigmas == DEFAULT else (True,)):
        _, g, p = U.reference(h, w, sigmas, fulls)
        _, planes = RX.retinex_np(ctx, clip, sigmas, fulls=fulls, fulld=fulls, range_tv=fulls, tap=True)
        assert planes.shape == (6, len(sigmas) + 1, h, w)
        for k in range(len(sigmas)):
            bad = np.argwhere(planes[:, k].view(np.uint64) != g[:, k].view(np.uint64))
            assert len(bad) == 0, (h, w, sigmas[k], fulls, len(bad), bad[0].tolist(), planes[:, k][tuple(bad[0])], g[:, k][tuple(bad[0])])
        bad = np.argwhere(planes[:, -1].view(np.uint64) != p.view(np.uint64))
        assert len(bad) == 0, (h, w, "P", fulls, len(bad), bad[0].tolist())


@pytest.mark.parametrize("h,w", U.SIZES)
def test_bytes(ctx, h, w):
    clip = U.make_clip(h, w)
    for blend, tv_in, tv_out in itertools.product((False, True), (True, False), (True, False)):
        rtx = U.reference_bytes(h, w, DEFAULT, tv_in, tv_out)
        want = U.retinex_ref(clip, range_tv_in=tv_in, range_tv_out=tv_out, blend=blend, rtx=rtx)
        got = RX.retinex_np(ctx, clip, DEFAULT, fulls=tv_in, fulld=tv_out, range_tv=tv_in, blend=blend)
        _close(got, want, (h, w, blend, tv_in, tv_out))
        for k in (0, 1, 4):                                        # gated out (the constant frame by the default bounds): the input, byte for byte
            assert np.array_equal(got[k], clip[k]), (h, w, blend, tv_in, tv_out, k)
        assert not np.array_equal(got[3], clip[3])
        if blend:                                                  # the blend zone's frame is a blend: neither the input nor the stand-in's frame
            assert not np.array_equal(got[2], clip[2]) and not np.array_equal(got[2], rtx[2])


@pytest.mark.parametrize("h,w", [(7, 5), (64, 64), (33, 257)])
def test_the_constant_frame_through_the_gate_is_unchanged(ctx, h, w):
    """luma_dark = 0 lets the constant frame in: it takes the mx <= mn path and comes back as it went in"""
    clip = U.make_clip(h, w)
    for tv in (True, False):
        want = U.retinex_ref(clip, luma_dark=0.0, range_tv_in=tv, range_tv_out=tv, blend=True, rtx=U.reference_bytes(h, w, DEFAULT, tv, tv))
        got = RX.retinex_np(ctx, clip, DEFAULT, fulls=tv, fulld=tv, luma_dark=0.0, range_tv=tv, blend=True)
        _close(got, want, ("open gate", h, w, tv))
        assert np.array_equal(got[4], clip[4]) and not np.array_equal(got[0], clip[0])


def test_chunks(ctx):
    h, w = 33, 257
    clip = U.make_clip(h, w)[[2, 3, 5, 0, 3]]
    whole = RX.retinex_np(ctx, clip, blend=True)
    for chunk in (2, 1, 5, 7):
        assert np.array_equal(RX.retinex_np(ctx, clip, blend=True, chunk_frames=chunk), whole), chunk
    _, planes = RX.retinex_np(ctx, clip, chunk_frames=2, tap=True)
    _, g, p = U.reference(h, w, DEFAULT, True)
    assert np.array_equal(planes[:, :3].view(np.uint64), g[[2, 3, 5, 0, 3]].view(np.uint64)) and np.array_equal(planes[:, 3].view(np.uint64), p[[2, 3, 5, 0, 3]].view(np.uint64))


def test_device_operands(ctx):
    h, w = 65, 130
    clip = U.make_clip(h, w)
    dclip = DeviceImage.from_numpy(ctx, clip)
    want = RX.retinex_np(ctx, clip, blend=True)
    dout = RX.retinex_np(ctx, dclip, blend=True)
    assert isinstance(dout, DeviceImage) and dout.shape == clip.shape
    first = dout.numpy()
    assert np.array_equal(first, want)
    assert np.array_equal(RX.retinex_np(ctx, dclip, blend=True).numpy(), first)
    assert np.array_equal(dclip.numpy(), clip)


def test_havc_retinex_equals_retinex_np(ctx):
    h, w = 96, 200
    clip = U.make_clip(h, w)
    for dark, bright, sigmas, tv_in, tv_out, blend in ((0.20, 0.80, (25, 80, 250), True, True, False), (0.1, 0.7, [15.5, 300], False, True, True)):
        want = RX.retinex_np(ctx, clip, **RX.plugin_args(sigmas, tv_in, tv_out), luma_dark=dark, luma_bright=bright, range_tv=tv_in, blend=blend)
        got = havc.HAVC_retinex(clip, dark, bright, sigmas, tv_in, tv_out, blend)
        assert np.array_equal(got, want)
        frame = havc.HAVC_retinex(clip[3], dark, bright, sigmas, tv_in, tv_out, blend)
        assert frame.shape == clip[3].shape and np.array_equal(frame, want[3])
    _close(havc.HAVC_retinex(clip), U.retinex_ref(clip, rtx=U.reference_bytes(h, w, DEFAULT, True, True)), "HAVC_retinex defaults")
    dout = havc.HAVC_retinex(DeviceImage.from_numpy(ctx, clip))
    assert isinstance(dout, DeviceImage) and np.array_equal(dout.numpy(), havc.HAVC_retinex(clip))
    dframe = havc.HAVC_retinex(DeviceImage.from_numpy(ctx, clip[3]))
    assert isinstance(dframe, DeviceImage) and dframe.shape == clip[3].shape and np.array_equal(dframe.numpy(), havc.HAVC_retinex(clip[3]))


def test_bad_arguments_are_refused(ctx):
    h, w, n = 8, 8, 2
    src, dst = np.zeros((n, h, w, 3), np.uint8), np.full((n, h, w, 3), 7, np.uint8)

    def params(**kw):
        p = nat.RetinexParams(width=w, height=h, n_frames=n, n_sigmas=3, luma_dark=0.2, luma_bright=0.8, fulls=1, fulld=1, range_tv=1)
        p.sigma[0], p.sigma[1], p.sigma[2] = 25, 80, 250
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def call(s, d, p):
        return ctx.lib.havc_retinex_clip(ctx.h, s, d, C.byref(p) if p is not None else None, None)
    ps, pd = nat.as_ptr(src), nat.as_ptr(dst)
    E = nat.HAVC_E_INVALID
    assert call(None, pd, params()) == E and call(ps, None, params()) == E and call(ps, pd, None) == E
    assert ctx.lib.havc_retinex_clip(None, ps, pd, C.byref(params()), None) == E
    assert call(ps, ps, params()) == E
    assert call(ps, pd, params(n_sigmas=0)) == E and call(ps, pd, params(n_sigmas=9)) == E
    zero = params()
    zero.sigma[1] = 0.0
    assert call(ps, pd, zero) == E
    assert call(ps, pd, params(width=0)) == E and call(ps, pd, params(n_frames=0)) == E and call(ps, pd, params(chunk_frames=-1)) == E
    assert (dst == 7).all()                                        # nothing ran
    assert call(ps, pd, params()) == 0
