"""-m gpu: havc.HAVC_deepex(method=0, ex_model=0) on a 9-frame 64 x 96 clip with seeded ColorMNet weights (the network of tests/test_colormnet_net.py) against
the same steps made by hand: byte equality, no new tolerance.  64 x 96 is 3:2, so SmartResizeColorizer's black borders (9 pixels a side) are part of it."""
import numpy as np
import pytest

from tests.test_colormnet_net import gpu_network
from vsdeoldify_amd import havc
from vsdeoldify_amd import imfilters as F
from vsdeoldify_amd import scdetect as SD
from vsdeoldify_amd.colormnet_render import DeepExColorMNet
from vsdeoldify_amd.device import DeviceImage
from vsdeoldify_amd.stabilizer import stabilize_np

pytestmark = pytest.mark.gpu
N, H, W = 9, 64, 96


def _clips():
    """gray clip with a cut at frame 4 (two textures around different levels, inside the luma thresholds) and a coloured reference clip of it"""
    r = np.random.default_rng(3)
    yy, xx = np.mgrid[0:H, 0:W]
    tex = [90 + 50 * np.sin(xx / 9.0 + yy / 5.0), 150 + 40 * np.cos(xx / 4.0 - yy / 11.0)]
    gray = np.stack([np.clip(tex[0 if i < 4 else 1] + 2 * i + r.integers(-3, 4, (H, W)), 0, 255) for i in range(N)]).astype(np.uint8)
    clip = np.stack([gray] * 3, -1)
    tint = np.array([[1.10, 0.92, 0.70], [0.75, 1.0, 1.15]])
    ref = np.stack([np.clip(clip[i].astype(np.float32) * tint[0 if i < 4 else 1] + [12, 0, 8], 0, 255) for i in range(N)]).astype(np.uint8)
    return clip, ref


def _scenes(prev, threshold=0.10, frequency=0):
    prev = np.asarray(prev, np.int8)
    return SD.SceneInfo(prev, np.zeros(N, np.int8), np.full(N, 0.5), np.zeros(N), threshold, frequency)


def _by_hand(net, clip, refs_small=None, refs=None, blends=None):
    """DeepExColorMNet driven by hand.  refs: {frame: full-size reference} through colorize_frame; refs_small / blends: the steps themselves -- the render
    class on the squashed frame, havc_blend with the squashed reference, Spline64 back to the bordered size, crop, luma of the source."""
    dx = DeepExColorMNet(vid_length=N, render_speed="medium", network=net)
    out = []
    for i in range(N):
        if refs is not None:
            out.append(np.asarray(dx.colorize_frame(clip[i], refs.get(i))))
            continue
        small, (ph, pw) = dx._small(clip[i])
        dx.render.set_ref_frame(refs_small.get(i), False)
        col = np.asarray(dx.render.colorize_frame(i, small))
        if blends and i in blends:
            col = F.blend_np(dx.ctx, col, blends[i][0], blends[i][1])
        up = havc.spline64(dx.ctx, col, W + 2 * pw, H + 2 * ph)[ph:ph + H, pw:pw + W]
        out.append(F.chroma_post_process_np(dx.ctx, np.ascontiguousarray(up), clip[i]))
    return np.stack(out), dx


def test_deepex_equals_the_hand_driven_loop_and_the_hand_made_chains(ctx):
    net = gpu_network()
    clip, ref = _clips()
    scenes = _scenes([1, 0, 0, 0, 1, 0, 0, 0, 0])
    # ref_merge = 0: DeepExColorMNet.colorize_frame by hand with the references at frames 0 and 4
    want, dx = _by_hand(net, clip, refs={0: ref[0], 4: ref[4]})
    assert dx._borders(H, W) == (0, 9)
    got = havc.HAVC_deepex(clip, ref, scenes=scenes, network=net)
    assert got.dtype == np.uint8 and got.shape == clip.shape and np.array_equal(got, want)
    assert not np.array_equal(got[5], clip[5])                                                   # (something was coloured)
    # a DeviceImage clip: stays a DeviceImage, the bytes of the host clip
    dgot = havc.HAVC_deepex(DeviceImage.from_numpy(net.ctx, clip), DeviceImage.from_numpy(net.ctx, ref), scenes=scenes, network=net)
    assert isinstance(dgot, DeviceImage) and np.array_equal(dgot.numpy(), got)
    # every frame a reference (sc_frequency = 1), ref_merge = 3: the clip's own scenes (frames 0 and 4) set the references and stay unblended, the others are
    # propagate -> havc_blend at 0.5 with the squashed reference -> Spline64 back + luma
    every = _scenes(np.ones(N), 0.10, 1)
    dbg = {}
    got3 = havc.HAVC_deepex(clip, ref, ref_merge=3, scenes=every, network=net, debug=dbg)
    assert list(np.flatnonzero(dbg["clip_sc"].scene_change_prev)) == [0, 4] and dbg["ref_weight"] == 0.5
    small = {i: dx._squash(ref[i])[0] for i in range(N)}
    for i in range(N):
        assert np.array_equal(dbg["ref_small"][i], small[i])
    want3, _ = _by_hand(net, clip, refs_small={0: small[0], 4: small[4]}, blends={i: (small[i], 0.5) for i in range(N) if i not in (0, 4)})
    assert np.array_equal(got3, want3)
    assert np.array_equal(got3[0], want[0]) and np.array_equal(got3[4], want[4]) and not np.array_equal(got3[2], want[2])     # flagged: unblended
    # dark + colormap: frames 0 and 4 of the squashed reference go through the stabilizer chain (colormap first), the others stay as squashed
    dbg = {}
    got_t = havc.HAVC_deepex(clip, ref, ref_merge=3, dark=True, dark_p=(0.3, 0.8), colormap="blue->brown", scenes=_scenes([1, 0, 0, 0, 1, 0, 0, 0, 0], 0.10, 1),
                             network=net, debug=dbg)
    cm = havc._get_colormap("blue->brown")
    for i in range(N):
        tweaked = stabilize_np(dx.ctx, small[i], (0.3, 0.8, "none"), None, cm, order=("colormap", "dark", "smooth"))
        assert np.array_equal(dbg["ref_small"][i], tweaked if i in (0, 4) else small[i]), i
        if i in (0, 4):
            by_steps = stabilize_np(dx.ctx, stabilize_np(dx.ctx, small[i], None, None, cm), (0.3, 0.8, "none"))
            assert np.array_equal(tweaked, by_steps) and not np.array_equal(tweaked, small[i])
    assert got_t.shape == clip.shape and not np.array_equal(got_t[0], got3[0])


def test_deepex_device_clip_without_borders_equals_the_host_clip(ctx):
    """72 x 128 is 16:9: no borders, so a DeviceImage clip takes the resident path (squash, frame-in, blend and Spline64 back on the device; frames without
    a reference are squashed on the look-ahead stream, frames WITH one -- flagged at i > 0 -- on the network's own).  Same bytes as the host clip and as the
    hand-driven loop."""
    net = gpu_network()
    r = np.random.default_rng(8)
    n, h, w = 7, 72, 128
    yy, xx = np.mgrid[0:h, 0:w]
    tex = [100 + 55 * np.sin(xx / 8.0 + yy / 6.0), 140 + 45 * np.cos(xx / 5.0 - yy / 9.0)]
    gray = np.stack([np.clip(tex[0 if i < 3 else 1] + 3 * i + r.integers(-3, 4, (h, w)), 0, 255) for i in range(n)]).astype(np.uint8)
    clip = np.stack([gray] * 3, -1)
    ref = np.stack([np.clip(clip[i].astype(np.float32) * ([1.1, 0.9, 0.7] if i < 3 else [0.8, 1.0, 1.15]) + [10, 0, 6], 0, 255) for i in range(n)]).astype(np.uint8)
    prev = np.array([1, 0, 0, 1, 0, 1, 0], np.int8)
    scenes = SD.SceneInfo(prev, np.zeros(n, np.int8), np.full(n, 0.5), np.zeros(n), 0.10, 0)
    dx = DeepExColorMNet(vid_length=n, render_speed="medium", network=net)
    assert dx._borders(h, w) == (0, 0)
    want = np.stack([np.asarray(dx.colorize_frame(clip[i], ref[i] if prev[i] else None)) for i in range(n)])
    host = havc.HAVC_deepex(clip, ref, scenes=scenes, network=net)
    assert np.array_equal(host, want)
    for rep in range(2):
        dgot = havc.HAVC_deepex(DeviceImage.from_numpy(net.ctx, clip), DeviceImage.from_numpy(net.ctx, ref), scenes=scenes, network=net)
        assert isinstance(dgot, DeviceImage) and np.array_equal(dgot.numpy(), host), rep
    # with merging and a tweak, device against host
    every = SD.SceneInfo(np.ones(n, np.int8), np.zeros(n, np.int8), np.full(n, 0.5), np.zeros(n), 0.10, 1)
    kw = dict(ref_merge=2, dark=True, colormap="red->blue", scenes=every, network=net)
    hm = havc.HAVC_deepex(clip, ref, **kw)
    dm = havc.HAVC_deepex(DeviceImage.from_numpy(net.ctx, clip), DeviceImage.from_numpy(net.ctx, ref), **kw)
    assert np.array_equal(dm.numpy(), hm) and not np.array_equal(hm, host)
