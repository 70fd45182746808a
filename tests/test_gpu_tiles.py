"""-m gpu: HAVC_clip_slice / HAVC_clip_reconstruct (vsdeoldify/__init__.py:2886-2945; csrc/tiles.hip) against the numpy restatement of tests/tiles_util.py
(pinned by tests/test_tiles_host.py) and the executed reference's tiles (tests/golden/tiles.npz).  Byte equality throughout.  Shapes are tiny and chosen
against the kernels: both sizes odd (37 x 51), multiples of four (36 x 48), a clip narrower than three thread groups (6 x 10); tile row pitches
(base_w + overlap) * 3 of every alignment; 1 and 3 frames."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import tiles_util as U
from vsdeoldify_amd import _native as nat
from vsdeoldify_amd import havc
from vsdeoldify_amd import imfilters as F
from vsdeoldify_amd.device import DeviceImage

pytestmark = pytest.mark.gpu

SHAPES = [(1, 37, 51), (3, 37, 51), (3, 36, 48), (1, 6, 10)]                                     # (frames, height, width)
OVERLAPS = (0, 2, 6)
WEIGHTS = (0, 0.001, 0.3, 0.5, 1.0)


def _legal(h, w, slices, ov):
    return ov < (w + 1) // 2 and (slices == 2 or ov < (h + 1) // 2)


def _geometries():
    return [(s, sl, ov) for s, sl, ov in itertools.product(SHAPES, (2, 4), OVERLAPS) if _legal(s[1], s[2], sl, ov)]


def test_slice_equals_the_restatement_and_the_executed_reference(ctx):
    g, cases = U.fixture()
    for k, c in enumerate(cases):
        clip = g[f"in_{c['input']}"]
        ct = havc.HAVC_clip_slice(clip, c["slices"], c["overlap_x"], c["overlap_y"])
        assert [ct.base_tile_w, ct.base_tile_h, ct.overlap_x, ct.overlap_y] == c["numbers"] and ct.clip_orig is clip
        want = U.fixture_tiles(g, k, c["slices"])
        assert len(ct.tiles) == c["slices"]
        for t, (a, b) in enumerate(zip(ct.tiles, want)):
            assert isinstance(a, np.ndarray) and a.dtype == np.uint8 and a.shape == b.shape and np.array_equal(a, b), (c, t)
    geoms = _geometries()
    assert len(geoms) >= 20
    for (n, h, w), slices, ov in geoms:
        clip = U.clip(n * h + w + ov, n, h, w)
        want, *numbers = U.slice_np(clip, slices, ov + 1, ov + 1)                                # odd overlaps in: rounded down to even
        ct = havc.HAVC_clip_slice(clip, slices, ov + 1, ov + 1)
        assert [ct.base_tile_w, ct.base_tile_h, ct.overlap_x, ct.overlap_y] == numbers
        for a, b in zip(ct.tiles, want):
            assert np.array_equal(a, b), (n, h, w, slices, ov)
        dclip = DeviceImage.from_numpy(ctx, clip)
        dt = havc.HAVC_clip_slice(dclip, slices, ov, ov)
        assert dt.clip_orig is dclip and all(isinstance(t, DeviceImage) and t.shape == b.shape for t, b in zip(dt.tiles, want))
        for a, b in zip(dt.tiles, want):
            assert np.array_equal(a.numpy(), b), (n, h, w, slices, ov)
        assert np.array_equal(dclip.numpy(), clip)                                               # the input is left alone
    # one frame in, one-frame tiles out; a device frame view at an odd byte offset into its stack
    clip = U.clip(3, 3, 37, 51)
    want = U.slice_np(clip[1:2], 4, 6, 2)[0]
    one = havc.HAVC_clip_slice(clip[1], 4, 6, 2)
    assert all(t.shape == b.shape[1:] and np.array_equal(t, b[0]) for t, b in zip(one.tiles, want))
    done = havc.HAVC_clip_slice(DeviceImage.from_numpy(ctx, clip).frame(1), 4, 6, 2)
    assert all(isinstance(t, DeviceImage) and t.shape == b.shape[1:] and np.array_equal(t.numpy(), b[0]) for t, b in zip(done.tiles, want))


def _random_tiles(seed, n, h, w, slices, ov):
    """tiles of a slice's geometry filled with INDEPENDENT random bytes: seams and the two roundings only show when the tiles differ"""
    base_w, base_h = (w + 1) // 2, ((h + 1) // 2 if slices == 4 else h)
    oy = ov if slices == 4 else 0
    r = np.random.default_rng(seed)
    tiles = [r.integers(0, 256, (n, base_h + oy, base_w + ov, 3), dtype=np.uint8) for _ in range(slices)]
    orig = r.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    return havc.ClipTiles(orig, tiles, base_w, base_h, ov, oy)


def test_reconstruct_equals_the_restatement(ctx):
    """every geometry x every blend weight, chroma_resize off and on; with it on the fused launch also equals the existing entry point
    (imfilters.chroma_post_process_np) applied to its own output without it"""
    differs = 0
    for i, ((n, h, w), slices, ov) in enumerate(_geometries()):
        ct = _random_tiles(100 + i, n, h, w, slices, ov)
        args = (ct.tiles, ct.clip_orig, ct.base_tile_w, ct.base_tile_h, ct.overlap_x, ct.overlap_y)
        for weight in WEIGHTS:
            want = U.reconstruct_np(*args, weight, False)
            got = havc.HAVC_clip_reconstruct(ct, weight, False)
            assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == (n, h, w, 3)
            assert np.array_equal(got, want), (n, h, w, slices, ov, weight, int((got != want).sum()))
            luma = havc.HAVC_clip_reconstruct(ct, weight, True)
            assert np.array_equal(luma, U.reconstruct_np(*args, weight, True)), (n, h, w, slices, ov, weight)
            rows = F.chroma_post_process_np(ctx, got.reshape(n * h, w, 3), ct.clip_orig.reshape(n * h, w, 3))
            assert np.array_equal(luma, rows.reshape(n, h, w, 3)), (n, h, w, slices, ov, weight)
            differs += bool((luma != got).any())
        if ov:                                                                                   # the ramp and the constants are different blends
            assert (havc.HAVC_clip_reconstruct(ct, 0) != havc.HAVC_clip_reconstruct(ct, 0.5)).any()
    assert differs > 0
    # without clip_orig nothing is cropped: the full 2 * base size
    ct = _random_tiles(7, 2, 37, 51, 4, 6)
    ct.clip_orig = None
    got = havc.HAVC_clip_reconstruct(ct, 0.3)
    assert got.shape == (2, 38, 52, 3) and np.array_equal(got, U.reconstruct_np(ct.tiles, None, 26, 19, 6, 6, 0.3))


def test_device_and_mixed_operands_and_single_frames(ctx):
    for i, ((n, h, w), slices, ov) in enumerate(_geometries()):
        ct = _random_tiles(300 + i, n, h, w, slices, ov)
        weight, luma = WEIGHTS[i % len(WEIGHTS)], bool(i % 2)
        want = havc.HAVC_clip_reconstruct(ct, weight, luma)                                      # host path: checked against the restatement above
        dev = havc.ClipTiles(DeviceImage.from_numpy(ctx, ct.clip_orig), [DeviceImage.from_numpy(ctx, t) for t in ct.tiles], ct.base_tile_w,
                             ct.base_tile_h, ct.overlap_x, ct.overlap_y)
        got = havc.HAVC_clip_reconstruct(dev, weight, luma)
        assert isinstance(got, DeviceImage) and got.shape == (n, h, w, 3) and np.array_equal(got.numpy(), want), (n, h, w, slices, ov)
        mixed = havc.ClipTiles(ct.clip_orig if i % 3 else dev.clip_orig, [t if (j + i) % 2 else d for j, (t, d) in enumerate(zip(ct.tiles, dev.tiles))],
                               ct.base_tile_w, ct.base_tile_h, ct.overlap_x, ct.overlap_y)
        got = havc.HAVC_clip_reconstruct(mixed, weight, luma)
        assert isinstance(got, DeviceImage) and np.array_equal(got.numpy(), want), (n, h, w, slices, ov)
        for t, d in zip(ct.tiles, dev.tiles):
            assert np.array_equal(d.numpy(), t)                                                  # the tiles are left alone
        # frame 0 alone, as single frames: host, and device views
        one = havc.ClipTiles(ct.clip_orig[0], [t[0] for t in ct.tiles], ct.base_tile_w, ct.base_tile_h, ct.overlap_x, ct.overlap_y)
        got = havc.HAVC_clip_reconstruct(one, weight, luma)
        assert got.shape == (h, w, 3) and np.array_equal(got, want[0])
        k = n - 1                                                                                # the last frame: a view at an odd byte offset when n > 1
        done = havc.ClipTiles(dev.clip_orig.frame(k), [d.frame(k) for d in dev.tiles], ct.base_tile_w, ct.base_tile_h, ct.overlap_x, ct.overlap_y)
        got = havc.HAVC_clip_reconstruct(done, weight, luma)
        assert isinstance(got, DeviceImage) and got.shape == (h, w, 3) and np.array_equal(got.numpy(), want[k])


def test_reconstruct_of_a_slice_is_the_clip_on_the_device(ctx):
    for (n, h, w), slices, ov in _geometries():
        clip = U.clip(h * w + ov, n, h, w)
        dclip = DeviceImage.from_numpy(ctx, clip)
        for weight in WEIGHTS:
            back = havc.HAVC_clip_reconstruct(havc.HAVC_clip_slice(dclip, slices, ov, ov), weight)
            assert isinstance(back, DeviceImage) and np.array_equal(back.numpy(), clip), (n, h, w, slices, ov, weight)
    # with chroma_resize the clip's own luma goes under its own chroma: cv2's YUV round trip is not the identity on every RGB triple, the result is the
    # library's chroma_post_process(clip, clip)
    clip = U.clip(11, 2, 37, 51)
    want = F.chroma_post_process_np(ctx, clip.reshape(74, 51, 3), clip.reshape(74, 51, 3)).reshape(clip.shape)
    assert np.array_equal(havc.HAVC_clip_reconstruct(havc.HAVC_clip_slice(clip, 4, 6, 6), 0, True), want)


def test_a_bad_geometry_launches_nothing(ctx):
    clip = U.clip(1, 2, 20, 30)
    tiles = [np.full((2, 12, 17, 3), 7, np.uint8) for _ in range(4)]
    out = np.full_like(clip, 7)
    ptrs = (C.c_void_p * 4)(*[nat.as_ptr(t) for t in tiles])
    good = dict(width=30, height=20, n_frames=2, n_tiles=4, base_w=15, base_h=10, overlap_x=2, overlap_y=2, mask_val=128, recover_luma=0)
    for field, value in (("n_tiles", 3), ("n_tiles", 0), ("overlap_x", 15), ("overlap_x", -2), ("overlap_y", 10), ("overlap_y", -1), ("base_w", 14),
                         ("base_h", 9), ("width", 31), ("height", 0), ("n_frames", 0), ("mask_val", 256), ("mask_val", -1)):
        geom = nat.TileGeom(**dict(good, **{field: value}))
        ctx.synchronize()
        before = ctx.stats().launches
        for name, call in ((b"tile_slice", lambda: ctx.lib.havc_tile_slice(ctx.h, nat.as_ptr(clip), ptrs, C.byref(geom))),
                           (b"tile_reconstruct", lambda: ctx.lib.havc_tile_reconstruct(ctx.h, ptrs, nat.as_ptr(clip), nat.as_ptr(out), C.byref(geom)))):
            rc = call()                                                                          # (the error text is that of the LAST call)
            assert rc == nat.HAVC_E_INVALID == -1, (field, value, rc)
            assert name in ctx.lib.havc_last_error(ctx.h)
        assert ctx.stats().launches == before and (out == 7).all() and all((t == 7).all() for t in tiles), (field, value)
    two = nat.TileGeom(**dict(good, n_tiles=2))                                                  # 2 tiles: base_h = height and overlap_y = 0
    assert ctx.lib.havc_tile_slice(ctx.h, nat.as_ptr(clip), ptrs, C.byref(two)) == -1
    geom = nat.TileGeom(**dict(good, recover_luma=1))
    assert ctx.lib.havc_tile_reconstruct(ctx.h, ptrs, None, nat.as_ptr(out), C.byref(geom)) == -1                      # luma without its source
    assert ctx.lib.havc_tile_reconstruct(ctx.h, ptrs, nat.as_ptr(clip), nat.as_ptr(tiles[1]), C.byref(geom)) == -1     # out is a tile
    assert ctx.lib.havc_tile_reconstruct(ctx.h, ptrs, nat.as_ptr(clip), nat.as_ptr(clip), C.byref(geom)) == -1         # out is clip_orig
    assert ctx.lib.havc_tile_reconstruct(ctx.h, ptrs, nat.as_ptr(clip), nat.as_ptr(out), None) == -1
    with pytest.raises(havc.HAVCError):
        havc.HAVC_clip_slice(clip, 4, 16, 2)                                                     # the Python layer refuses the same, earlier
    # each call is ONE launch
    ctx.synchronize()
    before = ctx.stats().launches
    ct = havc.HAVC_clip_slice(clip, 4, 2, 2)
    havc.HAVC_clip_reconstruct(ct, 0, True)
    assert ctx.stats().launches == before + 2


def test_tiled_colorization_end_to_end(ctx):
    """the VerySlow loop (__init__.py:862-870) with seeded weights: slice into 2 tiles, HAVC_colorizer on each, reconstruct with the linear ramp and the
    clip's luma -- the device path stays in HBM and carries the bytes of the host path"""
    from tests.test_havc_harness import _frame, _weights
    sds, _ = _weights()
    clip = np.stack([_frame(21, 120, 256), _frame(22, 120, 256)])                                # tiles 120 x 160: render factor 10's own frame size
    kw = dict(method=0, deoldify_p=(0, 10, 1.0, 0.0), state_dicts=sds)

    def run(c):
        ct = havc.HAVC_clip_slice(c, slices=2, overlap_x=32, overlap_y=32)
        assert (ct.base_tile_w, ct.base_tile_h, ct.overlap_x, ct.overlap_y) == (128, 120, 32, 0)
        for i in range(2):
            ct.tiles[i] = havc.HAVC_colorizer(ct.tiles[i], **kw)
        return ct, havc.HAVC_clip_reconstruct(ct, blend_weight=0, chroma_resize=True)
    hct, host = run(clip)
    assert isinstance(host, np.ndarray) and host.shape == clip.shape and host.dtype == np.uint8
    assert np.array_equal(host, U.reconstruct_np(hct.tiles, clip, 128, 120, 32, 0, 0, True))      # the blend of the GPU's own tiles, restated
    assert (host != clip).any()
    dct, dev = run(DeviceImage.from_numpy(ctx, clip))
    assert all(isinstance(t, DeviceImage) for t in dct.tiles)
    assert isinstance(dev, DeviceImage) and dev.shape == clip.shape
    assert np.array_equal(dev.numpy(), host)
