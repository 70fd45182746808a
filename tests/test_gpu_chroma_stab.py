"""-m gpu: havc_chroma_stab_clip / havc_reduce_flicker_clip (csrc/chroma_stab.hip, csrc/tweak.hip) and HAVC_stabilizer(stab=True) against the numpy definition of
tests/stab_util.py: every comparison is byte-equal, on host arrays and on a DeviceImage.

Sizes, h x w:   2 x 2      every tap is mirrored                  34 x 66    one band, partial tiles
                70 x 130   rows cross the 64-row band, columns cross two tiles
Frames: 1; 4 (all below 15, flicker passes every frame); 19 with first_frame = 0 for N = 3, 5, 15 (frames 15..18 are restored, 17 and 18 have clamped
neighbours) at the two smaller sizes.  chunk_frames 4 as well as 0: the halo of (N - 1) / 2 + 2 frames.  The clips (stab_util.make_clip) have frames
desaturated towards gray, a dark and a bright frame and a region oscillating from frame to frame; the tests assert from stab_util's own bookkeeping that the
reference takes and does not take the tht_scen gate and the luma band, that the flicker pass changes samples and that the scene walk replaces slots."""
import functools

import numpy as np
import pytest

from tests import stab_util as SU
from tests import stabilizer_util as STU
from vsdeoldify_amd import chroma_stab as CS
from vsdeoldify_amd import havc
from vsdeoldify_amd.device import DeviceImage
from vsdeoldify_amd.scdetect import SceneInfo

pytestmark = pytest.mark.gpu

SIZES = [(2, 2), (34, 66), (70, 130)]
SMALL = SIZES[:2]


def _same(got, want, what):
    bad = np.argwhere(got != want)
    print(what, "differing bytes:", len(bad))
    assert got.shape == want.shape and len(bad) == 0, (what, len(bad), bad[0].tolist(), int(got[tuple(bad[0])]), int(want[tuple(bad[0])]))


@functools.lru_cache(maxsize=None)
def _clip(h, w, n):
    c = SU.make_clip(h, w, n)
    c.setflags(write=False)
    return c


def _scenes(n):
    """scene changes at frame 1 and at the boundaries of chunks of four frames"""
    prev, nxt = np.zeros(n, np.int8), np.zeros(n, np.int8)
    for f in (1, 4, 8):
        if f < n:
            prev[f], nxt[f - 1] = 1, 1
    return SceneInfo(prev, nxt, np.full(n, 0.5), np.zeros(n), 0.1, 0)


def _both(ctx, clip, want, what, **kw):
    """host array in -> host array out, DeviceImage in -> DeviceImage out: the same bytes"""
    _same(CS.chroma_stab_np(ctx, clip, **kw), want, ("host",) + what)
    dev = CS.chroma_stab_np(ctx, DeviceImage.from_numpy(ctx, clip), **kw)
    assert isinstance(dev, DeviceImage)
    _same(dev.numpy(), want, ("device",) + what)


# ---- tht == 0: the temporal average with the scene walk --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [0, 4])
@pytest.mark.parametrize("h,w,n", [(h, w, n) for h, w in SIZES for n in (1, 4)] + [(h, w, 19) for h, w in SMALL])
def test_temporal_average(ctx, h, w, n, chunk):
    clip = _clip(h, w, n)
    for nframes, mode in ((3, "A"), (5, "W"), (15, "A")):
        for scenes in (None, _scenes(n)):
            for flicker in (False, True):
                book = {}
                want = SU.stab_stage(clip, nframes, mode, tht=0, scenes=scenes, flicker=flicker, book=book)
                if scenes is not None and n >= 4:
                    assert book["replaced"] > 0                                  # the scene walk replaces at least one slot
                if flicker and n == 19:
                    assert book["flicker_changed"] > 0
                _both(ctx, clip, want, (h, w, n, nframes, mode, scenes is not None, flicker, chunk), nframes=nframes, mode=mode, tht=0, scenes=scenes,
                      flicker=flicker, chunk_frames=chunk)


# ---- tht > 0: the shifted clips, restore_color with its gate, the list-form average ---------------------------------------------------------------------------------
RESTORE = [dict(mode="A", sat=1.0, weight=0.2, tht_scen=0.8), dict(mode="W", sat=0.5, weight=-0.3, tht_scen=0.5), dict(mode="A", sat=1.0, weight=0.0, tht_scen=0.8),
           dict(mode="W", sat=0.5, weight=0.6, tht_scen=1.0)]


@pytest.mark.parametrize("chunk", [0, 4])
@pytest.mark.parametrize("nframes", [3, 5, 15])
@pytest.mark.parametrize("h,w", SMALL)
def test_restored_average_19_frames(ctx, h, w, nframes, chunk):
    clip = _clip(h, w, 19)
    for k, kw in enumerate(RESTORE):
        flicker = k % 2 == 0
        book = {}
        want = SU.stab_stage(clip, nframes, tht=15, flicker=flicker, book=book, **kw)
        assert set(n for n, _ in book["gate"]) == {15, 16, 17, 18}              # what the n < 15 rule leaves
        if 0 < kw["tht_scen"] < 1:
            assert any(book["gate"].values()) and not all(book["gate"].values())  # the gate is taken, and not taken
        else:
            assert not any(book["gate"].values())
        if (h, w) != (2, 2):                                                     # four pixels: the dark / bright frames still decide the band
            assert any(book["band"].values()) and not all(book["band"].values())
        if flicker:
            assert book["flicker_changed"] > 0
        _both(ctx, clip, want, (h, w, nframes, chunk, k), nframes=nframes, tht=15, flicker=flicker, chunk_frames=chunk, **kw)


@pytest.mark.parametrize("h,w,n", [(h, w, n) for h, w in SIZES for n in (1, 4)])
def test_restored_average_short_clips(ctx, h, w, n):
    """every frame below 15: the shifted clips pass as they are, through both conversions; first_frame = 14 puts frames 1.. into the restored range"""
    clip = _clip(h, w, n)
    for first in (0, 14):
        for chunk in (0, 4):
            book = {}
            kw = dict(nframes=5, mode="W", sat=0.5, tht=15, weight=0.2, tht_scen=0.8, first_frame=first)
            want = SU.stab_stage(clip, flicker=True, book=book, **kw)
            assert bool(book.get("gate")) == (first == 14 and n > 1)
            _both(ctx, clip, want, (h, w, n, first, chunk), flicker=True, chunk_frames=chunk, **kw)


def test_flicker_alone(ctx):
    for shape in ((7, 3, 5, 3), (4, 2, 2, 3), (9, 34, 66, 3)):                   # 45 bytes per frame: the tail that is no group of four
        clip = np.random.default_rng(shape[1]).integers(0, 256, shape, dtype=np.uint8)
        clip[:, :2] = (clip[:, :2].astype(int) // 8 + np.arange(shape[0])[:, None, None, None] % 2 * 60 + 90).astype(np.uint8)
        book = {}
        want = SU.reduce_flicker(clip, book)
        assert (book["flicker_changed"] > 0) == (shape[0] >= 5)
        _same(CS.reduce_flicker_np(ctx, clip), want, ("flicker", shape))
        _same(CS.reduce_flicker_np(ctx, DeviceImage.from_numpy(ctx, clip)).numpy(), want, ("flicker device", shape))


def test_refusals_leave_the_output_alone(ctx):
    import ctypes as C
    from vsdeoldify_amd import _native as nat
    clip = _clip(34, 66, 4)
    out = np.full_like(clip, 7)

    def call(src, dst, **kw):
        p = nat.ChromaStabParams(width=66, height=34, n_frames=4, n_weights=5, sat=1.0, tht=15, weight=0.2, tht_scen=0.8)
        for k, v in enumerate([20] * 5):
            p.weights[k] = v
        for k, v in kw.items():
            setattr(p, k, v)
        return ctx.lib.havc_chroma_stab_clip(ctx.h, src, dst, C.byref(p))
    src, dst = nat.as_ptr(clip), nat.as_ptr(out)
    assert call(src, dst, width=65) == -1 and call(src, dst, height=0) == -1 and call(src, dst, width=4098) == -1 and call(src, dst, n_frames=0) == -1
    assert call(src, dst, n_weights=4) == -1 and call(src, dst, n_weights=1) == -1 and call(src, dst, n_weights=17) == -1
    assert call(None, dst) == -1 and call(src, None) == -1 and call(src, src) == -1
    assert ctx.lib.havc_chroma_stab_clip(ctx.h, src, dst, None) == -1
    assert (out == 7).all()
    assert call(src, dst) == 0 and (out != 7).any()


# ---- the public level ---------------------------------------------------------------------------------------------------------------------------------------------
def test_havc_stabilizer_equals_the_stage_by_stage_chain(ctx):
    """HAVC_stabilizer(clip, dark, smooth, stab) == spline64(flicker(stab(oracle chain(spline64(clip, fs, fs)))), w, h, luma_from=clip): the two resamples are the
    library's own entry point, the chain is the oracle's, stab and flicker are stab_util's"""
    _, _, table = STU.fixture()
    n, h, w = 19, 40, 66
    clip = np.stack([SU.make_clip(h, w, n)[i] // 2 + STU.colourful(5, n, h, w)[i] // 2 for i in range(n)])
    fs = min(24 * 16, w)
    sq = havc.spline64(ctx, clip, fs, fs)
    assert sq.shape == (n, fs, fs, 3)
    kw = dict(dark=True, smooth=True)
    chain = STU.oracle_chain(sq, *STU.parsed(table, **kw))
    for stab_p in ((5, "A", 1, 15, 0.2, 0.8), (7, "W", 0.8, 0, 0.2, 0.8)):
        book = {}
        col = SU.stab_stage(chain, *stab_p, book=book)
        assert book["flicker_changed"] > 0 and (stab_p[3] == 0 or book["gate"])
        want = havc.spline64(ctx, col, w, h, luma_from=clip)
        got = havc.HAVC_stabilizer(clip, stab=True, stab_p=stab_p, **kw)
        assert isinstance(got, np.ndarray) and got.dtype == np.uint8
        _same(got, want, ("HAVC_stabilizer", stab_p))
        assert (got != havc.HAVC_stabilizer(clip, **kw)).any()
    # the same call with the clip's scene changes (tht == 0: AverageFrames' scene walk)
    book = {}
    col = SU.stab_stage(chain, 7, "W", 0.8, 0, 0.2, 0.8, _scenes(n), book=book)
    assert book["replaced"] > 0
    got = havc.HAVC_stabilizer_scenes(clip, _scenes(n), stab=True, stab_p=(7, "W", 0.8, 0, 0.2, 0.8), **kw)
    _same(got, havc.spline64(ctx, col, w, h, luma_from=clip), "HAVC_stabilizer_scenes")
    assert (got != havc.HAVC_stabilizer(clip, stab=True, stab_p=(7, "W", 0.8, 0, 0.2, 0.8), **kw)).any()
    # stab_p[6], the hue adjustment: between the stabiliser and the flicker pass, on every frame (vs_adjust_clip_hue; the oracle's adjust_hue_range)
    from oracle import tweaks
    stab_p = (5, "A", 1, 15, 0.2, 0.8, "0:140|0.6,0.2")
    col = SU.chroma_stabilizer_ex(chain, *stab_p[:6])
    hued = np.stack([tweaks.adjust_hue_range(f, stab_p[6]) for f in col])
    assert (hued != col).any()
    for operand in (clip, DeviceImage.from_numpy(ctx, clip)):
        got = havc.HAVC_stabilizer(operand, stab=True, stab_p=stab_p, **kw)
        _same(got if isinstance(got, np.ndarray) else got.numpy(), havc.spline64(ctx, SU.reduce_flicker(hued), w, h, luma_from=clip), ("hue adjust", type(got)))
    dev = havc.HAVC_stabilizer(DeviceImage.from_numpy(ctx, clip), stab=True, **kw)
    assert isinstance(dev, DeviceImage)
    _same(dev.numpy(), havc.HAVC_stabilizer(clip, stab=True, **kw), "HAVC_stabilizer device")
