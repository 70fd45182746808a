"""-m gpu: havc_recover_color_clip (csrc/recover.hip), mcomb.chroma_retention_merge_clip and HAVC_recover_clip_color against the CPU reference of
tests/recover_util.py (pinned to the executed reference by tests/test_recover_host.py) -- exact byte equality: the luma sums are integers and the pixel
arithmetic a stated float64 / float32 sequence -- except mask algorithms 1 and 2 (powf / exp: the rule of tests/test_tweaks.py).  The chroma_resize path is
compared with the composition of the library's own existing calls (the Spline64 stand-in has its own tests in tests/test_gpu_resize.py).

Shapes: 64 x 24 (1536 pixels: one block per launch), 16 x 8 x 17 frames (the binary selector's `n < 15`), 67 x 5 (335 pixels: no multiple of four, frames at odd
byte offsets, a tail group), 272 x 48 (the smallest width the size rule shrinks), 768 x 768 (a frame split over 72 / 576 blocks)."""
import ctypes as C
import itertools

import numpy as np
import pytest

from oracle import cvcolor
from tests import recover_util as U
from vsdeoldify_amd import _native as nat
from vsdeoldify_amd import havc, mcomb
from vsdeoldify_amd.device import DeviceImage

pytestmark = pytest.mark.gpu

H, W = 24, 64


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.uint8, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} bytes differ, first at {bad[0].tolist()}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}")


_CLIPS = {}


def clip4():
    """4 frames of 64 x 24: two inside the luma band, one dark, one bright"""
    if "c4" not in _CLIPS:
        a, b = U.make_clips([120, 90, 30, 225], (H, W), seed=11)
        assert [U.frame_is_standard(f) for f in a] == [True, True, False, False]
        _CLIPS["c4"] = (a, b)
    return _CLIPS["c4"]


def clip17(outside):
    """17 frames of 16 x 8; frame 15 or 16 outside the luma band"""
    key = ("c17", outside)
    if key not in _CLIPS:
        levels = [40 + 10 * k for k in range(15)] + ([130, 232] if outside == 16 else [25, 128])
        a, b = U.make_clips(levels, (8, 16), seed=13 + outside)
        assert [U.frame_is_standard(f) for f in a[15:]] == [outside != 15, outside != 16]
        _CLIPS[key] = (a, b)
    return _CLIPS[key]


def clip272():
    if "c272" not in _CLIPS:
        _CLIPS["c272"] = U.make_clips([110, 35, 150], (48, 272), seed=17)
    return _CLIPS["c272"]


def composition(ctx, a, b, sat, tht, strength, alpha, mask_weight, algo=0):
    """ChromaRetentionMerge(chroma_resize=True) out of the entry points that existed before the clip call: Spline64 down on both clips, the per-frame gradient
    selector (one luma read-back per frame), Spline64 up with the luma of a, simple_merge"""
    h, w = a.shape[1:3]
    fs = mcomb.recover_size(w)
    sa, sb = (a, b) if fs is None else (havc.spline64(ctx, a, fs, fs), havc.spline64(ctx, b, fs, fs))
    restored = np.stack([mcomb.chroma_retention_frame(x, y, sat, tht, mask_weight, alpha, False, algo) for x, y in zip(sa, sb)])
    if fs is not None:
        restored = havc.spline64(ctx, restored, w, h, luma_from=a)
    return mcomb.simple_merge(a.reshape(-1, w, 3), restored.reshape(-1, w, 3), strength).reshape(a.shape)


# ---- 1. gradient path, algo 0, no resize ----
@pytest.mark.parametrize("mask_weight,sat,alpha", list(itertools.product((1.0, 0.0, -0.3), (0.8, 1.0), (2, 6))))
def test_gradient_equals_cpu_reference(ctx, mask_weight, sat, alpha):
    a, b = clip4()
    got = havc.HAVC_recover_clip_color(a, b, sat=sat, alpha=alpha, mask_weight=mask_weight, chroma_resize=False)
    _same(got, U.recover_clip_color_ref(a, b, sat, 30, 1.0, alpha, mask_weight, False), (mask_weight, sat, alpha))


# ---- 2. the edges of the luma gate ----
def _frame_with_sum(value, total):
    """64 x 24 gray frame of `value` with single pixels moved by one count until the sum of Y is `total` (R = G = B = v has Y = v)"""
    f = np.full((H * W, 3), value, np.uint8)
    d = total - value * H * W
    assert abs(d) < H * W
    f[:abs(d)] += np.uint8(1) if d > 0 else np.uint8(255)                      # +1 or -1 (mod 256; 0 < value < 255)
    f = f.reshape(H, W, 3)
    assert int(cvcolor.rgb2yuv_u8(f)[..., 0].sum(dtype=np.int64)) == total
    return f


def test_gate_edges(ctx):
    npix = H * W
    assert npix == 1536

    def f_luma(s):
        return np.rint(s / npix / 255 * 1e6) / 1e6
    lo_out, lo_in, hi_in, hi_out = 86169, 86170, 305510, 305511
    assert 56 * npix < lo_out and lo_in < 57 * npix and 198 * npix < hi_in and hi_out < 199 * npix      # 56 / 199 lie outside the band, 57 / 198 inside
    assert f_luma(lo_out) == 0.219998 < 0.22 <= f_luma(lo_in) == 0.220001 and f_luma(hi_in) == 0.779999 <= 0.78 < f_luma(hi_out) == 0.780002     # one count of Y apart
    a = np.stack([_frame_with_sum(56, lo_out), _frame_with_sum(56, lo_in), _frame_with_sum(199, hi_in), _frame_with_sum(199, hi_out)])
    assert [U.frame_is_standard(f) for f in a] == [False, True, True, False]                              # neighbouring sums, different branches
    rng = np.random.default_rng(5)
    b = np.stack([U.make_donor(rng, (H, W)) for _ in range(4)])
    for binary in (False, True):
        want = U.selector_clip(a, b, 0.8, 30, 0.2, 2.0, False, binary, 0, 15)
        _same(mcomb.recover_color_clip(ctx, a, b, 0.8, 30, 0.2, 2.0, False, binary, 0, 15), want, ("gate", binary))
        # the two sides of an edge differ by far more than the moved pixels
        assert (np.abs(want[0].astype(int) - want[1]) > 4).mean() > 0.25 and (np.abs(want[2].astype(int) - want[3]) > 4).mean() > 0.25


# ---- 3. mask algorithms 1 and 2 ----
@pytest.mark.parametrize("algo", (1, 2))
def test_algos_1_and_2(ctx, algo):
    a, b = clip4()
    for kw in (dict(), dict(return_mask=True), dict(mask_weight=0.0, alpha=1.5, tht=25)):
        p = dict(sat=0.8, tht=40, alpha=2.0, mask_weight=1.0)
        p.update(kw)
        got = havc.HAVC_recover_clip_color(a, b, chroma_resize=False, algo=algo, **p)
        want = U.recover_clip_color_ref(a, b, p["sat"], p["tht"], 1.0, p["alpha"], p["mask_weight"], False, p.get("return_mask", False), False, algo)
        d = np.abs(got.astype(int) - want)
        print(f"algo {algo} {kw}: max |d| = {int(d.max())}, share of bytes that differ = {float((d > 0).mean()):.3e}")
        assert d.max() <= 1 and (d > 0).mean() < 2e-3, (algo, kw, int(d.max()), float((d > 0).mean()))


# ---- 4. binary path ----
@pytest.mark.parametrize("outside", (15, 16))
@pytest.mark.parametrize("mask_weight", (1.0, 0.0, -0.4))
def test_binary_path(ctx, mask_weight, outside):
    a, b = clip17(outside)
    got = havc.HAVC_recover_clip_color(a, b, mask_weight=mask_weight, binary_mask=True)
    _same(got[:15], a[:15], "frames 0..14 come back unchanged")
    want = U.recover_clip_color_ref(a, b, 0.8, 30, 1.0, 2.0, mask_weight, True, False, True)
    _same(got[15:], want[15:], ("binary", mask_weight, outside))
    if mask_weight != 1.0:                                                     # (weight 1 merges a frame inside the band back to the gray frame)
        assert not np.array_equal(got[15], a[15]) and not np.array_equal(got[16], a[16])
    got10 = mcomb.recover_color_clip(ctx, a, b, 0.8, 30, mask_weight, 2.0, False, True, 0, first_frame=10)
    _same(got10[:5], a[:5], "first_frame = 10: frames 0..4 unchanged")
    _same(got10, U.selector_clip(a, b, 0.8, 30, mask_weight, 2.0, False, True, 0, 10), "first_frame = 10")
    assert all(not np.array_equal(got10[i], a[i]) for i in range(5, 17) if mask_weight != 1.0 or not U.frame_is_standard(a[i]))


# ---- 5. return_mask ----
def test_return_mask(ctx):
    a, b = clip4()
    for kw in (dict(), dict(alpha=6, tht=50)):
        got = havc.HAVC_recover_clip_color(a, b, return_mask=True, chroma_resize=False, **kw)
        _same(got, U.recover_clip_color_ref(a, b, return_mask=True, chroma_resize=False, **kw), ("gradient mask", kw))
        assert (got[..., 0] == got[..., 1]).all() and (got[..., 0] == got[..., 2]).all()
    a17, b17 = clip17(16)
    got = havc.HAVC_recover_clip_color(a17, b17, return_mask=True, binary_mask=True, tht=40)
    _same(got, U.recover_clip_color_ref(a17, b17, tht=40, return_mask=True, binary_mask=True), "binary mask")
    _same(got[:15], a17[:15], "binary frames below 15 are the gray frame, not a mask")
    assert set(np.unique(got[15:]).tolist()) == {0, 255}
    a272, b272 = clip272()
    for binary in (False, True):
        got = havc.HAVC_recover_clip_color(a272, b272, strength=0.5, chroma_resize=True, return_mask=True, binary_mask=binary)
        want = U.selector_clip(a272, b272, 0.8, 30, 1.0, 2.0, True, binary)                              # the input size: no resize, no merge
        _same(got, want, ("272 wide mask", binary))


# ---- 6. the resize path ----
@pytest.mark.parametrize("strength", (1.0, 0.5))
def test_resize_path_equals_the_composition_of_existing_calls(ctx, strength):
    a, b = clip272()
    assert mcomb.recover_size(272) == 256
    got = havc.HAVC_recover_clip_color(a, b, strength=strength)
    _same(got, composition(ctx, a, b, 0.8, 30, strength, 2.0, 1.0), ("resize", strength))
    assert not np.array_equal(got, a)


# ---- 7. strength ----
def test_strength(ctx):
    a, b = clip4()
    restored = havc.HAVC_recover_clip_color(a, b, strength=1.0, chroma_resize=False)
    _same(restored, U.recover_clip_color_ref(a, b, chroma_resize=False), "strength 1")
    _same(havc.HAVC_recover_clip_color(a, b, strength=0, chroma_resize=False), a, "strength 0")
    half = havc.HAVC_recover_clip_color(a, b, strength=0.5, chroma_resize=False)
    _same(half, mcomb.simple_merge(a.reshape(-1, W, 3), restored.reshape(-1, W, 3), 0.5).reshape(a.shape), "strength 0.5")
    assert not np.array_equal(half, restored) and not np.array_equal(half, a)


# ---- 8. shapes and operands ----
def _c_call(ctx, gray, color, out, n, h, w, **kw):
    p = nat.RecoverParams(width=w, height=h, n_frames=n, first_frame=kw.get("first_frame", 0), sat=kw.get("sat", 0.8), tht=kw.get("tht", 30),
                          algo=kw.get("algo", 0), weight=kw.get("weight", 0.0), alpha=kw.get("alpha", 2.0), binary_mask=kw.get("binary_mask", 0),
                          return_mask=kw.get("return_mask", 0))
    return ctx.lib.havc_recover_color_clip(ctx.h, gray, color, out, C.byref(p))


def test_tail_group_and_guard_bytes(ctx):
    a, b = U.make_clips([120, 40, 200], (5, 67), seed=23)                      # 335 pixels a frame: 83 groups and 3 tail pixels, frames at odd offsets
    n, nb = 3, a.nbytes
    assert (5 * 67) % 4 == 3 and nb == 3015
    for binary in (0, 1):
        want = U.selector_clip(a, b, 0.8, 30, 0.3, 2.0, False, bool(binary), 0, 20)
        # host result behind a host guard
        out = np.full(nb + 64, 0xA5, np.uint8)
        assert _c_call(ctx, nat.as_ptr(a), nat.as_ptr(b), nat.as_ptr(out), n, 5, 67, weight=0.3, binary_mask=binary, first_frame=20) == nat.HAVC_OK
        _same(out[:nb].reshape(a.shape), want, ("host", binary))
        assert (out[nb:] == 0xA5).all()
        # device result: a buffer of n + 1 frames, the last one is the guard
        da, db = DeviceImage.from_numpy(ctx, a), DeviceImage.from_numpy(ctx, b)
        dout = DeviceImage.from_numpy(ctx, np.full((n + 1,) + a.shape[1:], 0xA5, np.uint8))
        assert _c_call(ctx, da.ptr, db.ptr, dout.ptr, n, 5, 67, weight=0.3, binary_mask=binary, first_frame=20) == nat.HAVC_OK
        res = dout.numpy()
        _same(res[:n], want, ("device", binary))
        assert (res[n] == 0xA5).all(), "bytes behind n * h * w * 3 were written"


def test_operand_kinds_single_frames_and_repeatability(ctx):
    a, b = clip4()
    want = havc.HAVC_recover_clip_color(a, b, chroma_resize=False, mask_weight=0.0)
    assert isinstance(want, np.ndarray)
    da, db = DeviceImage.from_numpy(ctx, a), DeviceImage.from_numpy(ctx, b)
    dgot = havc.HAVC_recover_clip_color(da, db, chroma_resize=False, mask_weight=0.0)
    assert isinstance(dgot, DeviceImage) and dgot.shape == a.shape
    _same(dgot.numpy(), want, "DeviceImage in / out")
    mixed = havc.HAVC_recover_clip_color(a, db, chroma_resize=False, mask_weight=0.0)
    assert isinstance(mixed, DeviceImage)
    _same(mixed.numpy(), want, "mixed operands")
    f = havc.HAVC_recover_clip_color(a[2], b[2], chroma_resize=False, mask_weight=0.0)
    assert f.shape == a.shape[1:]
    _same(f, want[2], "3-D frame")
    df = havc.HAVC_recover_clip_color(da.frame(3), db.frame(3), chroma_resize=False, mask_weight=0.0)
    assert isinstance(df, DeviceImage) and df.shape == a.shape[1:]
    _same(df.numpy(), want[3], "3-D device frame")
    _same(havc.HAVC_recover_clip_color(a[1:2], b[1:2], chroma_resize=False, mask_weight=0.0), want[1:2], "single-frame clip")
    _same(havc.HAVC_recover_clip_color(a, b, chroma_resize=False, mask_weight=0.0), want, "second run")
    a272, b272 = clip272()
    _same(havc.HAVC_recover_clip_color(a272, b272, strength=0.7), havc.HAVC_recover_clip_color(a272, b272, strength=0.7), "second run, resize path")


def test_frames_split_over_many_blocks(ctx):
    """768 x 768, the size chroma_resize works at for 1080p: 72 blocks add to a frame's luma slot; against the per-frame call (one sum, read back, per frame)"""
    rng = np.random.default_rng(29)
    base = np.stack([U.make_frame(rng, v, (96, 96)) for v in (120, 30)])
    a = np.ascontiguousarray(np.tile(base, (1, 8, 8, 1)))
    b = np.ascontiguousarray(np.tile(np.stack([U.make_donor(rng, (96, 96)) for _ in range(2)]), (1, 8, 8, 1)))
    assert a.shape == (2, 768, 768, 3) and [U.frame_is_standard(f) for f in base] == [True, False]
    got = mcomb.recover_color_clip(ctx, a, b, 0.8, 30, 0.0, 2.0)
    _same(got, np.stack([mcomb.chroma_retention_frame(x, y, 0.8, 30, 0.0, 2.0) for x, y in zip(a, b)]), "768 x 768")
    want_tile = U.selector_clip(base, np.ascontiguousarray(b[:, :96, :96]), 0.8, 30, 0.0, 2.0)          # per-pixel work + the same frame means
    _same(got[:, :96, :96], want_tile, "768 x 768, one tile against the CPU reference")


# ---- 9. method 6 ----
def test_method_6_routes_chroma_resize(ctx):
    a, b = clip272()
    w = 0.6
    got = havc.combine_models(a, b, 6, w, crt_p=[0.8, 30, 2, True, 0, 0])
    _same(got, mcomb.chroma_retention_merge_clip(a, b, 0.8, 30, w, 2, 0, True), "crt_p[3] = True")
    _same(got, composition(ctx, a, b, 0.8, 30, w, 2, 0), "crt_p[3] = True against the composition")
    plain = havc.combine_models(a, b, 6, w, crt_p=[0.8, 30, 2, False, 0, 0])
    restored = np.stack([mcomb.chroma_retention_frame(x, y, 0.8, 30, 0, 2, False, 0) for x, y in zip(a, b)])
    _same(plain, mcomb.simple_merge(a.reshape(-1, 272, 3), restored.reshape(-1, 272, 3), w).reshape(a.shape), "crt_p[3] = False: the per-frame path")
    assert not np.array_equal(plain, got)


# ---- 10. C ABI errors ----
def test_invalid_arguments_run_nothing(ctx):
    a, b = clip4()
    n, h, w = a.shape[:3]
    out = np.full(a.shape, 0x5A, np.uint8)
    pa, pb, po = nat.as_ptr(a), nat.as_ptr(b), nat.as_ptr(out)
    before = ctx.stats().launches
    bad = [dict(algo=3), dict(algo=-1), dict(n=0), dict(n=-2), dict(w=0), dict(h=0), dict(w=-64), dict(first_frame=-1),
           dict(gray=None), dict(color=None), dict(out=None), dict(out=pa), dict(out=pb),
           dict(out=C.c_void_p(pa.value + 3 * w)), dict(out=C.c_void_p(pb.value + a.nbytes - 1))]
    for kw in bad:
        rc = _c_call(ctx, kw.get("gray", pa), kw.get("color", pb), kw.get("out", po), kw.get("n", n), kw.get("h", h), kw.get("w", w),
                     **{k: v for k, v in kw.items() if k in ("algo", "first_frame")})
        assert rc == nat.HAVC_E_INVALID == -1, (kw, rc)
    assert ctx.lib.havc_recover_color_clip(ctx.h, pa, pb, po, None) == nat.HAVC_E_INVALID
    assert (out == 0x5A).all() and np.array_equal(a, clip4()[0]) and ctx.stats().launches == before
    with pytest.raises(ValueError, match="algo must be 0..2"):
        mcomb.recover_color_clip(ctx, a, b, algo=5)
    assert _c_call(ctx, pa, pb, po, n, h, w) == nat.HAVC_OK                    # and the valid call still works
    _same(out, U.selector_clip(a, b, 0.8, 30, 0.0, 2.0), "valid call after the refused ones")
