"""-m gpu: what HAVC_restore_video adds, each part against its own reference, then the entry point against the composition of the parts.

  * Spline36 (havc_resize_n, filter 1) on every horizontal kernel variant, all bytes against the float64 reference of tests/restore_util.py under the rule of
    tests/resize_util.py (exact outside near-ties, either neighbour inside them); the variant of each case is asserted first (havc_resize_plan_filter).
    Spline64 through the new entry point gives the bytes of havc_spline64_resize_n.
  * Pillow LANCZOS (havc_pil_resize, resample 1): every byte equal to PIL.Image.resize(..., LANCZOS) computed here, from host and from device operands.
  * DeepRemaster's clip mode (remaster_render.RemasterClipRender) on tests/golden/restore_video.npz (the reference's RemasterColorizer on the CPU): `ab` and
    the u8 frames of every call within 3 x the fixture's fp16-operand floor, as tests/test_gpu_remaster.py derives its limits; the window numbers equal the
    reference's; the run blended at 0.4 (LANCZOS + Image.blend) under the same limits.
  * HAVC_restore_video: ex_model 2 byte-equal to Spline36 -> scene_detect -> clip-mode render -> Spline64 with luma -> luma recovery, host and device clips
    the same bytes; ex_model 0 byte-equal to HAVC_deepex on the scenes of clip_ref (method 6) and to the hand-driven loop, blended at 0.5 outside the scene changes of
    clip_ref, not of the clip (method 5, ref_merge 3); max_memory_frames > 0 leaves render_vivid on there.
"""
import os

import numpy as np
import pytest

from oracle import imaging
from tests import resize_util as RU
from tests import restore_util as U
from vsdeoldify_amd import _native as nat
from vsdeoldify_amd import havc
from vsdeoldify_amd import imfilters as F
from vsdeoldify_amd import scdetect as SD
from vsdeoldify_amd.device import DeviceImage
from vsdeoldify_amd.synth import synth_remaster_state_dict

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FACTOR = 3.0


# ---- Spline36 ----
@pytest.mark.parametrize("name", list(U.CASES))
def test_spline36_every_variant_against_float64(ctx, name):
    c = U.CASES[name]
    taps, variant, span_lds = U.plan(ctx.lib, c.sw, c.dw, c.n * c.sh, U.SPLINE36)
    assert (taps, variant) == (c.taps, c.variant), (name, taps, variant, span_lds)
    clip, luma = U.case_operands(name)
    ref = U.ref36(clip, c.dw, c.dh)
    sat = int(((ref.v > 255.5) | (ref.v < -0.5)).sum())
    print(f"spline36 case {name}: variant {variant}, {taps} taps, span {span_lds} bytes of LDS, {sat} values saturate")
    if name in ("a", "b", "c"):                 # up-sampled or merely halved, the 0 / 255 frame overshoots
        assert sat > 500 and ref.v[0].max() > 270 and ref.v[0].min() < -15
    label = f"spline36 case {name}"
    tie = RU.assert_near_tie_share(ref, label, per_pixel=c.luma)          # from the reference alone, before the GPU output exists
    got = havc.spline36(ctx, clip, c.dw, c.dh, luma_from=luma)
    if c.luma:
        RU.check_fused(got, ref, tie, luma, label)
    else:
        RU.check_bytes(got, ref, tie, label)
    if name == "b":                             # device operands: the same bytes
        dev = havc.spline36(ctx, DeviceImage.from_numpy(ctx, clip), c.dw, c.dh, luma_from=DeviceImage.from_numpy(ctx, luma))
        assert isinstance(dev, DeviceImage) and np.array_equal(dev.numpy(), got)


def test_spline64_through_the_new_entry_point_is_unchanged(ctx):
    from tests.test_gpu_resize import CASES
    c = CASES["b"]
    assert U.plan(ctx.lib, c.sw, c.dw, c.n * c.sh, U.SPLINE64)[:2] == (c.taps, c.variant)
    r = np.random.default_rng(c.seed)
    clip = r.integers(0, 256, (c.n, c.sh, c.sw, 3), dtype=np.uint8)
    luma = r.integers(0, 256, (c.n, c.dh, c.dw, 3), dtype=np.uint8)
    old = havc.spline64(ctx, clip, c.dw, c.dh, luma_from=luma)                                     # havc_spline64_resize_n
    new = havc._resize(ctx, clip, c.dw, c.dh, luma, nat.RESIZE_SPLINE64)                           # havc_resize_n(filter 0)
    assert np.array_equal(old, new)
    assert not np.array_equal(old, havc.spline36(ctx, clip, c.dw, c.dh, luma_from=luma))


# ---- Pillow LANCZOS ----
# (sw, sh) -> (dw, dh): up; about 8 x down (49 taps); a long row squeezed 35 x (211 taps); down to one pixel; up from one pixel; identity; widths % 4 != 0
LANCZOS_SHAPES = [((33, 24), (48, 32)), ((455, 256), (57, 32)), ((1400, 9), (40, 9)), ((7, 5), (1, 1)), ((1, 1), (5, 3)), ((61, 83), (61, 83)),
                  ((13, 6), (10, 9)), ((10, 9), (13, 6))]


@pytest.mark.parametrize("case", range(len(LANCZOS_SHAPES)))
def test_lanczos_every_byte_equals_pillow_host_and_device(ctx, case):
    from PIL import Image
    from vsdeoldify_amd.remaster_render import lanczos_resize
    (sw, sh), (dw, dh) = LANCZOS_SHAPES[case]
    r = np.random.default_rng(100 + case)
    img = r.integers(0, 256, (sh, sw, 3), dtype=np.uint8)
    if sh > 2:
        img[: sh // 2] = r.integers(0, 2, img[: sh // 2].shape, dtype=np.uint8) * 255             # hard edges: the negative lobes clip at both ends
    want = np.asarray(Image.fromarray(img).resize((dw, dh), Image.LANCZOS))
    got = lanczos_resize(ctx, img, dw, dh)
    assert got.shape == want.shape and np.array_equal(got, want), (LANCZOS_SHAPES[case], int((got != want).sum()))
    dev = lanczos_resize(ctx, DeviceImage.from_numpy(ctx, img), dw, dh)
    assert isinstance(dev, DeviceImage) and np.array_equal(dev.numpy(), want)
    mixed = lanczos_resize(ctx, img, dw, dh, device=True)                                          # host frame in, device frame out
    assert isinstance(mixed, DeviceImage) and np.array_equal(mixed.numpy(), want)


def test_lanczos_several_frames_in_one_call(ctx):
    from PIL import Image
    from vsdeoldify_amd.remaster_render import lanczos_resize
    r = np.random.default_rng(200)
    clip = r.integers(0, 256, (3, 36, 54, 3), dtype=np.uint8)
    want = np.stack([np.asarray(Image.fromarray(f).resize((48, 32), Image.LANCZOS)) for f in clip])
    assert np.array_equal(lanczos_resize(ctx, clip, 48, 32), want)
    dev = lanczos_resize(ctx, DeviceImage.from_numpy(ctx, clip), 48, 32)
    assert isinstance(dev, DeviceImage) and dev.shape == want.shape and np.array_equal(dev.numpy(), want)


# ---- DeepRemaster clip mode on the fixture ----
@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "restore_video.npz"))


@pytest.fixture(scope="module")
def model(fx):
    from vsdeoldify_amd.remaster_net import RemasterColorNet
    return RemasterColorNet(synth_remaster_state_dict(int(fx["seed"])))


def check_u8(fx, name, got, label):
    de = imaging.delta_e00_images(got, fx[name])
    fl, st = fx[name + "_floor_de"], fx[name + "_step_de"]
    lim = [FACTOR * (fl[i] if fl[i] > 0 else st[i]) for i in (0, 1)]
    mean, p99 = float(de.mean()), float(np.percentile(de, 99))
    line = f"{label:28s} u8 dE00 mean {mean:.4f} (limit {lim[0]:.4f})   p99 {p99:.4f} (limit {lim[1]:.4f})   max {de.max():.3f}"
    print(line)
    assert mean <= lim[0] and p99 <= lim[1], line


def run_clip_mode(fx, model, clip, clip_ref, merge_weight):
    """the fixture's 14 frames through RemasterClipRender in batches of 2 -> (u8 frames, `ab` per call on the fixture's sub-sample, window numbers per call)"""
    from vsdeoldify_amd.remaster_render import RemasterClipRender
    N, k = clip.shape[0], int(fx["ab_stride"])
    r = RemasterClipRender(ref_minedge=int(fx["params"][0]), ref_buffer_size=int(fx["params"][1]), length=2, model=model)
    try:
        assert r.load_clip_ref(clip_ref, fx["flags"]) == int(fx["found"]) and (r.target_w, r.target_h) == tuple(fx["target_wh"])
        outs, abs_, trace = [], [], []
        for n0 in range(0, N, 2):
            outs.append(r.process_clip_frames(clip.frames(n0, n0 + 2) if isinstance(clip, DeviceImage) else clip[n0:n0 + 2], n0, min(n0 + 1, N - 1), merge_weight))
            abs_.append(r._session.tap("ab", 2).reshape(-1)[::k].astype(np.float64))
            trace.append(r.window.numbers())
    finally:
        r.close()
    outs = np.concatenate([o.numpy() if isinstance(o, DeviceImage) else o for o in outs])
    return outs, np.stack(abs_), trace


def check_ab(fx, ab):
    ref, floor = fx["ab"].astype(np.float64), fx["ab_floor"].astype(np.float64)
    assert ab.shape == ref.shape
    bad = []
    for call in range(len(ref)):
        e, f = np.abs(ab[call] - ref[call]), np.abs(floor[call] - ref[call])
        line = f"call {call} ab max {e.max():.3e} (floor {f.max():.3e}, x{e.max() / f.max():.2f})   mean {e.mean():.3e} (floor {f.mean():.3e}, x{e.mean() / f.mean():.2f})"
        print(line)
        if not (e.max() <= FACTOR * f.max() and e.mean() <= FACTOR * f.mean()):
            bad.append(line)
    assert not bad, "\n".join(bad)


def test_clip_mode_follows_the_reference_colorizer(ctx, fx, model):
    out, ab, trace = run_clip_mode(fx, model, fx["clip"], fx["clip_ref"], 1.0)
    assert trace == fx["trace"].tolist()
    check_ab(fx, ab)
    check_u8(fx, "out", out, "clip mode")


def test_clip_mode_blended_with_the_reference_clip(ctx, fx, model):
    out, ab, trace = run_clip_mode(fx, model, fx["clip"], fx["clip_ref"], float(fx["merge_weight"]))
    assert trace == fx["trace"].tolist()
    check_ab(fx, ab)
    check_u8(fx, "merged", out, "clip mode, merged at 0.4")
    assert not np.array_equal(out, fx["out"])
    # device-resident clip and clip_ref: stills and blend operands never leave HBM; the same bytes
    dout, _, dtrace = run_clip_mode(fx, model, DeviceImage.from_numpy(ctx, fx["clip"]), DeviceImage.from_numpy(ctx, fx["clip_ref"]), float(fx["merge_weight"]))
    assert dtrace == trace and np.array_equal(dout, out)


# ---- HAVC_restore_video ----
def test_restore_video_remaster_equals_the_composition_of_its_parts(ctx, fx, model):
    from vsdeoldify_amd.remaster_render import RemasterClipRender, resize_for_inference_size
    clip, clip_ref = fx["clip"], fx["clip_ref"]
    N, h, w = clip.shape[:3]
    assert clip_ref.shape[1:3] == (36, 54) != (h, w)
    kw = dict(ex_model=2, render_vivid=False, frame_mindim=32, ref_minedge=24, max_memory_frames=4, ref_freq=3, model=model)
    for method, ref_merge in ((6, 0), (5, 2)):
        dbg = {}
        got = havc.HAVC_restore_video(clip, clip_ref, method=method, ref_merge=ref_merge, debug=dbg, **kw)
        assert got.shape == clip.shape and got.dtype == np.uint8
        # the parts, each pinned on its own
        ref36 = havc.spline36(ctx, clip_ref, w, h)
        detected = SD.scene_detect(ctx, ref36, threshold=0.10, frequency=3)
        assert np.array_equal(dbg["clip_ref"], ref36)
        if ref_merge:
            flags, weight = detected.scene_change_prev, 0.4
            assert np.array_equal(dbg["clip_sc"].scene_change_prev, flags) and dbg["scenes"].scene_change_prev.all() and dbg["ref_weight"] == 0.4
        else:
            flags, weight = detected.scene_change_prev, 1.0
            assert np.array_equal(dbg["scenes"].scene_change_prev, flags) and dbg["clip_sc"] is None and dbg["ref_weight"] == 1.0
        assert int(flags.sum()) >= 5                                                               # more references than the 4 slots: the window advances
        fw, fh = resize_for_inference_size(w, h, 32)
        small = havc.spline64(ctx, clip, fw, fh)
        eng = RemasterClipRender(ref_minedge=24, ref_buffer_size=4, length=2, model=model)
        try:
            eng.load_clip_ref(ref36, flags)
            first = eng.window.numbers()
            col = np.concatenate([eng.process_clip_frames(small[n0:n0 + 2], n0, min(n0 + 1, N - 1), weight) for n0 in range(0, N, 2)])
            assert eng.window.numbers() != first
        finally:
            eng.close()
        up = havc.spline64(ctx, col, w, h, luma_from=clip)
        want = np.stack([F.chroma_post_process_np(ctx, up[i], clip[i]) for i in range(N)])
        assert np.array_equal(got, want), (method, int((got != want).sum()))
        assert not np.array_equal(got, clip)
        dev = havc.HAVC_restore_video(DeviceImage.from_numpy(ctx, clip), DeviceImage.from_numpy(ctx, clip_ref), method=method, ref_merge=ref_merge, **kw)
        assert isinstance(dev, DeviceImage) and np.array_equal(dev.numpy(), got)


def test_restore_video_remaster_needs_four_references(ctx, fx, model):
    still = np.repeat(fx["clip_ref"][:1], 6, 0)                                                    # no scene change: frames 0 and 4 by frequency alone
    with pytest.raises(havc.HAVCError, match="number of reference frames must be at least 2, found  2"):
        havc.HAVC_restore_video(fx["clip"][:6], still, ex_model=2, render_vivid=False, frame_mindim=32, ref_minedge=24, ref_freq=4, model=model)


def _cmn_clips(n=6, h=72, w=128, hr=54, wr=96, cut=2, cut_ref=3):
    """gray master with a cut at frame `cut` and a coloured reference video at another size whose cut comes one frame later, at `cut_ref` (both 16:9: no
    borders): scenes detected on the master differ from scenes detected on clip_ref"""
    r = np.random.default_rng(11)

    def frames(hh, ww, c):
        yy, xx = np.mgrid[0:hh, 0:ww] * (h / hh)
        tex = [95 + 50 * np.sin(xx / 9.0 + yy / 5.0), 150 + 40 * np.cos(xx / 4.0 - yy / 11.0)]
        return np.stack([np.clip(tex[0 if i < c else 1] + 2 * i + r.integers(-3, 4, (hh, ww)), 0, 255) for i in range(n)]).astype(np.uint8)

    clip = np.stack([frames(h, w, cut)] * 3, -1)
    g = np.stack([frames(hr, wr, cut_ref)] * 3, -1).astype(np.float32)
    tint = np.array([[1.10, 0.92, 0.70], [0.75, 1.0, 1.15]])
    ref = np.stack([np.clip(g[i] * tint[0 if i < cut_ref else 1] + [12, 0, 8], 0, 255) for i in range(n)]).astype(np.uint8)
    return clip, ref


def _cmn_by_hand(net, clip, ref36, ref_frames, weight=None, **kw):
    """DeepExColorMNet driven by hand: the frames in ref_frames hand their (squashed) clip_ref frame over as the new reference; with a weight every other
    frame is blended with its squashed clip_ref frame (colorize_frame's own steps are pinned by tests/test_gpu_deepex.py)"""
    from vsdeoldify_amd.colormnet_render import DeepExColorMNet
    dx = DeepExColorMNet(vid_length=len(clip), render_speed="medium", network=net, **kw)
    out = []
    for i in range(len(clip)):
        small = dx._squash(ref36[i])[0]
        out.append(np.asarray(dx.colorize_frame(clip[i], ref_small=small if i in ref_frames else None,
                                                blend=(small, weight) if (weight is not None and i not in ref_frames) else None)))
    return np.stack(out), dx


def test_restore_video_colormnet_takes_its_scenes_from_clip_ref(ctx):
    from tests.test_colormnet_net import gpu_network
    net = gpu_network()
    clip, ref = _cmn_clips()
    n, h, w = clip.shape[:3]
    ref36 = havc.spline36(net.ctx, ref, w, h)
    scenes = havc.HAVC_SceneDetect(ref36, 0.10)
    assert list(np.flatnonzero(scenes.scene_change_prev)) == [0, 3]
    assert list(np.flatnonzero(havc.HAVC_SceneDetect(clip, 0.10).scene_change_prev)) == [0, 2]   # the master's own cut sits elsewhere
    # method 6: HAVC_deepex on clip_ref's own scenes, and the hand-driven loop with references at frames 0 and 3
    want = havc.HAVC_deepex(clip, ref36, method=0, scenes=scenes, network=net)
    got = havc.HAVC_restore_video(clip, ref, network=net)
    assert got.shape == clip.shape and np.array_equal(got, want) and not np.array_equal(got[4], clip[4])
    assert np.array_equal(got, _cmn_by_hand(net, clip, ref36, (0, 3))[0])
    dev = havc.HAVC_restore_video(DeviceImage.from_numpy(net.ctx, clip), DeviceImage.from_numpy(net.ctx, ref), network=net)
    assert isinstance(dev, DeviceImage) and np.array_equal(dev.numpy(), got)
    # method 5, ref_merge 3: every clip_ref frame is a reference; clip_sc is detected on CLIP_REF (frames 0 and 3), those frames set the reference and stay
    # unblended, the others are blended at 0.5.  HAVC_deepex detects clip_sc on the clip (frames 0 and 2) and gives other bytes.
    dbg, dbg_dx = {}, {}
    got5 = havc.HAVC_restore_video(clip, ref, method=5, ref_merge=3, network=net, debug=dbg)
    assert list(np.flatnonzero(dbg["clip_sc"].scene_change_prev)) == [0, 3] and dbg["scenes"].scene_change_prev.all() and dbg["ref_weight"] == 0.5
    assert np.array_equal(got5, _cmn_by_hand(net, clip, ref36, (0, 3), 0.5)[0])
    every = SD.SceneInfo(np.ones(n, np.int8), np.zeros(n, np.int8), np.full(n, 0.5), np.zeros(n), 0.10, 1)
    on_clip = havc.HAVC_deepex(clip, ref36, method=0, ref_merge=3, scenes=every, network=net, debug=dbg_dx)
    assert list(np.flatnonzero(dbg_dx["clip_sc"].scene_change_prev)) == [0, 2] and not np.array_equal(got5, on_clip)
    assert np.array_equal(on_clip, _cmn_by_hand(net, clip, ref36, (0, 2), 0.5)[0])
    for i in range(n):                                                                             # the same references as method 6: only the blend differs
        assert np.array_equal(got5[i], got[i]) == (i in (0, 3)), i


def test_restore_video_colormnet_keeps_render_vivid_with_a_memory_limit(ctx):
    """max_memory_frames > 0 switches render_vivid off in HAVC_deepex alone (__init__.py:1692-1693); HAVC_restore_video hands render_vivid on unchanged
    (:2099-2105), so ColorMNet's memory is reset at every reference update (reset_on_ref_update)"""
    from tests.test_colormnet_net import gpu_network
    net = gpu_network()
    clip, ref = _cmn_clips()
    n, h, w = clip.shape[:3]
    ref36 = havc.spline36(net.ctx, ref, w, h)
    scenes = havc.HAVC_SceneDetect(ref36, 0.10)
    got = havc.HAVC_restore_video(clip, ref, max_memory_frames=150, network=net)
    want, dx = _cmn_by_hand(net, clip, ref36, (0, 3), max_memory_frames=150, render_vivid=True)
    assert dx.render.reset_on_ref_update is True and dx.render.max_memory_frames == 150
    assert np.array_equal(got, want)
    plain, dx0 = _cmn_by_hand(net, clip, ref36, (0, 3), max_memory_frames=150, render_vivid=False)
    assert dx0.render.reset_on_ref_update is False
    assert np.array_equal(havc.HAVC_restore_video(clip, ref, max_memory_frames=150, render_vivid=False, network=net), plain)
    # HAVC_deepex keeps its override: the bytes of render_vivid=False whatever it is given
    assert np.array_equal(havc.HAVC_deepex(clip, ref36, method=0, scenes=scenes, max_memory_frames=150, render_vivid=True, network=net), plain)
    assert not np.array_equal(want[3:], plain[3:])                                                 # the reset at frame 3 shows
