"""-m gpu: the per-pixel colour kernels over ALL 2^24 RGB inputs against the oracle (tests/sweep_util.py).

The claim "the u8 colour filters are bit-exact with the reference" is a chain: executed reference -> oracle (golden vectors), oracle -> definitions
(tests/test_cvcolor_sweep.py, tests/test_labcolor_sweep.py over the whole cube on the CPU), HIP kernels -> oracle.  The sample-image tests
(tests/test_tweaks.py, test_filters2.py, test_gpu_kernels.py) see about 10^-4 of the input space; the inputs on which a device build can disagree with
numpy or Pillow -- a tie of round(), a sextant boundary, a product just below an integer, a contracted multiply-add -- are rarer than that.  Every
single-image kernel takes one RGB triple per pixel, so the whole input space is one 4096 x 4096 image: it is swept here slab by slab (the same slab on
both sides, which also gives image_tweak's Contrast step eight different mean-L values), the two-image kernels against the cube under a bijection.

Integer / float64 per-pixel paths (csrc/pixel_ops.h through tweaks.hip, colorfilters.hip, stabilizer.hip): equal bytes, every pixel.
restore_color_gradient algo 1 / 2 (powf / exp): the rule of tests/test_tweaks.py, |d| <= 1 on fewer than 2e-3 of the bytes.
Lab kernels (csrc/zhang.hip, fp64 with the device libm): rgb -> Lab float32 planes bit-identical on all but 1e-6 of the values, Lab -> rgb equal bytes
except where the oracle's own value sits within 1e-9 of an integer (sweep_util), OP_PREP_LAB_L bit-equal on all but 1e-6 of the pixels.  The two caps
of 1e-6 are derived, not measured: the sides can differ only where the float64 value lies within libm noise (1e-15 relative) of a rounding boundary
of the narrower format (float32 spacing 6e-8 relative), an expected share of 1e-8; 1e-6 is a hundredfold margin.
OP_PREP_DDCOLOR (the imagenet-normalised RGB rendering of Lab(L, 0, 0), gray table g_gray_dd) is held to the same rule as OP_PREP_LAB_L.
Not covered: zhang_post_kernel and ddcolor_post_kernel are reachable only behind a whole network (ddcolor_post shares lab_to_rgb01 with the
Lab -> rgb sweep).

Every item counts the pixels it compared and asserts n == 1 << 24 (or the byte-pair count).  The CPU tests at the bottom check the helper itself."""
import numpy as np
import pytest

from oracle import colormnet_net as O
from oracle import imaging, pipeline, tweaks, zhang
from tests import sweep_util as su

P1, P2 = su.PARTNERS


def _sweep1(label, gpu, ref):
    """one-image kernel: gpu(slab) against ref(slab) over the cube"""
    n = 0
    for slab in su.cube_slabs():
        n += su.assert_same_bytes(gpu(slab), ref(slab), slab, label)
    print(f"{label}: n == {n}")
    assert n == su.N_CUBE
    return n


def _sweep2(label, gpu, ref, pair, swap=False):
    """two-image kernel: (cube, partner) -- or (partner, cube) -- slab by slab"""
    n = 0
    for slab in su.cube_slabs():
        a, b = slab, su.partner(slab, *pair)
        if swap:
            a, b = b, a
        n += su.assert_same_bytes(gpu(a, b), ref(a, b), (a, b), f"{label} K, c = {pair}{' swapped' if swap else ''}")
    print(f"{label}: n == {n}")
    assert n == su.N_CUBE
    return n


def _ids(cases):
    return [str(c).replace(" ", "") for c in cases]


# ---- 1: image_tweak (Pillow HSV hue shift, ImageEnhance Brightness / Contrast / Color, hue-range mask) ------------------------------------------------------
TWEAK = [dict(hue=35.0),                                               # the hue shift alone
         dict(hue=-120.0, sat=0.5),
         dict(sat=0.7, bright=10, hue=10, cont=0.9),                   # everything together
         dict(sat=2.5, cont=2.0, bright=100),                          # factors above 1: the extrapolating branch of pil_blendx
         dict(sat=0.3, cont=1.2, hue_range="green,280:360"),           # one named and one numeric range
         dict(sat=0.8, cont=0.6, bright=-60),                          # factors in (0.5, 1) whose float32 value lies above the decimal one, see blend below
         dict(hue=359.0, sat=0.0)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", TWEAK, ids=_ids(TWEAK))
def test_image_tweak_over_the_cube(ctx, case):
    from vsdeoldify_amd import imfilters as F
    _sweep1(f"image_tweak {case}", lambda s: F.image_tweak_np(ctx, s, **case), lambda s: tweaks.image_tweak(s, **case))


# ---- 2: image_chroma_tweak / adjust_hue_range (cv2 HSV, wrapping u8 casts, float64 merges) ----------------------------------------------------------------------
CTWEAK = [dict(hue=40, sat=0.6),
          dict(hue=-75, sat=3.0, bright=0.8),                          # sat > 1 and 1 + bright > 1 wrap the u8 cast
          dict(bright=-0.4),
          dict(sat=0.9, hue_adjust="rose,red|0.8,0.5"),                # adjust stage: saturation, positive weight
          dict(hue=20, hue_adjust="30:90|0.5,-0.3"),                   # negative weight
          dict(hue_adjust="blue|+40,0.2")]                             # hue-only second stage (the merge then goes back to the original)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CTWEAK, ids=_ids(CTWEAK))
def test_image_chroma_tweak_over_the_cube(ctx, case):
    from vsdeoldify_amd import imfilters as F
    _sweep1(f"image_chroma_tweak {case}", lambda s: F.image_chroma_tweak_np(ctx, s, **case), lambda s: tweaks.np_image_chroma_tweak(s, **case))


HUE_ADJUST = ["300:360|0.8,0.1", "green,30:60|-60,-0.4", "red|+30,0.3", "blue,cyan|1.6,0.0"]


@pytest.mark.gpu
@pytest.mark.parametrize("spec", HUE_ADJUST)
def test_adjust_hue_range_over_the_cube(ctx, spec):
    from vsdeoldify_amd import imfilters as F
    _sweep1(f"adjust_hue_range {spec}", lambda s: F.adjust_hue_range_np(ctx, s, spec), lambda s: tweaks.adjust_hue_range(s, spec))


# ---- 3: luma_adjusted_levels (two of the parameter sets of tests/test_tweaks.py; the frame luma differs per slab) ---------------------------------------------
LEVELS = [dict(luma_min=0.7, gamma=0.7, gamma_luma_min=0.9, gamma_alpha=0.5), dict(gamma=1.4, gamma_luma_min=0.8)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", LEVELS, ids=_ids(LEVELS))
def test_luma_adjusted_levels_over_the_cube(ctx, case):
    from vsdeoldify_amd import imfilters as F
    _sweep1(f"luma_adjusted_levels {case}", lambda s: F.luma_adjusted_levels_np(ctx, s, **case), lambda s: tweaks.luma_adjusted_levels(s, **case))


# ---- 4: the two-image YUV filters and luma merges: the cube against its partners ---------------------------------------------------------------------------------
PAIRS = [(P1, False), (P2, True)]
PAIR_IDS = ["cube-partner1", "partner2-cube"]


@pytest.mark.gpu
@pytest.mark.parametrize("pair,swap", PAIRS, ids=PAIR_IDS)
def test_chroma_post_process_over_the_cube(ctx, pair, swap):
    from vsdeoldify_amd import imfilters as F
    _sweep2("chroma_post_process", lambda a, b: F.chroma_post_process_np(ctx, a, b), pipeline.chroma_post_process, pair, swap)


@pytest.mark.gpu
@pytest.mark.parametrize("alpha,weight,pair,swap", [(0.15, 1.0) + PAIRS[0], (0.2, 0.6) + PAIRS[1]], ids=["0.15-1.0", "0.2-0.6"])
def test_chroma_stabilizer_over_the_cube(ctx, alpha, weight, pair, swap):
    from vsdeoldify_amd import imfilters as F
    _sweep2(f"chroma_stabilizer alpha {alpha} weight {weight}", lambda a, b: F.chroma_stabilizer_np(ctx, a, b, alpha, weight),
            lambda a, b: pipeline.chroma_stabilizer(a, b, alpha, weight), pair, swap)


@pytest.mark.gpu
@pytest.mark.parametrize("alpha,pair,swap", [(0.05,) + PAIRS[0], (0.2,) + PAIRS[1]], ids=["0.05", "0.2"])
def test_chroma_temporal_limiter_over_the_cube(ctx, alpha, pair, swap):
    from vsdeoldify_amd import imfilters as F
    _sweep2(f"chroma_temporal_limiter alpha {alpha}", lambda a, b: F.chroma_temporal_limiter_np(ctx, a, b, alpha),
            lambda a, b: pipeline.chroma_temporal_limiter(a, b, alpha), pair, swap)


# mode 0: hard mask at round(0.3 * 255); mode 1: the ramp of tests/test_filters2.py (threshold 66, gradient round(1 / (204 - 66), 3)); mode 2: luma / 255;
# mode 3: uint8(luma) / 255
def _luma_merge_fns(ctx, mode):
    from vsdeoldify_amd import imfilters as F
    if mode == 0:
        return lambda a, b: F.luma_merge_np(ctx, a, b, 0, round(0.3 * 255)), lambda a, b: pipeline.image_luma_merge(a, b, 0.3)
    if mode == 1:
        return lambda a, b: F.luma_merge_np(ctx, a, b, 1, 66, round(1 / (204 - 66), 3)), lambda a, b: pipeline.w_image_luma_merge(a, b, 0.26, 0.8)
    if mode == 2:
        return lambda a, b: F.luma_merge_np(ctx, a, b, 2), lambda a, b: pipeline.w_image_luma_merge(a, b, 0.0, 0.8)
    return lambda a, b: F.luma_merge_np(ctx, a, b, 3), lambda a, b: pipeline.image_luma_merge(a, b, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("pair,swap", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_luma_merge_over_the_cube(ctx, mode, pair, swap):
    gpu, ref = _luma_merge_fns(ctx, mode)
    _sweep2(f"luma_merge mode {mode}", gpu, ref, pair, swap)


@pytest.mark.gpu
@pytest.mark.parametrize("weights,order", [([25, 50, 25], (P1, None, P2)), ([10, 60, 30], (P2, None, P1))], ids=["25-50-25", "10-60-30"])
def test_color_temporal_stabilizer_over_the_cube(ctx, weights, order):
    """three frames: the cube in the middle, its two partners around it"""
    from vsdeoldify_amd import imfilters as F
    n = 0
    for slab in su.cube_slabs():
        frames = [slab if p is None else su.partner(slab, *p) for p in order]
        n += su.assert_same_bytes(F.color_temporal_stabilizer_np(ctx, frames, weights), pipeline.color_temporal_stabilizer(frames, weights), tuple(frames),
                                  f"color_temporal_stabilizer {weights}")
    print(f"color_temporal_stabilizer {weights}: n == {n}")
    assert n == su.N_CUBE


# ---- 5: chroma_stabilizer_adaptive reads a Laplacian neighbourhood of the stable frame: both sides see the same slab ----------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("base_tol,max_extra,weight,pair,swap", [(18, 22, 1.0) + PAIRS[0], (10, 40, 0.7) + PAIRS[1]], ids=["18-22-1.0", "10-40-0.7"])
def test_chroma_stabilizer_adaptive_over_the_cube(ctx, base_tol, max_extra, weight, pair, swap):
    from vsdeoldify_amd import imfilters as F
    _sweep2(f"chroma_stabilizer_adaptive {base_tol} {max_extra} {weight}", lambda a, b: F.chroma_stabilizer_adaptive_np(ctx, a, b, base_tol, max_extra, weight),
            lambda a, b: pipeline.chroma_stabilizer_adaptive(a, b, base_tol, max_extra, weight), pair, swap)


# ---- 6: blend, per channel: every byte pair; 0.1 and 1 / 3 are weights whose float32 value is not the float64 value.  0.6 and 0.8 are the weights at
# which a contracted multiply-add changes bytes (361 and 596 of the 65 536 pairs; none at the other six): a + w (b - a) must cancel (b < a, w > 0.5) for
# the sum to keep more bits than the product, and float32(w) must lie above w for the exact sum to fall just BELOW the integer the rounded product hits
@pytest.mark.gpu
@pytest.mark.parametrize("w", [0.3, 0.4, 0.5, 0.77, 0.1, 1 / 3, 0.6, 0.8])
def test_blend_over_all_byte_pairs(ctx, w):
    from vsdeoldify_amd import imfilters as F
    a, b = su.byte_pairs()
    n = su.assert_same_bytes(F.blend_np(ctx, a, b, w), imaging.pil_blend(a, b, w), (a, b), f"blend {w}")
    n += su.assert_same_bytes(F.blend_np(ctx, b, a, w), imaging.pil_blend(b, a, w), (b, a), f"blend {w} swapped")
    print(f"blend {w}: byte pairs per channel == {n}")
    assert n == 2 * 65536


# ---- 7 / 8: restore_color_gradient: colour image = the cube, gray image = its partner ---------------------------------------------------------------------------
RESTORE = [(dict(sat=0.8, tht=30, alpha=2.0), P1), (dict(sat=1.5, tht=60, weight=0.3, alpha=3.0), P2), (dict(sat=0.6, tht=20, weight=-0.4), P1),
           (dict(tht=45, alpha=1.5), P2),                              # sat == 1: the kernel skips the saturation cast
           (dict(tht=30, return_mask=True), P2)]


@pytest.mark.gpu
@pytest.mark.parametrize("case,pair", RESTORE, ids=_ids([c for c, _ in RESTORE]))
def test_restore_color_gradient_algo0_over_the_cube(ctx, case, pair):
    from vsdeoldify_amd import imfilters as F
    _sweep2(f"restore_color_gradient {case}", lambda a, b: F.restore_color_gradient_np(ctx, a, b, **case),
            lambda a, b: tweaks.restore_color_gradient(a, b, **case), pair)


RESTORE_F = [(dict(tht=40, algo=1), P1), (dict(tht=25, alpha=1.5, algo=2), P2), (dict(tht=40, algo=1, return_mask=True), P2),
             (dict(tht=25, alpha=1.5, algo=2, return_mask=True), P1)]


@pytest.mark.gpu
@pytest.mark.parametrize("case,pair", RESTORE_F, ids=_ids([c for c, _ in RESTORE_F]))
def test_restore_color_gradient_algo12_over_the_cube(ctx, case, pair):
    """algo 1 / 2 build the mask with powf / exp: a mask value sitting on an integer may land on the other side.  The rule of tests/test_tweaks.py:
    |d| <= 1 and fewer than 2e-3 of the bytes differ, here over the whole cube."""
    from vsdeoldify_amd import imfilters as F
    n = nbytes = differ = worst = 0
    for slab in su.cube_slabs():
        gray = su.partner(slab, *pair)
        d = np.abs(F.restore_color_gradient_np(ctx, slab, gray, **case).astype(np.int16) - tweaks.restore_color_gradient(slab, gray, **case))
        worst, differ, nbytes, n = max(worst, int(d.max())), differ + int((d > 0).sum()), nbytes + d.size, n + d.shape[0] * d.shape[1]
    share = differ / nbytes
    print(f"restore_color_gradient {case}: n == {n}, max |d| {worst}, share of bytes that differ {share:.3e} (cap 2e-3)")
    assert n == su.N_CUBE
    assert worst <= 1 and share < 2e-3, (case, worst, share)


# ---- 9: csrc/stabilizer.hip is a second translation unit including pixel_ops.h: the fused launch against the chain of stand-alone launches -----------
DARK, SMOOTH, CMAP = (0.3, 0.8, "280:360,0:30"), (0.3, 0.6, 0.8, -0.10, "red|0.5,0.0"), "blue|+40,0.2"


@pytest.mark.gpu
def test_fused_stabilizer_equals_the_stand_alone_filters_over_the_cube(ctx):
    """GPU against GPU, equal bytes: each stage alone (so that each sees the whole cube) and the three-stage chain"""
    from vsdeoldify_amd import stabilizer as S
    n = 0
    for slab in su.cube_slabs():
        d, s, c = S.dark_tweak_frame(slab, *DARK), S.chroma_bright_tweak_frame(slab, *SMOOTH), S.colormap_frame(slab, CMAP)
        su.assert_same_bytes(S.stabilize_np(ctx, slab, dark=DARK), d, slab, "fused dark stage")
        su.assert_same_bytes(S.stabilize_np(ctx, slab, smooth=SMOOTH), s, slab, "fused smooth stage")
        su.assert_same_bytes(S.stabilize_np(ctx, slab, colormap=CMAP), c, slab, "fused colormap stage")
        chain = S.colormap_frame(S.chroma_bright_tweak_frame(d, *SMOOTH), CMAP)
        n += su.assert_same_bytes(S.stabilize_np(ctx, slab, dark=DARK, smooth=SMOOTH, colormap=CMAP), chain, slab, "fused three-stage chain")
    print(f"fused stabilizer: n == {n}")
    assert n == su.N_CUBE


# ---- 10 - 12: the Lab kernels ---------------------------------------------------------------------------------------------------------------------------------------
_LAB32 = {}


def lab32(k, slab):
    """float32(oracle.zhang.rgb2lab(slab k)) [H, W, 3]; computed once per process"""
    if k not in _LAB32:
        _LAB32[k] = zhang.rgb2lab(slab).astype(np.float32)
    return _LAB32[k]


def lab_norm(k, slab):
    """oracle.colormnet_net.frame_to_lab_tensor(slab k) as float32 planes [3, H, W], in numpy from the cached Lab (the same float32 operations)"""
    lab = lab32(k, slab).transpose(2, 0, 1)
    return (lab - np.array([50.0, 0, 0], np.float32).reshape(3, 1, 1)) / np.array([50.0, 110, 110], np.float32).reshape(3, 1, 1)


@pytest.mark.gpu
def test_rgb_to_lab_over_the_cube(ctx):
    """havc_colormnet_rgb_to_lab as image_to_lab calls it, against oracle.colormnet_net.frame_to_lab_tensor"""
    from vsdeoldify_amd import _native as nat
    n = differ = values = 0
    worst = 0.0
    for slab in su.cube_slabs():
        h, w = slab.shape[:2]
        got = np.empty((3, h, w), np.float32)
        nat.check(ctx.lib.havc_colormnet_rgb_to_lab(ctx.h, nat.as_ptr(slab), nat.as_ptr(got), w, h), ctx.h)
        want = O.frame_to_lab_tensor(slab).numpy()
        worst = max(worst, float(np.abs(got - want).max()))
        differ += int((got.view(np.uint32) != want.view(np.uint32)).sum())
        values += got.size
        n += h * w
    share = differ / values
    print(f"rgb_to_lab: n == {n}, max |d| {worst:.3e} (bound 2e-6), float32 values not bit-identical {differ} of {values} = {share:.3e} (cap 1e-6)")
    assert n == su.N_CUBE
    assert worst < 2e-6 and share <= 1e-6, (worst, differ, share)


def _lab_to_rgb_inputs(which, k, slab):
    planes = lab_norm(k, slab)
    return planes if which == "round_trip" else su.perturb_ab(planes, k)


def _lab_to_rgb_reference(planes):
    """(bytes of the oracle, mask of the bytes left out) for float32 planes [3, H, W]"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(planes))
    want = O.lab_tensor_to_rgb(t[:1], t[1:])
    v = su.lab2rgb_unclipped(su.denormalise_lab(planes))
    return want, su.left_out(v), v


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["round_trip", "perturbed"])
def test_lab_to_rgb_over_the_cube(ctx, which):
    """havc_colormnet_lab_to_rgb against oracle.colormnet_net.lab_tensor_to_rgb on the same float32 planes: (a) the oracle's Lab of the cube, (b) the
    same with +-40 Lab units of seeded noise on a and b.  Equal bytes except where the oracle's unclipped value * 255 is within 1e-9 of an integer."""
    from vsdeoldify_amd import _native as nat
    n = out = nbytes = bad_total = 0
    first = []
    for k, slab in enumerate(su.cube_slabs()):
        planes = np.ascontiguousarray(_lab_to_rgb_inputs(which, k, slab))
        want, skip, v = _lab_to_rgb_reference(planes)
        out, nbytes = out + int(skip.sum()), nbytes + skip.size
        h, w = slab.shape[:2]
        got = np.empty((h, w, 3), np.uint8)
        nat.check(ctx.lib.havc_colormnet_lab_to_rgb(ctx.h, nat.as_ptr(planes[:1]), nat.as_ptr(planes[1:]), nat.as_ptr(got), w, h), ctx.h)
        bad = (got != want) & ~skip
        bad_total += int(bad.sum())
        for y, x, c in np.argwhere(bad)[:max(0, 10 - len(first))]:
            first.append((slab[y, x].tolist(), planes[:, y, x].tolist(), int(c), int(got[y, x, c]), int(want[y, x, c]), float(v[y, x, c] * 255.0)))
        n += h * w
    share = out / nbytes
    print(f"lab_to_rgb {which}: n == {n}, bytes left out {out} of {nbytes} = {share:.3e} (cap {su.LEFT_OUT_CAP:.0e}), wrong bytes {bad_total}")
    assert n == su.N_CUBE and share <= su.LEFT_OUT_CAP, (n, share)
    assert bad_total == 0, f"lab_to_rgb {which}: {bad_total} bytes differ; first (rgb of the cube, planes, channel, got, want, oracle value * 255): {first}"


def _prep_lab_l(ctx, frames, precise):
    """OP_PREP_LAB_L through a one-op plan: uint8 [n, S, S, 3] -> the raw fp16 buffer [n, S, S, pitch]"""
    from tests import gpu_util as gu
    from vsdeoldify_amd.plan import PlanBuilder, WeightPack
    n, S = frames.shape[:2]
    b = PlanBuilder(precise=precise)
    inb = b.buf(S * S * 3, 1)
    y = b.tensor(S, S, 8, zero_init=False)
    b.prep_lab_l("prep_lab_l", inb, S, y)
    return gu.run_plan(ctx, WeightPack(), b, {inb: frames}, {y.buf: ((n, S, S, y.cpitch), np.float16)}, n)[y.buf]


def _prep_lab_l_expected(L32):
    """the kernel's own float32 and fp16 steps on float32(L of the oracle): v = (L - 50) / 100, hi = fp16(v), lo = fp16((v - hi) * 2048)"""
    v = (L32 - np.float32(50.0)) / np.float32(100.0)
    hi = v.astype(np.float16)
    lo = ((v - hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    return v, hi, lo


@pytest.mark.gpu
@pytest.mark.parametrize("precise", [False, True], ids=["fast", "precise"])
def test_prep_lab_l_over_the_cube(ctx, precise):
    """fast mode writes fp16(v), precise mode the hi / lo pair; a pixel that is not bit-equal must be within one fp16 ulp (hi, and hi + lo / 2048
    against v).  The 256 grays go through the table g_gray_L: all of them bit-equal, checked apart."""
    gray = np.repeat(np.arange(256, dtype=np.uint8), 3).reshape(1, 16, 16, 3)
    raw = _prep_lab_l(ctx, gray, precise)
    _, hi, lo = _prep_lab_l_expected(zhang.rgb2lab(gray)[..., 0].astype(np.float32))
    P = raw.shape[-1] // 2 if precise else raw.shape[-1]
    assert np.array_equal(raw[..., 0].view(np.uint16), hi.view(np.uint16)), "gray table: hi"
    assert not precise or np.array_equal(raw[..., P].view(np.uint16), lo.view(np.uint16)), "gray table: lo"
    n = differ = 0
    for k, slab in enumerate(su.cube_slabs()):
        frames = slab.reshape(-1, 512, 512, 3)                     # per-pixel kernel: any cut of the slab into square frames holds the same pixels
        raw = _prep_lab_l(ctx, frames, precise)
        v, hi, lo = _prep_lab_l_expected(lab32(k, slab)[..., 0].reshape(frames.shape[:3]))
        assert not raw[..., 1:P].any() and not raw[..., P + 1:].any(), "channels 1 - 7 are zero"
        ne = raw[..., 0].view(np.uint16) != hi.view(np.uint16)
        got = raw[..., 0].astype(np.float32)
        if precise:
            ne |= raw[..., P].view(np.uint16) != lo.view(np.uint16)
            got_v = got + raw[..., P].astype(np.float32) / np.float32(2048.0)
        ulp = np.spacing(np.abs(hi)).astype(np.float32)
        assert (np.abs(got - hi.astype(np.float32)) <= ulp).all(), "hi further than one fp16 ulp from the oracle"
        assert not precise or (np.abs(got_v - v) <= ulp).all(), "hi + lo / 2048 further than one fp16 ulp from the oracle"
        differ += int(ne.sum())
        n += ne.size
    share = differ / n
    print(f"prep_lab_l {'precise' if precise else 'fast'}: n == {n}, pixels not bit-equal {differ} = {share:.3e} (cap 1e-6); 256 grays bit-equal")
    assert n == su.N_CUBE and share <= 1e-6, (n, differ, share)


def _prep_ddcolor(ctx, frames, precise):
    """OP_PREP_DDCOLOR through a one-op plan: uint8 [n, S, S, 3] -> the raw fp16 buffer [n, S, S, pitch]"""
    from tests import gpu_util as gu
    from vsdeoldify_amd.plan import PlanBuilder, WeightPack
    n, S = frames.shape[:2]
    b = PlanBuilder(precise=precise)
    inb = b.buf(S * S * 3, 1)
    y = b.tensor(S, S, 3, zero_init=False)
    b.prep_ddcolor("prep_ddcolor", inb, S, y)
    return gu.run_plan(ctx, WeightPack(), b, {inb: frames}, {y.buf: ((n, S, S, y.cpitch), np.float16)}, n)[y.buf]


def _prep_ddcolor_expected(rgb_u8):
    """oracle.ddcolor.colorize_frame's network input: float32(lab2rgb(L, 0, 0)), (x - MEAN) / STD in float32; then the kernel's own fp16 steps"""
    from oracle import ddcolor
    L = zhang.rgb2lab(rgb_u8)[..., :1]
    gray = zhang.lab2rgb(np.concatenate([L, np.zeros_like(L), np.zeros_like(L)], -1)).astype(np.float32)
    v = (gray - ddcolor.MEAN.numpy().reshape(3)) / ddcolor.STD.numpy().reshape(3)
    assert v.dtype == np.float32
    hi = v.astype(np.float16)
    lo = ((v - hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    return v, hi, lo


@pytest.mark.gpu
def test_prep_ddcolor_over_the_cube(ctx):
    """both modes in one pass over the oracle; the rule of OP_PREP_LAB_L on the three channels: bit-equal on all but 1e-6 of the pixels, those within
    one fp16 ulp; the 256 grays (table g_gray_dd) all bit-equal"""
    gray = np.repeat(np.arange(256, dtype=np.uint8), 3).reshape(1, 16, 16, 3)
    _, ghi, glo = _prep_ddcolor_expected(gray)
    for precise in (False, True):
        raw = _prep_ddcolor(ctx, gray, precise)
        P = raw.shape[-1] // 2 if precise else raw.shape[-1]
        assert np.array_equal(raw[..., :3].view(np.uint16), ghi.view(np.uint16)), f"gray table: hi (precise {precise})"
        assert not precise or np.array_equal(raw[..., P:P + 3].view(np.uint16), glo.view(np.uint16)), "gray table: lo"
    n, differ = 0, {False: 0, True: 0}
    for slab in su.cube_slabs():
        frames = slab.reshape(-1, 512, 512, 3)
        v, hi, lo = _prep_ddcolor_expected(frames)
        ulp = np.spacing(np.abs(hi)).astype(np.float32)
        for precise in (False, True):
            raw = _prep_ddcolor(ctx, frames, precise)
            P = raw.shape[-1] // 2 if precise else raw.shape[-1]
            assert not raw[..., 3:P].any() and not raw[..., P + 3:].any(), "channels 3 - 7 are zero"
            ne = (raw[..., :3].view(np.uint16) != hi.view(np.uint16)).any(-1)
            got = raw[..., :3].astype(np.float32)
            assert (np.abs(got - hi.astype(np.float32)) <= ulp).all(), "hi further than one fp16 ulp from the oracle"
            if precise:
                ne |= (raw[..., P:P + 3].view(np.uint16) != lo.view(np.uint16)).any(-1)
                assert (np.abs(got + raw[..., P:P + 3].astype(np.float32) / np.float32(2048.0) - v) <= ulp).all(), "hi + lo / 2048 further than one fp16 ulp"
            differ[precise] += int(ne.sum())
        n += frames.shape[0] * 512 * 512
    print(f"prep_ddcolor: n == {n}, pixels not bit-equal fast {differ[False]} = {differ[False] / n:.3e}, precise {differ[True]} = {differ[True] / n:.3e} (cap 1e-6); 256 grays bit-equal")
    assert n == su.N_CUBE and max(differ.values()) / n <= 1e-6, (n, differ)


# ---- CPU: the helper itself ----------------------------------------------------------------------------------------------------------------------------------------
def test_slabs_cover_each_triple_once():
    for n_slabs in (8, 4):
        seen = np.zeros(su.N_CUBE, np.int64)
        for slab in su.cube_slabs(n_slabs):
            assert slab.shape == (512 * (8 // n_slabs), 4096, 3) and slab.dtype == np.uint8
            seen += np.bincount(su.indices(slab).reshape(-1), minlength=su.N_CUBE)
        assert (seen == 1).all()


def test_partner_is_a_bijection_far_from_the_diagonal():
    for K, c in su.PARTNERS:
        seen = np.zeros(su.N_CUBE, bool)
        same = 0
        for slab in su.cube_slabs():
            p = su.partner(slab, K, c)
            assert p.shape == slab.shape and p.dtype == np.uint8
            idx = su.indices(p).reshape(-1)
            assert not seen[idx].any() and len(np.unique(idx)) == len(idx)
            seen[idx] = True
            same += int((p == slab).all(-1).sum())
        assert seen.all() and same <= 4, (K, c, same)
    assert su.PARTNERS[0] != su.PARTNERS[1]


def test_byte_pairs_hold_every_pair_in_every_channel():
    a, b = su.byte_pairs()
    assert a.shape == b.shape == (256, 256, 3)
    for ch in range(3):
        assert len(np.unique(a[..., ch].astype(np.int32) * 256 + b[..., ch])) == 65536


def test_failure_message_names_the_pixels():
    a, _ = su.byte_pairs()
    bad = a.copy()
    bad[3, 5, 1] ^= 1
    with pytest.raises(AssertionError, match=r"1 of 65536 pixels differ.*\(\(\[3, 3, 3\],\), \[3, 2, 3\], \[3, 3, 3\]\)"):
        su.assert_same_bytes(bad, a, a, "x")
    assert su.assert_same_bytes(a, a, a, "x") == 65536


def test_lab_restatement_and_left_out_share_over_the_cube():
    """On both inputs of the Lab -> rgb sweep, over the whole cube: lab2rgb_unclipped clipped to [0, 1] IS oracle.zhang.lab2rgb, its bytes are those
    of oracle.colormnet_net.lab_tensor_to_rgb, and the share of bytes the comparison leaves out is at most 5e-4 (measured on a quarter of the cube:
    1.0e-4 on the round trip, whose values sit near integers by construction, spread by the float32 rounding of Lab; 0 on the perturbed input)."""
    out = {"round_trip": 0, "perturbed": 0}
    nbytes = 0
    for k, slab in enumerate(su.cube_slabs()):
        if k == 0:
            assert np.array_equal(lab_norm(k, slab), O.frame_to_lab_tensor(slab).numpy())          # the cached planes are the oracle's
        for which in out:
            planes = _lab_to_rgb_inputs(which, k, slab)
            v = su.lab2rgb_unclipped(su.denormalise_lab(planes))
            assert np.array_equal(np.clip(v, 0, 1), zhang.lab2rgb(su.denormalise_lab(planes))), which
            if k in (0, 7):
                want, _, _ = _lab_to_rgb_reference(planes)
                assert np.array_equal((np.clip(v, 0, 1) * 255).astype(np.uint8), want), which
            out[which] += int(su.left_out(v).sum())
        nbytes += slab.size
    for which, cnt in out.items():
        print(f"lab_to_rgb {which}: bytes left out {cnt} of {nbytes} = {cnt / nbytes:.3e} (cap {su.LEFT_OUT_CAP:.0e})")
        assert cnt / nbytes <= su.LEFT_OUT_CAP, (which, cnt)
    assert nbytes == 3 * su.N_CUBE
