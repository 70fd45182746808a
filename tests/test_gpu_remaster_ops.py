"""GPU: the five kernels of csrc/remaster.hip one op at a time against oracle/remaster.py (plain float64), each through a one-op plan whose buffers are
uploaded directly (tests/remaster_util.py: the cases, the inputs, the attention bound and the ulp rules; tests/test_remaster_ops_host.py shows on the CPU
that those rules can fail).  tests/test_gpu_remaster.py keeps the end-to-end check of the whole network; this file holds what that one is too loose
to see: one fragment, one lane group, one tail key, one byte.

HAVC_REMASTER_OPS_OUT=<file> writes every measured figure and the time of every item (profiles/remaster_ops.txt)."""
import os
import time

import numpy as np
import pytest

from oracle import remaster as O
from tests import remaster_util as U
from tests import sweep_util as su

pytestmark = pytest.mark.gpu
REPORT, TIMES, RATIOS = [], [], []
SENT = U.bits(np.array([U.SENTINEL]))[0]


def note(line):
    REPORT.append(line)
    print(line)


@pytest.fixture(scope="module", autouse=True)
def _profile():
    yield
    out = os.environ.get("HAVC_REMASTER_OPS_OUT")
    if out and REPORT:
        with open(out, "w") as f:
            f.write("The DeepRemaster kernels (csrc/remaster.hip) op by op against float64 (tests/test_gpu_remaster_ops.py, oracle/remaster.py).\n"
                    "attention: max over the output of |GPU - ref| / bound, bound = 2^-11 (|gamma| A + |ref|); the limit is 2.0 and a figure above 1.0 asks for an\n"
                    f"explanation.  Largest figure of this run: {max(RATIOS, default=0.0):.3f}" + (" (none above 1.0)" if max(RATIOS, default=0.0) <= 1.0 else " (ABOVE 1.0)") + ".\n"
                    "elu / prep: |GPU - exact| in fp16 ulp at the exact value, limit 0.5 + 2^-10.  sigmoid tap: fp32 ulp, limit 4.\n\n")
            f.write("\n".join(REPORT) + "\n\nseconds per item (host wall clock, reference included)\n" + "\n".join(TIMES) + "\n")


@pytest.fixture(autouse=True)
def _timed(request):
    t0 = time.perf_counter()
    yield
    TIMES.append(f"{time.perf_counter() - t0:7.3f}  {request.node.name}")


# ---- source-reference attention ----------------------------------------------------------------------------------------------------------------------
_CACHE = {}


def attn_case(name, regime, gamma):
    """(case, inputs, (ref, A)) computed once per module and never written to"""
    case = U.CASES[name]
    if (name, regime) not in _CACHE:
        x, q, k, v = U.attn_inputs(case, regime)
        U.check_regime(case, regime, q, k)
        for a in (x, q, k, v):
            a.setflags(write=False)
        _CACHE[name, regime] = (x, q, k, v)
    if (name, regime, gamma) not in _CACHE:
        ref, A = U.attn_reference(case, *_CACHE[name, regime], gamma)
        ref.setflags(write=False)
        A.setflags(write=False)
        _CACHE[name, regime, gamma] = (ref, A)
    return case, _CACHE[name, regime], _CACHE[name, regime, gamma]


def held(case, regime, gamma, inp, ref_A, got, label, bad):
    ratio, worst = U.attn_ratio(got.astype(np.float64), ref_A[0], ref_A[1], gamma)
    RATIOS.append(ratio)
    note(f"attention {case.name:10s} {regime:8s} gamma {gamma:+.1f} {label:15s} max err / bound {ratio:.3f}")
    if not (ratio <= U.LIMIT and np.isfinite(got.astype(np.float32)).all()):
        bad.append(f"{case.name} {regime} gamma {gamma} {label}: " + U.attn_worst_text(case, inp[1], inp[2], worst, ratio))
    return ratio


@pytest.mark.parametrize("name", list(U.CASES))
def test_attention_is_within_the_bound_of_the_float64_reference(ctx, name):
    bad = []
    for regime in U.CASES[name].regimes:
        for gamma in U.GAMMAS:
            case, inp, ref_A = attn_case(name, regime, gamma)
            x, q, k, v = inp
            got, full = U.run_attention(ctx, case, x, q, k, U.value_rows(case, v), gamma)
            held(case, regime, gamma, inp, ref_A, got, "", bad)
            assert (U.bits(full[case.frames:]) == SENT).all(), "frames past the batch were written"
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", list(U.CASES))
def test_attention_with_gamma_zero_returns_x_bit_for_bit(ctx, name):
    case, (x, q, k, v), _ = attn_case(name, "flat", 0.0)
    got, _ = U.run_attention(ctx, case, x, q, k, U.value_rows(case, v), 0.0)
    assert np.array_equal(U.bits(got), U.bits(x[:case.frames]))


@pytest.mark.parametrize("name", ["cross", "three"])
def test_attention_reads_and_writes_channel_views(ctx, name):
    """q at offset 64 of a 128-wide buffer, x at offset 512 of a 1024-pitch buffer, y at offset 0 of a 1024-pitch buffer whose other half is a sentinel"""
    bad = []
    case, inp, ref_A = attn_case(name, "flat", 0.7)
    x, q, k, v = inp
    got, full = U.run_attention(ctx, case, x, q, k, U.value_rows(case, v), 0.7, views=True)
    held(case, "flat", 0.7, inp, ref_A, got, "views", bad)
    assert full.shape[-1] == 1024 and (U.bits(full[..., 512:]) == SENT).all(), "the other half of the destination buffer was written"
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", ["small", "edge65", "three", "three_wide"])
def test_attention_never_weighs_the_value_padding(ctx, name):
    """columns nk .. npitch of every V^T row set to +-60000: bit-identical to the zero-padded run, so P is exactly 0 for every masked key.
    (NaN or inf there is outside the contract: 0 x NaN is NaN in any MFMA.)"""
    case = U.CASES[name]
    for regime in case.regimes:
        _, (x, q, k, v), _ = attn_case(name, regime, 0.7)
        r = np.random.default_rng(11)
        pad = np.where(r.integers(0, 2, (len(v), U.DV, case.npitch - case.nk)) == 1, 60000.0, -60000.0).astype(np.float16)
        zero, _ = U.run_attention(ctx, case, x, q, k, U.value_rows(case, v), 0.7)
        big, _ = U.run_attention(ctx, case, x, q, k, U.value_rows(case, v, pad), 0.7)
        same = U.bits(zero) == U.bits(big)
        assert same.all(), f"{name} {regime}: {int((~same).sum())} of {same.size} outputs change with the padding; first at {np.argwhere(~same)[:5].tolist()}"


def test_attention_does_not_depend_on_the_slot_order_of_the_stills(ctx):
    bad = []
    for regime in U.CASES["cross"].regimes:
        case, inp, ref_A = attn_case("cross", regime, 0.7)
        x, q, k, v = inp
        got, _ = U.run_attention(ctx, case, x, q, k, U.value_rows(case, v), 0.7, still_order=(3, 0, 4, 1, 2))
        held(case, regime, 0.7, inp, ref_A, got, "slots 3,0,4,1,2", bad)
    assert not bad, "\n".join(bad)


# ---- one-op plans for the element-wise kernels --------------------------------------------------------------------------------------------------------
def run_elu(ctx, src, coff, C, H, W, dst=None, dcoff=0):
    """src [1][H W][pitch] fp16; dst None = in place.  Returns the destination buffer [1][H W][pitch]."""
    from vsdeoldify_amd.plan import PlanBuilder, View, WeightPack
    from tests.gpu_util import run_plan
    b = PlanBuilder()
    xv = View(b.buf(H * W * src.shape[-1]), coff, src.shape[-1], H, W, C, C)
    ups = {xv.buf: src}
    yv = None
    if dst is not None:
        yv = View(b.buf(H * W * dst.shape[-1]), dcoff, dst.shape[-1], H, W, C, C)
        ups[yv.buf] = dst
    b.elu("elu", xv, yv)
    o = yv or xv
    return run_plan(ctx, WeightPack(), b, ups, {o.buf: ((1, H * W, o.cpitch), np.float16)}, 1)[o.buf]


def check_elu(got, h, label):
    """got, h: fp16 arrays of equal shape (h = the inputs).  Returns the largest error over the finite negative inputs, in fp16 ulp."""
    got, h = got.reshape(-1), h.reshape(-1)
    gb, hb = U.bits(got), U.bits(h)
    nan = np.isnan(h)
    pos = ~nan & ~np.signbit(h)                                      # +0, positives, +inf: the value itself, bit for bit
    assert np.array_equal(gb[pos], hb[pos]), f"{label}: {int((gb[pos] != hb[pos]).sum())} non-negative inputs changed"
    assert np.isnan(got[nan]).all() and nan.sum() == 2046
    assert (gb[hb == 0x8000] == 0x8000).all(), f"{label}: -0 -> {got[hb == 0x8000]}"
    assert (gb[hb == 0xFC00] == 0xBC00).all(), f"{label}: -inf -> {got[hb == 0xFC00]}"
    neg = np.isfinite(h) & np.signbit(h) & (hb != 0x8000)
    e = U.ulp16_error(got[neg], O.elu(h[neg].astype(np.float64)))
    worst = int(np.argmax(e))
    note(f"elu {label:9s} {int(neg.sum())} finite negative inputs: max |err| {e.max():.6f} fp16 ulp at x = {float(h[neg][worst])!r}: excess over 0.5 = {e.max() - 0.5:+.2e} (limit 2^-10 = {2.0 ** -10:.2e})")
    assert e.max() <= U.HALF_ULP_LIMIT, (label, float(e.max()), float(h[neg][worst]), float(got[neg][worst]))


def test_elu_on_every_fp16_bit_pattern_in_place(ctx):
    h = U.all_halves()
    got = run_elu(ctx, h.reshape(1, 8192, 8), 0, 8, 64, 128)
    check_elu(got, h, "in place")


def test_elu_between_channel_views(ctx):
    """a 16-channel view at offset 8 of a 32-pitch buffer -> offset 512 of a 1024-pitch buffer; everything outside the destination view keeps its sentinel"""
    h = U.all_halves().reshape(1, 4096, 16)
    src = np.full((1, 4096, 32), 1.5, np.float16)
    src[..., 8:24] = h
    dst = np.full((1, 4096, 1024), U.SENTINEL, np.float16)
    got = run_elu(ctx, src, 8, 16, 64, 64, dst, 512)
    check_elu(got[..., 512:528], h, "views")
    outside = np.delete(U.bits(got), np.s_[512:528], axis=-1)
    assert (outside == SENT).all(), f"{int((outside != SENT).sum())} elements outside the destination view were written"


def run_tstack(ctx, src, coff, C, T, y_pitch, y_coff, H=5, W=7):
    """src [max_batch][H W][pitch] fp16 (all frames uploaded), batch T -> the whole destination buffer [max_batch][H W][y_pitch], sentinel-filled before"""
    from vsdeoldify_amd.plan import PlanBuilder, View, WeightPack
    from tests.gpu_util import run_plan
    b = PlanBuilder()
    xv = View(b.buf(H * W * src.shape[-1]), coff, src.shape[-1], H, W, C, C)
    yv = View(b.buf(H * W * y_pitch), y_coff, y_pitch, H, W, 3 * C, 3 * C)
    b.tstack("tstack", xv, yv)
    dst = np.full((len(src), H * W, y_pitch), U.SENTINEL, np.float16)
    return run_plan(ctx, WeightPack(), b, {xv.buf: src, yv.buf: dst}, {yv.buf: (dst.shape, np.float16)}, T, max_batch=len(src))[yv.buf]


def tstack_source(frames, pitch, seed):
    """fp16 with random positive finite bit patterns (never 0, never the sentinel): a copy is bit-exact or wrong"""
    r = np.random.default_rng(seed)
    return r.integers(1, 0x7C00, (frames, 35, pitch)).astype(np.uint16).view(np.float16)


def check_tstack(got, src, coff, C, T, y_coff):
    want = np.full(got.shape, SENT, np.uint16)
    want[:T, :, y_coff:y_coff + 3 * C] = U.bits(O.tstack(src[:T, :, coff:coff + C]))
    same = U.bits(got) == want
    assert same.all(), f"{int((~same).sum())} of {same.size} elements differ; first (frame, pixel, channel): {np.argwhere(~same)[:5].tolist()}"
    if T >= 1:
        assert not U.bits(got)[0, :, y_coff:y_coff + C].any() and not U.bits(got)[T - 1, :, y_coff + 2 * C:y_coff + 3 * C].any()


@pytest.mark.parametrize("T", [1, 2, 3, 5])
@pytest.mark.parametrize("C", [8, 24])
def test_tstack_is_bit_exact_and_stays_inside_its_view(ctx, T, C):
    src = tstack_source(T, C, [T, C])
    got = run_tstack(ctx, src, 0, C, T, 3 * C + 16, 8)
    check_tstack(got, src, 0, C, T, 8)


def test_tstack_of_1024_channels_from_a_view_at_an_offset(ctx):
    src = tstack_source(3, 1024 + 128, 5)
    got = run_tstack(ctx, src, 64, 1024, 3, 3072 + 64, 64)
    check_tstack(got, src, 64, 1024, 3, 64)


def test_tstack_of_a_short_batch_does_not_look_past_it(ctx):
    """batch 2 on a net of five frames whose source frames 2-4 are non-zero: frame 1's t+1 block is zero, destination frames 2-4 are untouched"""
    src = tstack_source(5, 8, 9)
    got = run_tstack(ctx, src, 0, 8, 2, 40, 8)
    check_tstack(got, src, 0, 8, 2, 8)
    assert not U.bits(got)[1, :, 8 + 16:8 + 24].any()


def test_tstack_and_3x3_conv_equal_a_direct_3d_convolution(ctx):
    """T = 3, Ci = 16, Co = 24, 8 x 8, bias only, fp16-exact inputs and weights against float64.
    limit = 2 (2^-11 |ref| + n 2^-24 sum |w x|), n = 27 Ci: the fp16 store plus the standard bound of an fp32 sum of n terms, times 2"""
    from tests.gpu_util import run_plan
    from vsdeoldify_amd.plan import PlanBuilder, View, WeightPack, pack_conv, pitch_for
    from vsdeoldify_amd.remaster_net import repack_temporal
    T, Ci, Co, H, W = 3, 16, 24, 8, 8
    r = np.random.default_rng(21)
    x = U.f16(r.standard_normal((Ci, T, H, W)))
    w = U.f16(0.1 * r.standard_normal((Co, Ci, 3, 3, 3)))
    bias = r.standard_normal(Co).astype(np.float32)
    ref, mag = O.conv3d_same(x, w, bias)
    pack, b = WeightPack(), PlanBuilder()
    xv = b.tensor(H, W, Ci)
    pitch = pitch_for(3 * Ci)
    xs = View(b.buf(H * W * pitch), 0, pitch, H, W, 3 * Ci, 3 * Ci)
    b.tstack("tstack", xv, xs)
    pc = pack_conv(pack, repack_temporal(w.astype(np.float32)), np.concatenate([kt * Ci + np.arange(Ci) for kt in range(3)]), xs.span, bias=bias)
    yv = b.tensor(H, W, Co)
    b.conv("conv", pc, xs, yv, pad=1)
    got = run_plan(ctx, pack, b, {xv.buf: np.ascontiguousarray(x.transpose(1, 2, 3, 0))}, {yv.buf: ((T, H, W, yv.cpitch), np.float16)}, T)[yv.buf]
    got = got[..., :Co].astype(np.float64).transpose(3, 0, 1, 2)
    n = 27 * Ci
    bound = 2.0 ** -11 * np.abs(ref) + n * 2.0 ** -24 * mag
    ratio = np.abs(got - ref) / bound
    note(f"tstack + 3x3 conv against a float64 3-D convolution: max err / bound {ratio.max():.3f} (limit 2), n = {n}")
    assert ratio.max() <= 2.0, (float(ratio.max()), np.unravel_index(int(ratio.argmax()), ratio.shape))


# ---- prep -------------------------------------------------------------------------------------------------------------------------------------------------
def run_prep(ctx, rgb, refs, pitch, coff):
    """rgb u8 [B][Hi][Wi][3] -> the whole destination buffer [B][Ho][Wo][pitch] fp16, sentinel-filled before"""
    from tests.gpu_util import run_plan
    from vsdeoldify_amd.plan import PlanBuilder, View, WeightPack
    B, Hi, Wi = rgb.shape[:3]
    Ho, Wo = (Hi, Wi) if refs else (Hi + 2, Wi + 2)
    b = PlanBuilder()
    src = b.buf(Hi * Wi * 3, 1)
    yv = View(b.buf(Ho * Wo * pitch), coff, pitch, Ho, Wo, 3 if refs else 1, 8)
    b.prep_remaster("prep", src, Hi, Wi, yv, refs=refs)
    dst = np.full((B, Ho, Wo, pitch), U.SENTINEL, np.float16)
    return run_plan(ctx, WeightPack(), b, {src: rgb, yv.buf: dst}, {yv.buf: (dst.shape, np.float16)}, B)[yv.buf]


def prep_images(Hi, Wi):
    r = np.random.default_rng([Hi, Wi])
    rgb = r.integers(0, 256, (2, Hi, Wi, 3), dtype=np.uint8)
    if Hi * Wi >= 256:                                                # the second frame holds every grey level
        flat = rgb[1].reshape(-1, 3)
        flat[:256] = np.arange(256, dtype=np.uint8)[:, None]
    return rgb


@pytest.mark.parametrize("Hi,Wi,pitch,coff", [(1, 1, 8, 0), (3, 5, 8, 0), (3, 5, 24, 8), (16, 17, 8, 0)])
def test_prep_frames_gray_border_and_zero_channels(ctx, Hi, Wi, pitch, coff):
    rgb = prep_images(Hi, Wi)
    got = run_prep(ctx, rgb, False, pitch, coff)
    want = O.prep_frames(rgb)
    assert want.shape == got.shape[:3]
    e = U.ulp16_error(got[..., coff], want)
    note(f"prep frames {Hi}x{Wi} pitch {pitch} offset {coff}: max |err| {e.max():.6f} fp16 ulp (limit {U.HALF_ULP_LIMIT:.6f})")
    assert e.max() <= U.HALF_ULP_LIMIT, (float(e.max()), np.unravel_index(int(e.argmax()), e.shape))
    g = U.bits(got[..., coff])
    inner = g[:, 1:-1, 1:-1]
    assert np.array_equal(g[:, 0, 1:-1], inner[:, 0]) and np.array_equal(g[:, -1, 1:-1], inner[:, -1])                  # top / bottom edges, every frame
    assert np.array_equal(g[:, 1:-1, 0], inner[:, :, 0]) and np.array_equal(g[:, 1:-1, -1], inner[:, :, -1])            # left / right edges
    assert np.array_equal(g[:, [0, 0, -1, -1], [0, -1, 0, -1]], inner[:, [0, 0, -1, -1], [0, -1, 0, -1]])               # the four corners
    assert not U.bits(got[..., coff + 1:coff + 8]).any(), "channels 1-7 are not +0"
    outside = np.delete(U.bits(got), np.s_[coff:coff + 8], axis=-1)
    assert (outside == SENT).all()


@pytest.mark.parametrize("Hi,Wi,pitch,coff", [(1, 1, 8, 0), (3, 5, 24, 16), (16, 17, 8, 0)])
def test_prep_refs_three_channels_no_border(ctx, Hi, Wi, pitch, coff):
    rgb = prep_images(Hi, Wi)
    got = run_prep(ctx, rgb, True, pitch, coff)
    want = O.prep_refs(rgb)
    assert got.shape[:3] == rgb.shape[:3]
    e = U.ulp16_error(got[..., coff:coff + 3], want)
    note(f"prep refs   {Hi}x{Wi} pitch {pitch} offset {coff}: max |err| {e.max():.6f} fp16 ulp (limit {U.HALF_ULP_LIMIT:.6f})")
    assert e.max() <= U.HALF_ULP_LIMIT, (float(e.max()), np.unravel_index(int(e.argmax()), e.shape))
    assert not U.bits(got[..., coff + 3:coff + 8]).any(), "channels 3-7 are not +0"
    outside = np.delete(U.bits(got), np.s_[coff:coff + 8], axis=-1)
    assert (outside == SENT).all()


# ---- sigmoid + Lab -> RGB ---------------------------------------------------------------------------------------------------------------------------------
def run_out(ctx, ab, rgb, tap):
    """ab fp16 [B][P][8] (logits in channels 0, 1), rgb u8 [B][P][3] -> (bytes [B][P][3], tap float32 [B][P][2] or None)"""
    from tests.gpu_util import run_plan
    from vsdeoldify_amd.plan import PlanBuilder, View, WeightPack
    B, P = ab.shape[:2]
    b = PlanBuilder()
    xv = View(b.buf(P * 8), 0, 8, 256, P // 256, 2, 8)
    src, dst = b.buf(P * 3, 1), b.buf(P * 3, 1)
    tb = b.buf(P * 2, 4) if tap else -1
    b.remaster_out("out", xv, src, dst, tb)
    downs = {dst: ((B, P, 3), np.uint8)}
    if tap:
        downs[tb] = ((B, P, 2), np.float32)
    got = run_plan(ctx, WeightPack(), b, {xv.buf: ab, src: rgb}, downs, B)
    return got[dst], got.get(tb)


def test_output_kernel_sigmoid_tap_and_every_byte(ctx):
    """frame 0: 256 grey levels x 52 x 52 logits; frame 1: random RGB and random logits.  (1) the float32 sigmoid tap against float64, <= 4 fp32 ulp
    (expf, the add and the divide: about one each); (2) the bytes against the float32 Lab steps fed the tap's own values + float64 Lab -> RGB,
    truncated: equal except where the unclipped value x 255 is within 1e-9 of an integer."""
    rgb0, ab0 = U.out_grid()
    P = 256 * 2704
    r = np.random.default_rng(31)
    rgb = np.stack([rgb0.reshape(P, 3), r.integers(0, 256, (P, 3), dtype=np.uint8)])
    ab = np.full((2, P, 8), 5.0, np.float16)
    ab[0, :, :2] = ab0.reshape(P, 2)
    ab[1, :, :2] = U.f16(2.5 * r.standard_normal((P, 2)))
    out, tap = run_out(ctx, ab, rgb, True)
    # (1)
    logits = ab[..., :2].astype(np.float64)
    exact = O.sigmoid(logits)
    assert np.isfinite(tap).all()
    assert (tap[logits == -65504.0] == 0.0).all() and (tap[logits == 65504.0] == 1.0).all() and (logits == 65504.0).sum() == 2 * 256 * 52
    e = U.ulp32_error(tap, exact)
    e = np.where(exact == 0.0, np.where(tap == 0.0, 0.0, np.inf), e)
    worst = np.unravel_index(int(e.argmax()), e.shape)
    note(f"sigmoid tap: max |err| {e.max():.3f} fp32 ulp at logit {float(logits[worst])!r} (limit 4), {e.size} values")
    assert e.max() <= 4.0, (float(e.max()), float(logits[worst]), float(tap[worst]))
    # (2)
    lab = O.lab_from_sigmoid(O.gray_u8(rgb), tap[..., 0], tap[..., 1])
    want, v = U.out_bytes(lab)
    skip = su.left_out(v)
    share = float(skip.mean())
    clipped, fz = float(((v <= 0) | (v >= 1)).mean()), float(((lab[..., 0].astype(np.float64) + 16) / 116 - lab[..., 2].astype(np.float64) / 200 < 0).mean())
    note(f"output bytes: {skip.size} bytes, left out {int(skip.sum())} = {share:.3e} (cap {su.LEFT_OUT_CAP:.0e}); clipped {clipped:.3f}, pixels with fz < 0 {fz:.3f}")
    assert share <= su.LEFT_OUT_CAP
    for f, label in ((0, "grey x logit grid"), (1, "random frame")):
        n = su.assert_same_bytes(np.where(skip[f], want[f], out[f]).reshape(256, 2704, 3), want[f].reshape(256, 2704, 3), rgb[f].reshape(256, 2704, 3), label)
        assert n == P
    note(f"output bytes: 0 of {skip.size - int(skip.sum())} compared bytes differ")
    plain, none = run_out(ctx, ab, rgb, False)
    assert none is None and np.array_equal(plain, out), "the bytes depend on the tap buffer"
