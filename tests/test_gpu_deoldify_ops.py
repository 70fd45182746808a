"""GPU: the fast-mode non-conv kernels of the DeOldify generator one op at a time against plain float64 -- csrc/attention.hip (both kernels, D = 32 / 64 /
96) and the DeOldify half of csrc/elementwise.hip (max-pool, blur + nearest resize, affine / copy, prep_rgb8 in both forms), plus the transposed conv
store that feeds the attention -- each through a one-op plan whose buffers are uploaded directly (tests/deoldify_ops_util.py: the cases, the inputs, the
oracles and the rules; tests/test_deoldify_ops_host.py shows on the CPU that those rules can fail).  Also here: what the runtime's dispatch owes these
ops (csrc/rt_net.cpp): the fast attention op refuses what its kernels cannot run, and a batch on views that do not fill their buffers' frames runs frame
by frame.  tests/test_gpu_kernels.py keeps the composite checks; this file holds what those are too loose to see: one fragment, one lane group, one
tail key, one byte.

HAVC_DEOLDIFY_OPS_OUT=<file> writes every measured figure and the time of every item (profiles/deoldify_ops.txt)."""
import os
import time

import numpy as np
import pytest

from tests import deoldify_ops_util as U

pytestmark = pytest.mark.gpu
REPORT, TIMES, RATIOS = [], [], []
SENT = U.SENT


def note(line):
    REPORT.append(line)
    print(line)


@pytest.fixture(scope="module", autouse=True)
def _profile():
    yield
    out = os.environ.get("HAVC_DEOLDIFY_OPS_OUT")
    if out and REPORT:
        top = max(RATIOS, default=0.0)
        with open(out, "w") as f:
            f.write("The fast-mode DeOldify non-conv kernels (csrc/attention.hip, csrc/elementwise.hip) op by op against float64 (tests/test_gpu_deoldify_ops.py,\n"
                    "oracle.unet.self_attention_f64, tests/deoldify_ops_util.py).\n"
                    "attention: max over the output of |GPU - ref| / bound, bound = 2^-11 (|gamma| A + |ref|); the limit is 2.0 and a figure above 1.0 asks for an\n"
                    f"explanation.  Largest figure of this run: {top:.3f}" + (" (none above 1.0)" if top <= 1.0 else " (ABOVE 1.0)") + ".\n"
                    "affine: |GPU - exact| / (ulp16(exact) / 2 + 2^-22 (|x scale| + |shift|)); prep_rgb8: |GPU - exact| / (ulp16(exact) / 2 + 2^-20); <= 1 passes.\n"
                    "max-pool, blur + resize, copy and the transposed conv store are bit-exact checks and have no figure.\n\n")
            f.write("\n".join(REPORT) + "\n\nseconds per item (host wall clock, reference included)\n" + "\n".join(TIMES) + "\n")


@pytest.fixture(autouse=True)
def _timed(request):
    t0 = time.perf_counter()
    yield
    TIMES.append(f"{time.perf_counter() - t0:7.3f}  {request.node.name}")


# ---- self-attention -----------------------------------------------------------------------------------------------------------------------------------
_CACHE = {}


def attn_case(name, regime, gamma):
    """(case, inputs, (ref, A)) computed once per module and never written to"""
    case = U.CASES[name]
    if (name, regime) not in _CACHE:
        inp = U.attn_inputs(case, regime)
        U.check_regime(case, regime, inp[1], inp[2])
        for a in inp:
            a.setflags(write=False)
        _CACHE[name, regime] = inp
    if (name, regime, gamma) not in _CACHE:
        ref, A = U.attn_reference(case, *_CACHE[name, regime], gamma)
        ref.setflags(write=False)
        A.setflags(write=False)
        _CACHE[name, regime, gamma] = (ref, A)
    return case, _CACHE[name, regime], _CACHE[name, regime, gamma]


def held(case, regime, gamma, inp, ref_A, got, label, bad):
    ratio, worst = U.attn_ratio(got.astype(np.float64), ref_A[0], ref_A[1], gamma)
    RATIOS.append(ratio)
    note(f"attention {case.name:16s} {regime:8s} gamma {gamma:+.1f} {label:12s} max err / bound {ratio:.3f}")
    if not (ratio <= U.LIMIT and np.isfinite(got.astype(np.float32)).all()):
        bad.append(f"{case.name} {regime} gamma {gamma} {label}: " + U.attn_worst_text(case, inp[1], inp[2], worst, ratio))
    return ratio


@pytest.mark.parametrize("name", list(U.CASES))
def test_attention_is_within_the_bound_of_the_float64_reference(ctx, name):
    bad = []
    for regime in U.CASES[name].regimes:
        for gamma in U.GAMMAS:
            case, inp, ref_A = attn_case(name, regime, gamma)
            x, f, g, h = inp
            got, full = U.run_attention(ctx, x, f, g, U.value_rows(h, U.pad_to(case.N, 64)), gamma, batch=case.frames)
            held(case, regime, gamma, inp, ref_A, got, "", bad)
            assert (U.bits(full[case.frames:]) == SENT).all(), "frames past the batch were written"
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", list(U.CASES))
def test_attention_with_gamma_zero_returns_x_bit_for_bit(ctx, name):
    case, (x, f, g, h), _ = attn_case(name, "flat", 0.0)
    got, _ = U.run_attention(ctx, x, f, g, U.value_rows(h, U.pad_to(case.N, 64)), 0.0, batch=case.frames)
    assert np.array_equal(U.bits(got), U.bits(x[:case.frames]))


@pytest.mark.parametrize("name", ["d64c512n129", "d32c128n65"])
def test_attention_reads_and_writes_channel_views(ctx, name):
    """f | g at channel offset 64 of a 256-wide row, x at offset C of a 2 C-pitch buffer, y at offset 0 of a 2 C-pitch buffer whose other half is a sentinel"""
    bad = []
    case, inp, ref_A = attn_case(name, "flat", 0.7)
    x, f, g, h = inp
    got, full = U.run_attention(ctx, x, f, g, U.value_rows(h, U.pad_to(case.N, 64)), 0.7, views=True)
    held(case, "flat", 0.7, inp, ref_A, got, "views", bad)
    assert full.shape[-1] == 2 * case.C and (U.bits(full[..., case.C:]) == SENT).all(), "the other half of the destination buffer was written"
    plain, _ = U.run_attention(ctx, x, f, g, U.value_rows(h, U.pad_to(case.N, 64)), 0.7)
    assert np.array_equal(U.bits(got), U.bits(plain)), "the result depends on where the views lie"
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("extra", [0, 64])
@pytest.mark.parametrize("name", ["d32c128n15", "d64c384n65", "d64c512n129", "d96c768n200", "d32c256n63"])
def test_attention_never_weighs_the_value_padding(ctx, name, extra):
    """columns N .. npitch of every V^T row set to +-60000, npitch = pad_to(N, 64) [+ 64]: bit-identical to the zero-padded run, so P is exactly 0 for
    every masked key and no tile past the last key is walked.  (NaN or inf there is outside the contract: 0 x NaN is NaN in any MFMA.)"""
    case = U.CASES[name]
    npitch = U.pad_to(case.N, 64) + extra
    for regime in case.regimes:
        _, (x, f, g, h), _ = attn_case(name, regime, 0.7)
        r = np.random.default_rng(11)
        pad = np.where(r.integers(0, 2, (case.B, case.C, npitch - case.N)) == 1, 60000.0, -60000.0).astype(np.float16)
        zero, _ = U.run_attention(ctx, x, f, g, U.value_rows(h, npitch), 0.7)
        big, _ = U.run_attention(ctx, x, f, g, U.value_rows(h, npitch, pad), 0.7)
        same = U.bits(zero) == U.bits(big)
        assert same.all(), f"{name} {regime}: {int((~same).sum())} of {same.size} outputs change with the padding; first at {np.argwhere(~same)[:5].tolist()}"


@pytest.mark.parametrize("name,part", [("d64c512n129", 256), ("d64c384n65", 128)])
def test_attention_result_does_not_depend_on_the_channel_block(ctx, name, part):
    """C = 512 (kernel 2, two 256-channel blocks) == two C = 256 runs on the halves of V^T, x and y; C = 384 (kernel 1, three 128-channel blocks) == three
    C = 128 runs: bit for bit, a block's result may not depend on blockIdx.y"""
    case = U.CASES[name]
    for regime in ("flat", "sharp"):
        _, (x, f, g, h), _ = attn_case(name, regime, 0.7)
        vT = U.value_rows(h, U.pad_to(case.N, 64))
        whole, _ = U.run_attention(ctx, x, f, g, vT, 0.7)
        for c0 in range(0, case.C, part):
            piece, _ = U.run_attention(ctx, np.ascontiguousarray(x[..., c0:c0 + part]), f, g, np.ascontiguousarray(vT[:, c0:c0 + part]), 0.7)
            same = U.bits(piece) == U.bits(whole[..., c0:c0 + part])
            assert same.all(), f"{name} {regime} channels {c0}..{c0 + part}: {int((~same).sum())} differ; first at {np.argwhere(~same)[:5].tolist()}"


# ---- the runtime's side of the fast attention op: refusals ---------------------------------------------------------------------------------------------------
def _refused(ctx, b, batch, match):
    """the plan is refused with HAVC_E_INVALID (ValueError in _native._check) and a message that names the op, before anything is launched"""
    from tests.gpu_util import run_plan
    from vsdeoldify_amd.plan import WeightPack
    launches = ctx.stats().launches
    with pytest.raises(ValueError, match=match):
        run_plan(ctx, WeightPack(), b, {}, {}, batch)
    assert ctx.stats().launches == launches, "a kernel was launched for a refused plan"


REFUSALS = {
    "d_not_32_64_96": (dict(d=48), {}, r"attention op: d \(aux0\) must be 32, 64 or 96"),
    "d_128": (dict(d=128), {}, r"attention op: d \(aux0\) must be 32, 64 or 96"),
    "C_not_a_multiple_of_128": (dict(C=192), {}, r"attention op: C % 128 == 0"),
    "Kc_not_a_multiple_of_64": ({}, dict(Kc=96), r"attention op: value pitch Kc % 64 == 0, Kc >= N"),
    "Kc_below_N": (dict(npitch=64), {}, r"attention op: value pitch Kc % 64 == 0, Kc >= N"),
    "vT_buffer_too_small": (dict(vT_elems=256 * 128 - 8), {}, r"attention op: fp16 buffers of N x pitch elements per frame, V\^T of C x Kc"),
    "f_g_past_the_row": ({}, dict(res_coff=8), r"attention op: views inside their pixel rows"),
    "x_past_the_row": ({}, dict(src_coff=8), r"attention op: views inside their pixel rows"),
    "y_past_the_row": ({}, dict(dst_coff=8), r"attention op: views inside their pixel rows"),
    "qk_buffer_not_fp16": (dict(qk_bytes=4), {}, r"attention op: fp16 buffers of N x pitch elements per frame"),
    "x_buffer_too_small": (dict(x_rows=64), {}, r"attention op: fp16 buffers of N x pitch elements per frame"),
    "y_buffer_too_small": (dict(y_rows=64), {}, r"attention op: fp16 buffers of N x pitch elements per frame"),
    "qk_buffer_too_small": (dict(qk_rows=64), {}, r"attention op: fp16 buffers of N x pitch elements per frame"),
}


@pytest.mark.parametrize("what", list(REFUSALS))
def test_fast_attention_refuses_what_its_kernels_cannot_run(ctx, what):
    """N = 65, d = 64, C = 256, Kc = 128 with one thing wrong.  Nothing is uploaded and nothing may be launched: the plan is refused by the host checks."""
    from vsdeoldify_amd.plan import PlanBuilder, View
    shape, fields, match = REFUSALS[what]
    N, d, C, npitch = 65, shape.get("d", 64), shape.get("C", 256), shape.get("npitch", 128)
    b = PlanBuilder()
    xv = View(b.buf(shape.get("x_rows", N) * C), 0, C, 1, N, C, C)
    qv = View(b.buf(shape.get("qk_rows", N) * 2 * d, shape.get("qk_bytes", 2)), 0, 2 * d, 1, N, 2 * d, 2 * d)
    yv = View(b.buf(shape.get("y_rows", N) * C), 0, C, 1, N, C, C)
    vb = b.buf(shape.get("vT_elems", C * npitch))
    i = b.attention("attn", xv, qv, d, vb, npitch, yv, 0.7)
    for k, v in fields.items():
        b.ops[i][k] = v
    _refused(ctx, b, 1, match)


# ---- frames of views that do not fill their buffers' frames -------------------------------------------------------------------------------------------------
H5, W7, B3 = 5, 7, 3


def _frames_plan(kind, precise, extra):
    """one op of `kind` on an H5 x W7 view of buffers that hold `extra` more rows per frame (1 = the token-buffer shape of
    test_conv_views_that_do_not_fill_their_frame_run_frame_by_frame) -> (builder, pack, {buffer: (rows, row elements, dtype)} of the
    uploads, the destination buffers)"""
    from vsdeoldify_amd import _native as nat
    from vsdeoldify_amd.plan import PlanBuilder, View, WeightPack
    pack, b = WeightPack(), PlanBuilder(precise=precise)
    pm, C = b.pm, 64
    Ho, Wo = {"maxpool": (3, 4), "blur": (4, 6)}.get(kind, (H5, W7))
    ups, dsts = {}, []

    def view(H, W, pitch, coff, span, elem=2):
        rows = H * W + extra
        v = View(b.buf(rows * pitch, elem), coff, pitch, H, W, span, span)
        ups[v.buf] = (rows, pitch, np.float16)
        return v
    if kind == "prep":
        src = b.buf((H5 * W7 + extra) * 3, 1)
        ups[src] = (H5 * W7 + extra, 3, np.uint8)
        y0, y1 = view(H5, W7, 8 * pm, 0, 8), view(H5, W7, 64 * pm, 32, 8)
        i = b.prep_rgb8("op", src, H5, y0, y1, y1_fill=24)
        b.ops[i]["Wi"] = b.ops[i]["Wo"] = W7
        dsts = [y0.buf, y1.buf]
    elif kind == "attention":
        N, d, Ca, npitch = H5 * W7, 32, 128, 64
        xv, qv, yv = view(1, N, Ca, 0, Ca), view(1, N, 2 * d, 0, 2 * d), view(1, N, Ca, 0, Ca)
        vb = b.buf(Ca * npitch + 64 * extra)
        ups[vb] = (Ca * npitch // 64 + extra, 64, np.float16)
        b.attention("op", xv, qv, d, vb, npitch, yv, 0.7)
        dsts = [yv.buf]
    else:
        xv, yv = view(H5, W7, (C + 64) * pm, 8, C), view(Ho, Wo, (C + 64) * pm, 16, C)
        if kind == "maxpool":
            b.maxpool("op", xv, yv)
        elif kind == "blur":
            b.blur_resize("op", xv, yv)
        elif kind == "affine":
            r = np.random.default_rng(4)
            b.affine("op", xv, yv, pack.add(r.standard_normal(C).astype(np.float32)), pack.add(r.standard_normal(C).astype(np.float32)), True)
        else:
            b._op("op", type=nat.OP_COPY_CH, src=xv.buf, src_coff=xv.coff, src_cpitch=xv.cpitch, dst=yv.buf, dst_coff=yv.coff, dst_cpitch=yv.cpitch,
                  Hi=H5, Wi=W7, Ci=C, Ho=H5, Wo=W7, Co=C)
        dsts = [yv.buf]
    return b, pack, ups, dsts


@pytest.mark.parametrize("kind,precise", [("maxpool", False), ("maxpool", True), ("blur", False), ("blur", True), ("affine", False), ("affine", True),
                                          ("copy", False), ("prep", False), ("prep", True), ("attention", False)])
def test_a_batch_on_views_that_do_not_fill_their_frames_runs_frame_by_frame(ctx, kind, precise):
    """B = 3 on buffers of h x w + 1 rows per frame, the op on their h x w views (h, w = 5, 7): the extra row of every frame keeps its sentinel and the
    views hold, bit for bit, what the dense run of the same frames gives.  (As one launch with frame b at b x h x w x pitch, frame 1 began on frame
    0's extra row.)  The copy op has no precise form; the fast attention op's V^T buffer carries 64 extra elements per frame instead of a row."""
    from tests.gpu_util import run_plan
    got, before = {}, {}
    for extra in (0, 1):
        b, pack, ups, dsts = _frames_plan(kind, precise, extra)
        arrays = {}
        r = np.random.default_rng(23)                                           # the same frames in both runs; the destinations start with random values too
        for buf, (rows, width, dt) in ups.items():
            n = rows - extra
            a = np.empty((B3, rows, width), dt)
            a[:, :n] = r.integers(0, 256, (B3, n, width), dtype=np.uint8) if dt == np.uint8 else U.f16(r.standard_normal((B3, n, width)))
            if extra:
                a[:, n:] = 201 if dt == np.uint8 else U.SENTINEL
            arrays[buf] = a
        out = run_plan(ctx, pack, b, arrays, {d: (arrays[d].shape, arrays[d].dtype) for d in dsts}, B3)
        got[extra], before[extra] = [out[d] for d in dsts], [arrays[d] for d in dsts]
        if extra:
            for d in dsts:
                assert (U.bits(out[d][:, -1]) == SENT).all(), "the extra row of a frame was written"
    for dense, token, was in zip(got[0], got[1], before[0]):
        assert (U.bits(dense) != U.bits(was)).any(axis=(1, 2)).all(), "the dense run left a frame as it was"
        same = U.bits(dense) == U.bits(token[:, :dense.shape[1]])
        assert same.all(), f"{kind}: {int((~same).sum())} of {same.size} elements differ from the dense run; first (frame, row, channel): {np.argwhere(~same)[:5].tolist()}"


# ---- element-wise kernels, one op each ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", U.CHANNELS)
@pytest.mark.parametrize("H,W", U.SHAPES)
def test_maxpool_is_the_float64_maximum_of_the_valid_taps(ctx, H, W, C):
    r = np.random.default_rng([H, W, C])
    x = U.f16(r.standard_normal((2, H, W, C)))
    x[..., 0] = np.float16(-65504.0)                                            # a channel that never rises above the kernel's starting value
    x[..., 1] = np.where(r.integers(0, 2, (2, H, W)) == 1, 0.0, -0.0).astype(np.float16)      # -0 against +0: the value decides, not the sign
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    got, full = U.run_ew(ctx, "maxpool", x, Ho, Wo)
    want = U.maxpool_f64(x)
    assert got.shape == want.shape and np.array_equal(got.astype(np.float64), want)
    assert (got[..., 0] == -65504.0).all() and (got[..., 1] == 0).all()
    assert U.outside_is_sentinel(full, 16, C)


BLUR_SIZES = [((18, 18), (18, 18)), ((18, 18), (17, 17)), ((18, 18), (17, 18)), ((18, 18), (18, 17)), ((9, 9), (18, 18)), ((36, 36), (35, 35))] + \
             [(s, s) for s in U.SHAPES if s != (18, 18)]


@pytest.mark.parametrize("C", U.CHANNELS)
@pytest.mark.parametrize("src,dst", BLUR_SIZES)
def test_blur_resize_is_the_rounded_float64_mean_bit_for_bit(ctx, src, dst, C):
    x = U.blur_inputs((2,) + src + (C,), [src[0], src[1], dst[0], dst[1], C])
    got, full = U.run_ew(ctx, "blur", x, dst[0], dst[1])
    want = U.blur_resize_f64(x, dst[0], dst[1]).astype(np.float16)
    same = U.bits(got) == U.bits(want)
    assert same.all(), f"{int((~same).sum())} of {same.size} differ; first (frame, y, x, channel): {np.argwhere(~same)[:5].tolist()}"
    assert U.outside_is_sentinel(full, 16, C)


AFFINE_SHAPES = [(2,) + s for s in U.SHAPES] + [(1, 1, 1), (1, 1, 3)]           # (B, H, W): pixel counts 2, 12, 70, 648, 1054 and 1, 3


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("C", U.CHANNELS)
def test_affine_is_within_half_an_ulp_and_the_fp32_terms(ctx, C, relu):
    worst = 0.0
    for B, H, W in AFFINE_SHAPES:
        r = np.random.default_rng([B, H, W, C])
        x = U.f16(2.0 * r.standard_normal((B, H, W, C)))
        scale, shift = (1.5 * r.standard_normal(C)).astype(np.float32), (3.0 * r.standard_normal(C)).astype(np.float32)
        got, full = U.run_ew(ctx, "affine", x, H, W, scale, shift, relu)
        exact, mag = U.affine_exact(x, scale, shift, relu)
        assert np.abs(exact).max() < 1000
        e = U.affine_excess(got, exact, mag)
        worst = max(worst, float(e.max()))
        assert e.max() <= 1.0, (B, H, W, float(e.max()), np.unravel_index(int(e.argmax()), e.shape))
        assert not relu or not np.signbit(got).any()
        assert U.outside_is_sentinel(full, 16, C)
    note(f"affine C {C:3d} relu {int(relu)} ({'fast' if 256 % (C // 8) == 0 else 'generic'} kernel): max |err| / rule {worst:.4f}")


@pytest.mark.parametrize("C", U.CHANNELS)
def test_copy_ch_is_bit_exact(ctx, C):
    for B, H, W in AFFINE_SHAPES:
        x = U.finite_patterns((B, H, W, C), [B, H, W, C])
        got, full = U.run_ew(ctx, "copy", x, H, W)
        assert np.array_equal(U.bits(got), U.bits(x)), (B, H, W)
        assert U.outside_is_sentinel(full, 16, C)


def test_prep_rgb8_in_both_kernels(ctx):
    """all 256 greys and the 16^3 RGB lattice (frame 0), random pixels (frame 1) through prep_rgb8_kernel (no second destination; a second destination
    that is not 64-byte aligned) and prep_rgb8_fill_kernel (aligned slot + 24 pad channels)"""
    rgb = U.prep_images()
    L = U.gray_l(rgb).reshape(2, -1)
    exact = U.prep_exact(L)
    table = U.prep_exact(np.arange(256))                                          # [256][3]
    outs = {form: U.run_prep(ctx, rgb, form) for form in ("single", "plain", "fill")}
    for form, (y0, y1, slot) in outs.items():
        for label, t in (("y0", y0[..., 8:16]),) + ((("slot", y1[..., slot:slot + 8]),) if y1 is not None else ()):
            e = U.prep_excess(t[..., :3], exact)
            note(f"prep_rgb8 {form:6s} {label:4s}: max |err| / rule {e.max():.4f}")
            assert e.max() <= 1.0, (form, label, float(e.max()), np.unravel_index(int(e.argmax()), e.shape))
            for c in range(3):                                                  # L itself, read back through the value: the nearest of the 256 levels
                back = np.abs(t[..., c].astype(np.float64)[..., None] - table[:, c]).argmin(-1)
                assert np.array_equal(back, L), (form, label, c)
            assert not U.bits(t[..., 3:]).any(), f"{form} {label}: channels 3-7 are not +0"
        assert U.outside_is_sentinel(y0, 8, 8)
        if form == "plain":
            assert U.outside_is_sentinel(y1, slot, 8)
        if form == "fill":
            assert not U.bits(y1[..., slot + 8:slot + 32]).any(), "the 24 pad channels behind the slot are not +0"
            assert U.outside_is_sentinel(y1, slot, 32)
    assert np.array_equal(U.bits(outs["single"][0]), U.bits(outs["plain"][0])) and np.array_equal(U.bits(outs["plain"][0]), U.bits(outs["fill"][0]))
    assert np.array_equal(U.bits(outs["plain"][1][..., 280:288]), U.bits(outs["fill"][1][..., 288:296])), "the two kernels fill the slot differently"
    assert np.array_equal(U.bits(outs["fill"][0][..., 8:16]), U.bits(outs["fill"][1][..., 288:296]))


@pytest.mark.parametrize("C,H,W,npitch", [(128, 5, 13, 128), (256, 10, 20, 256)])
def test_transposed_conv_store_is_the_plain_store_transposed(ctx, C, H, W, npitch):
    """a 1x1 conv with HAVC_F_OUT_TRANSPOSED into a sentinel-filled [C][npitch] buffer (the attention's V^T), B = 2: columns < N equal the plain conv's
    NHWC output transposed, bit for bit; columns >= N keep the sentinel"""
    from tests.gpu_util import nhwc_pad, run_plan
    from vsdeoldify_amd import _native as nat
    from vsdeoldify_amd.plan import PlanBuilder, WeightPack, pack_conv
    r = np.random.default_rng([C, H, W])
    Cin, N = 64, H * W
    x = U.f16(r.standard_normal((2, Cin, H, W))).astype(np.float32)
    w = U.f16(r.standard_normal((C, Cin, 1, 1)) / 8).astype(np.float32)
    pack, b = WeightPack(), PlanBuilder()
    xv = b.tensor(H, W, Cin)
    pc = pack_conv(pack, w, xv.cmap, xv.span)
    yv = b.tensor(H, W, C)
    b.conv("plain", pc, xv, yv)
    vT = b.buf(C * npitch)
    b.conv("transposed", pc, xv, vT, flags=nat.F_OUT_TRANSPOSED, Co=C, aux0=npitch)
    out = run_plan(ctx, pack, b, {xv.buf: nhwc_pad(x, xv.cpitch), vT: np.full((2, C, npitch), U.SENTINEL, np.float16)},
                   {yv.buf: ((2, N, yv.cpitch), np.float16), vT: ((2, C, npitch), np.float16)}, 2)
    plain, t = out[yv.buf][..., :C], out[vT]
    assert np.abs(plain.astype(np.float32)).max() > 0.5
    assert np.array_equal(U.bits(t[:, :, :N]), U.bits(plain.transpose(0, 2, 1)))
    assert (U.bits(t[:, :, N:]) == SENT).all(), "columns past N were written"
