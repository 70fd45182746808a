"""GPU: the fast-mode non-conv kernels of DDColor (csrc/ddcolor.hip: both D = 32 attention kernels and the merge, LayerNorm in all four lane widths,
depthwise 7 x 7 alone and fused with LayerNorm, PixelShuffle(4) + blur, fold_queries, shuf4_blur_ab) and of the Zhang colorizers (csrc/elementwise.hip:
subsample2, proj2, bilinear2) one op at a time against plain float64 -- each through a one-op plan whose buffers are uploaded directly and whose
destination starts as a sentinel (tests/ddcolor_ops_util.py: the cases, the inputs, the oracles, the rules and their derivations;
tests/test_ddcolor_ops_host.py shows on the CPU that those rules can fail).  The attention cases reach what only the benchmark reached before: blocks of
the key-split kernel that walk two and four 256-key chunks, the ragged last block, and the one-block form of the coarse level.  Also here: what the
runtime's dispatch owes these ops (csrc/rt_net.cpp): more than 128 queries go to the kernel that can run them, channel counts the kernels cannot run are
refused before any launch, and a batch on views that do not fill their buffers' frames runs frame by frame.

HAVC_DDCOLOR_OPS_OUT=<file> writes every measured figure and the time of every item (profiles/ddcolor_ops.txt)."""
import os
import time

import numpy as np
import pytest

from tests import ddcolor_ops_util as U

pytestmark = pytest.mark.gpu
REPORT, TIMES, RATIOS = [], [], {}
SENT = U.SENT
F = np.float32


def note(op, ratio, line):
    RATIOS[op] = max(RATIOS.get(op, 0.0), float(ratio))
    REPORT.append(line)
    print(line)


@pytest.fixture(scope="module", autouse=True)
def _profile():
    yield
    out = os.environ.get("HAVC_DDCOLOR_OPS_OUT")
    if out and REPORT:
        top = max((v for k, v in RATIOS.items() if k.startswith("mha")), default=0.0)
        with open(out, "w") as f:
            f.write("The fast-mode DDColor and Zhang non-conv kernels (csrc/ddcolor.hip, csrc/elementwise.hip) op by op against float64\n"
                    "(tests/test_gpu_ddcolor_ops.py; the rules and their derivations: tests/ddcolor_ops_util.py).  Every figure is max |GPU - ref| / bound.\n"
                    "attention: bound = 2^-11 (A + |ref|); the limit is 2.0 and a figure above 1.0 asks for an explanation.  Largest attention figure of this\n"
                    f"run: {top:.3f}" + (" (none above 1.0: nothing to explain)" if top <= 1.0 else " (ABOVE 1.0)") + ".  Every other op passes at 1.0 or below.\n"
                    "subsample2, the blur on exactly summable inputs and the placement checks are bit-exact and have no figure.\n\n"
                    "largest figure per op\n" + "\n".join(f"{v:8.4f}  {k}" for k, v in sorted(RATIOS.items())) + "\n\n")
            f.write("\n".join(REPORT) + "\n\nseconds per item (host wall clock, inputs and reference included; the first item that computes a reference with\n"
                    "torch also pays for importing it when this file runs alone)\n" + "\n".join(TIMES) + "\n")


@pytest.fixture(autouse=True)
def _timed(request):
    t0 = time.perf_counter()
    yield
    TIMES.append(f"{time.perf_counter() - t0:7.3f}  {request.node.name}")


def _same(a, b, what):
    same = U.bits(a) == U.bits(b)
    assert same.all(), f"{what}: {int((~same).sum())} of {same.size} differ; first at {np.argwhere(~same)[:5].tolist()}"


# ---- multi-head attention ---------------------------------------------------------------------------------------------------------------------------------------
_CACHE = {}


def mha_case(name, regime):
    """(case, (q, k, v), reference) computed once per module and never written to; the large cases share one pool of random K / V rows"""
    case = U.MHA_CASES[name]
    if (name, regime) not in _CACHE:
        q, k, v = U.mha_inputs(case, regime)
        ref = U.mha_reference(q, k, v, case.heads, tgt=U.mha_targets(case, regime, k) if regime != "flat" else None)
        U.check_regime(case, regime, ref)
        for a in (q, ref["out"], ref["A"]):
            a.setflags(write=False)
        _CACHE[name, regime] = (case, (q, k, v), ref)
    return _CACHE[name, regime]


def _via_aux1(case):
    return case.kernel == "plain" and case.name.startswith("plain_")


@pytest.mark.parametrize("regime", U.REGIMES)
@pytest.mark.parametrize("name", list(U.MHA_CASES))
def test_attention_is_within_the_bound_of_the_float64_reference(ctx, name, regime):
    case = U.MHA_CASES[name]
    assert U.launcher_choice(case.B, case.heads, case.Lk) == (case.nch, case.nsplit), "the launcher's rule no longer selects the path this case is named for"
    case, (q, k, v), ref = mha_case(name, regime)
    got, full = U.run_mha(ctx, q, k, v, case.heads, case.layout, plain=_via_aux1(case))
    ratio, worst = U.mha_ratio(got, ref)
    kern = "mha32_kernel" if case.kernel == "plain" else f"split nch {case.nch} nsplit {case.nsplit}"
    note("mha " + ("plain" if case.kernel == "plain" else "split"), ratio,
         f"attention {name:14s} B {case.B:3d} heads {case.heads} Lq {case.Lq:3d} Lk {case.Lk:4d} {case.layout:5s} {kern:24s} {regime:6s} max err / bound {ratio:.3f}")
    assert np.isfinite(got.astype(F)).all() and ratio <= U.LIMIT, U.mha_worst_text(case, worst, ratio)
    assert U.mha_untouched(full, case.Lq, case.E), "rows past the queries or channels outside the view were written"


@pytest.mark.parametrize("name", ["k1", "k7", "k33", "k255", "k257", "k513", "q17", "q128", "q200", "plain_k65q100", "plain_k300q200"])
def test_attention_never_weighs_rows_past_the_keys(ctx, name):
    """rows Lk .. kv_tok of K and V set to +-60000: bit-identical to zeros there, so P is exactly 0 for every masked key and no row past the last key is
    read into a product.  (NaN or inf there is outside the contract: 0 x NaN is NaN in any MFMA.)"""
    for regime in U.REGIMES:
        case, (q, k, v), _ = mha_case(name, regime)
        zero, _ = U.run_mha(ctx, q, k, v, case.heads, case.layout, plain=_via_aux1(case))
        big, _ = U.run_mha(ctx, q, k, v, case.heads, case.layout, plain=_via_aux1(case), pad="big")
        _same(zero, big, f"{name} {regime}: outputs that change with the rows past the keys")


@pytest.mark.parametrize("name", ["q1", "q17", "q112", "q128", "q129"])
def test_attention_result_does_not_depend_on_the_batch(ctx, name):
    """frame 0 of the B = 3 (2) run equals the B = 1 run bit for bit at nch = 1: the frames' token strides are explicit in the op"""
    for regime in U.REGIMES:
        case, (q, k, v), _ = mha_case(name, regime)
        assert case.nch == 1 and case.B > 1
        whole, _ = U.run_mha(ctx, q, k, v, case.heads, case.layout)
        for f in (0, case.B - 1):
            one, _ = U.run_mha(ctx, q[f:f + 1], k[f:f + 1], v[f:f + 1], case.heads, case.layout)
            _same(whole[f:f + 1], one, f"{name} {regime} frame {f}")


@pytest.mark.parametrize("name", ["k257", "k513", "self100"])
def test_attention_heads_are_independent(ctx, name):
    """an 8-head run equals, bit for bit, eight 1-head runs on the channel slices"""
    for regime in ("flat", "edges"):
        case, (q, k, v), _ = mha_case(name, regime)
        whole, _ = U.run_mha(ctx, q, k, v, case.heads, case.layout)
        for h in range(case.heads):
            sl = np.s_[..., h * 32:h * 32 + 32]
            one, _ = U.run_mha(ctx, np.ascontiguousarray(q[sl]), np.ascontiguousarray(k[sl]), np.ascontiguousarray(v[sl]), 1, case.layout)
            _same(whole[sl], one, f"{name} {regime} head {h}")


# ---- LayerNorm -----------------------------------------------------------------------------------------------------------------------------------------------------
def _ln_held(ctx, C, x, eps, relu, label, views=True, B=1):
    g, b = U.ln_params(C)
    got, full = U.run_layernorm(ctx, x, g, b, eps, relu, views, B)
    e = U.ln_excess(got[:, :C], x, g, b, eps, relu)
    note(f"layernorm LP {U.ln_lanes(C)}", e.max(), f"layernorm C {C:4d} (LP {U.ln_lanes(C):2d}) pixels {len(x):5d} eps {eps:g} relu {int(relu)} {label:8s} max |err| / rule {e.max():.4f}")
    assert e.max() <= 1.0, (label, float(e.max()), np.unravel_index(int(e.argmax()), e.shape))
    assert not U.bits(got[:, C:]).any(), "the pad channels C .. C8 8 are not +0"
    assert not relu or not np.signbit(got).any()
    if views:
        assert U.outside_is_sentinel(full, 16, U.pad_to(C, 8))
    return got, g, b


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("C", U.LN_CHANNELS)
def test_layernorm_is_within_half_an_ulp_and_the_fp32_terms(ctx, C, relu):
    assert U.ln_lanes(C) == U.LN_LP[C], "the launcher's rule no longer selects the lane width this channel count is listed for"
    for npix in U.LN_PIXELS:
        for kind, eps in (("random", 1e-6), ("offset", 1e-5)) + ((("special", 1e-6),) if npix >= 7 else ()):
            x = U.ln_inputs(kind, npix, C)
            got, g, b = _ln_held(ctx, C, x, eps, relu, kind)
            if kind == "special":                                  # the all-equal pixel is beta (or its ReLU) exactly; the +-60000 pixel is finite
                want = np.maximum(b, 0).astype(np.float16) if relu else b.astype(np.float16)
                _same(got[npix // 2, :C], want, f"C {C}: the pixel of equal values")
                assert np.isfinite(got[-1].astype(F)).all()
    _ln_held(ctx, C, U.ln_inputs("random", 9, C, 1), 1e-5, relu, "dense", views=False)


@pytest.mark.parametrize("LP,C,npix", U.LN_SWEEPS)
def test_layernorm_walks_the_pixels_past_one_sweep_of_the_capped_grid(ctx, LP, C, npix):
    assert U.ln_lanes(C) == LP and U.ln_grid(npix, LP) == 1024 and npix > 1024 * 4 * (64 // LP)
    _ln_held(ctx, C, U.ln_inputs("random", npix, C), 1e-6, False, "sweeps")


# ---- depthwise 7 x 7, alone and with LayerNorm ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", U.DW_CHANNELS)
@pytest.mark.parametrize("H,W", U.DW_SHAPES)
def test_dwconv7_is_within_half_an_ulp_and_the_fp32_terms(ctx, H, W, C):
    w, bias, _, _ = U.dw_params(C)
    x = U.f16(np.random.default_rng([H, W, C]).standard_normal((2, H, W, C)))
    for bb in (bias, None):
        got, full = U.run_dwconv7(ctx, x, w, bb)
        ref, mag = U.dwconv7_f64(x, w, bb)
        e = U.dw_excess(got, ref, mag)
        note("dwconv7", e.max(), f"dwconv7 {H:2d} x {W:2d} C {C:3d} bias {int(bb is not None)}: max |err| / rule {e.max():.4f}")
        assert e.max() <= 1.0, (float(e.max()), np.unravel_index(int(e.argmax()), e.shape))
        assert U.outside_is_sentinel(full, 16, C)


@pytest.mark.parametrize("C", [8, 200])
def test_dwconv7_of_a_single_one_is_the_flipped_kernel(ctx, C):
    """a 1.0 at each corner and at the centre of a 13 x 10 image (one frame each): the output is the 7 x 7 kernel mirrored about that pixel, bit for bit
    (the weights are fp16), and +0 elsewhere -- a transposed or shifted tap table cannot pass"""
    H, W = 13, 10
    w, _, _, _ = U.dw_params(C)
    spots = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 2)]
    x = np.zeros((len(spots), H, W, C), np.float16)
    want = np.zeros((len(spots), H, W, C), np.float16)
    for f, (py, px) in enumerate(spots):
        x[f, py, px] = 1.0
        for dy in range(7):
            for dx in range(7):
                ho, wo = py - dy + 3, px - dx + 3
                if 0 <= ho < H and 0 <= wo < W:
                    want[f, ho, wo] = w[:, dy, dx]
    got, _ = U.run_dwconv7(ctx, x, w, None)
    _same(got, want, f"C {C}")


@pytest.mark.parametrize("C,H,W,B,views", [s + (False,) for s in U.DWLN_SHAPES] + [(192, 13, 10, 3, True), (1536, 5, 6, 3, True)])
def test_dwconv7_layernorm_fused_is_within_the_layernorm_rule_of_the_float64_composition(ctx, C, H, W, B, views):
    w, bias, g, be = U.dw_params(C)
    x = U.f16(np.random.default_rng(C + H).standard_normal((B, H, W, C)))
    got, full = U.run_dwconv7(ctx, x, w, bias, ln=(g, be, 1e-6), views=views)
    conv, _ = U.dwconv7_f64(x, w, bias)
    e = U.ln_excess(got, conv, g, be, 1e-6)
    note("dwconv7_ln", e.max(), f"dwconv7_ln C {C:4d} {H:2d} x {W:2d} B {B:2d} views {int(views)}: max |err| / rule {e.max():.4f}")
    assert e.max() <= 1.0, (float(e.max()), np.unravel_index(int(e.argmax()), e.shape))
    assert not views or U.outside_is_sentinel(full, 16, C)


# ---- PixelShuffle(4) + blur -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", U.PS_CHANNELS)
@pytest.mark.parametrize("Hi,Wi", U.PS_SHAPES)
def test_pixshuf4_blur_is_the_rounded_float64_mean(ctx, Hi, Wi, C):
    """bit for bit where the fp32 sum is exact (blur_inputs; the marks: every sub-pixel group and channel its own constant), within half an ulp and the
    fp32 sum's rounding on arbitrary fp16 values (the double rounding is named in tests/ddcolor_ops_util.py)"""
    for label, x in (("exact", U.blur_inputs((2, Hi, Wi, 16 * C), [Hi, Wi, C])), ("marks", U.ps_marks(2, Hi, Wi, C))):
        got, full = U.run_pixshuf4_blur(ctx, x)
        _same(got, U.pixshuf4_blur_f64(x)[0].astype(np.float16), f"{label} {Hi} x {Wi} C {C}")
        assert U.outside_is_sentinel(full, 16, C)
    x = U.ps_patterns((2, Hi, Wi, 16 * C), [Hi, Wi, C])
    got, full = U.run_pixshuf4_blur(ctx, x)
    ref, mag = U.pixshuf4_blur_f64(x)
    e = np.abs(got.astype(np.float64) - ref) / (U.ulp16(ref) / 2 + 4 * U.U32 * mag)
    note("pixshuf4_blur", e.max(), f"pixshuf4_blur {Hi} x {Wi} C {C:3d} arbitrary fp16 values: max |err| / rule {e.max():.4f}, {int((U.bits(got) != U.bits(ref.astype(np.float16))).sum())} "
         f"of {got.size} differ from float16(float64 mean)")
    assert e.max() <= 1.0 and U.outside_is_sentinel(full, 16, C)


# ---- Zhang ops -----------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", U.SUB_CHANNELS)
def test_subsample2_is_a_bit_exact_copy(ctx, C):
    for H, W in U.SUB_SHAPES:
        x = U.finite_patterns((2, H, W, C), [H, W, C])
        got, full = U.run_subsample2(ctx, x)
        _same(got, x[:, ::2, ::2], f"{H} x {W}")
        assert U.outside_is_sentinel(full, 16, C)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("C", U.PROJ_CHANNELS)
def test_proj2_is_within_its_fp32_bound(ctx, C, mode):
    for npix in U.PROJ_PIXELS:
        x, w, bias = U.proj_inputs(C, npix, mode)
        got = U.run_proj2(ctx, x, w, bias, mode, U.AB_MUL)
        ref, bound = U.proj2_f64(x, w, bias, mode, U.AB_MUL)
        e = np.abs(got.astype(np.float64) - ref) / bound
        note(f"proj2 mode {mode}", e.max(), f"proj2 mode {mode} C {C:3d} pixels {npix:4d}: max |err| / bound {e.max():.4f}")
        assert np.isfinite(got).all() and e.max() <= 1.0, (npix, float(e.max()), np.unravel_index(int(e.argmax()), e.shape))


@pytest.mark.parametrize("src,dst", U.BILINEAR_SIZES)
def test_bilinear2_is_the_float64_formula_on_the_float32_coordinates(ctx, src, dst):
    x = np.random.default_rng([src[0], src[1], dst[0]]).standard_normal((2,) + src + (2,)).astype(F)
    got = U.run_bilinear2(ctx, x, dst[0], dst[1], U.AB_MUL)
    fig, how = U.bilinear_excess(got, x, dst[0], dst[1], U.AB_MUL)
    note("bilinear2", fig, f"bilinear2 {src} -> {dst}: max |err| / bound {fig:.4f} (source coordinate: {how})")
    assert fig <= 1.0


# ---- DDColor tail ----------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [8, 256, 264])
def test_fold_queries_is_within_its_fp32_bound(ctx, C):
    """100 queries of a 112-row token buffer, B = 3: rows 100 .. 111 hold 3000 (nothing may read them), and every frame equals its own one-frame run bit
    for bit -- the op carries the token stride"""
    r = np.random.default_rng(C)
    e = U.f16(r.standard_normal((3, 112, C)))
    e[:, 100:] = np.float16(3000.0)
    rq = np.zeros((2, 104), F)
    rq[:, :100] = r.standard_normal((2, 100)).astype(F)
    got = U.run_fold_queries(ctx, e, rq, 100)
    ref, mag = U.fold_f64(e, rq, 100)
    fig = (np.abs(got.astype(np.float64) - ref) / (101 * U.U32 * mag)).max()
    note("fold_queries", fig, f"fold_queries C {C:3d}: max |err| / bound {fig:.4f}")
    assert fig <= 1.0
    for f in range(3):
        assert np.array_equal(got[f:f + 1].view(np.uint32), U.run_fold_queries(ctx, e[f:f + 1], rq, 100).view(np.uint32)), f
    _refused(ctx, *_fold_plan(C, nq=113), r"fold-queries op")                  # more queries than token rows


def _fold_plan(C, nq):
    from vsdeoldify_amd.plan import PlanBuilder, View, WeightPack
    pack, b = WeightPack(), PlanBuilder()
    ev = View(b.buf(112 * C), 0, C, 1, 112, C, C)
    b.fold_queries("fold", ev, nq, pack.add(np.zeros((2, 120), F)), 120, b.buf(2 * C, 4))
    return pack, b


@pytest.mark.parametrize("y_coff", [16, 11])
@pytest.mark.parametrize("Hi,Wi", U.PS_SHAPES)
def test_shuf4_blur_ab_in_both_stores(ctx, Hi, Wi, y_coff):
    """y_coff % 8 == 0: one 16-byte store, channels 2 .. 7 of the chunk are +0; an odd offset: two scalar stores, everything else keeps the sentinel"""
    r = np.random.default_rng([Hi, Wi, y_coff])
    proj = r.standard_normal((2, Hi, Wi, 16, 2)).astype(F)
    img = U.f16(r.standard_normal((2, 4 * Hi, 4 * Wi, 3)))
    rimg, bias = r.standard_normal((2, 3)).astype(F), r.standard_normal(2).astype(F)
    full = U.run_shuf4_blur_ab(ctx, proj, img, rimg, bias, y_coff)
    ref, mag = U.shuf_ab_f64(proj, img, rimg, bias)
    e = U.shuf_ab_excess(full[..., y_coff:y_coff + 2], ref, mag)
    note("shuf4_blur_ab", e.max(), f"shuf4_blur_ab {Hi} x {Wi} y_coff {y_coff:2d}: max |err| / rule {e.max():.4f}")
    assert e.max() <= 1.0, (float(e.max()), np.unravel_index(int(e.argmax()), e.shape))
    if y_coff % 8 == 0:
        assert not U.bits(full[..., y_coff + 2:y_coff + 8]).any(), "channels 2 .. 7 of the chunk are not +0"
        assert U.outside_is_sentinel(full, y_coff, 8)
    else:
        assert U.outside_is_sentinel(full, y_coff, 2)


# ---- the runtime's side: refusals ----------------------------------------------------------------------------------------------------------------------------------------
def _refused(ctx, pack, b, match, ups=None, keep=None):
    """the plan is refused with HAVC_E_INVALID (ValueError in _native._check) and a message that names the op, before anything is launched; `keep` =
    (buffer, shape, dtype): that buffer, uploaded in `ups`, is unchanged afterwards"""
    from vsdeoldify_amd import _native as nat
    ops, bufs = b.finish()
    w = nat.Weights(ctx, pack.blob() or b"\0" * 256)
    net = nat.Net(ctx, w, ops, bufs, 0, 0, 0, 1)
    try:
        for k, v in (ups or {}).items():
            net.upload(k, v)
        launches = ctx.stats().launches
        with pytest.raises(ValueError, match=match):
            net.run_ops(0, len(ops), 1)
        assert ctx.stats().launches == launches, "a kernel was launched for a refused plan"
        if keep:
            after = net.download(*keep)
            assert np.array_equal(after.view(np.uint8), np.ascontiguousarray(ups[keep[0]]).view(np.uint8)), "a refused op wrote to its destination"
    finally:
        net.close()
        w.close()


def test_channel_counts_the_kernels_cannot_run_are_refused(ctx):
    """layernorm_c_kernel holds four 8-channel chunks per lane of 64 (C <= 2048), proj2_kernel eight channels per lane (C <= 512): C = 2056 and C = 520
    are refused by the host checks, and the destinations keep their sentinel"""
    from vsdeoldify_amd.plan import PlanBuilder, View, WeightPack
    pack, b = WeightPack(), PlanBuilder()
    xv, yv = View(b.buf(9 * 2056), 0, 2056, 1, 9, 2056, 2056), View(b.buf(9 * 2056), 0, 2056, 1, 9, 2056, 2056)
    b.layernorm("ln", xv, yv, pack.add(np.ones(2056, F)), pack.add(np.zeros(2056, F)), 1e-6)
    dst = np.full((1, 9, 2056), U.SENTINEL, np.float16)
    _refused(ctx, pack, b, r"layernorm op: 1 <= C <= 2048", {xv.buf: np.ones((1, 9, 2056), np.float16), yv.buf: dst}, (yv.buf, dst.shape, np.float16))
    pack, b = WeightPack(), PlanBuilder()
    xv = View(b.buf(5 * 520), 0, 520, 1, 5, 520, 520)
    out = b.buf(10, 4)
    b.proj2("proj", xv, pack.add(np.ones((2, 520), F)), -1, 1, 1.0, out)
    dst = np.full((1, 5, 2), -777.0, F)
    _refused(ctx, pack, b, r"proj2 op: weights, 1 <= C <= 512", {xv.buf: np.ones((1, 5, 520), np.float16), out: dst}, (out, dst.shape, F))


# ---- frames of views that do not fill their buffers' frames ------------------------------------------------------------------------------------------------------------------
B3 = 3
KINDS = [("layernorm", False), ("layernorm", True), ("dwconv7", False), ("dwconv7", True), ("dwconv7_ln", False), ("dwconv7_ln", True), ("pixshuf4_blur", False),
         ("subsample2", False), ("subsample2", True), ("proj2", False), ("proj2", True), ("shuf4_blur_ab", False)]


def _frames_plan(kind, precise, extra):
    """one op of `kind` on views of buffers that hold `extra` more rows per frame (1 = the token-buffer shape) -> (builder, pack,
    {buffer: (rows, row elements, dtype)} of the uploads, the destination buffers).  Precise plans: pair tensors of twice the pitch."""
    from vsdeoldify_amd.plan import PlanBuilder, View, WeightPack
    pack, b = WeightPack(), PlanBuilder(precise=precise)
    pm = b.pm
    r = np.random.default_rng(4)
    ups = {}

    def view(H, W, C, coff=8, pad=64):
        rows, pitch = H * W + extra, (C + pad) * pm
        v = View(b.buf(rows * pitch), coff, pitch, H, W, C, U.pad_to(C, 8))
        ups[v.buf] = (rows, pitch, np.float16)
        return v

    def raw(rows, width):
        buf = b.buf((rows + extra) * width, 4)
        ups[buf] = (rows + extra, width, F)
        return buf
    vec = lambda n, s=1.0, o=0.0: pack.add((o + s * r.standard_normal(n)).astype(F))          # noqa: E731
    H, W = 5, 7
    if kind == "layernorm":
        xv, yv = view(H, W, 64), view(H, W, 64, 16)
        b.layernorm("op", xv, yv, vec(64, 0.2, 1.0), vec(64), 1e-6, relu=True)
        dsts = [yv.buf]
    elif kind in ("dwconv7", "dwconv7_ln"):
        C = 192 if kind == "dwconv7_ln" else 64
        xv, yv = view(H, W, C), view(H, W, C, 16)
        w_off = pack.add((r.standard_normal((49, C)) / 7).astype(F if precise else np.float16))
        if kind == "dwconv7":
            b.dwconv7("op", xv, yv, w_off, vec(C, 0.1), C)
        else:
            b.dwconv7_ln("op", xv, yv, w_off, vec(C, 0.1), C, vec(C, 0.2, 1.0), vec(C, 0.1), 1e-6)
        dsts = [yv.buf]
    elif kind == "pixshuf4_blur":
        xv, yv = view(2, 3, 16 * 8), view(8, 12, 8, 16)
        b.pixshuf4_blur("op", xv, yv)
        dsts = [yv.buf]
    elif kind == "subsample2":
        xv, yv = view(H, W, 64), view(3, 4, 64, 16)
        b.subsample2("op", xv, yv)
        dsts = [yv.buf]
    elif kind == "proj2":
        xv, out = view(H, W, 64), raw(H * W, 2)
        b.proj2("op", xv, pack.add(r.standard_normal((2, 64)).astype(F)), vec(2), 2, 110.0, out)
        dsts = [out]
    else:
        pb = raw(2 * 3, 32)
        iv, yv = view(8, 12, 3, 8, 21), view(8, 12, 2, 16, 22)                   # 24-pitch rows: the image at offset 8, the ab chunk at offset 16
        b.shuf4_blur_ab("op", pb, 2, 3, iv, pack.add(r.standard_normal((2, 3)).astype(F)), vec(2), yv)
        dsts = [yv.buf]
    return b, pack, ups, dsts


@pytest.mark.parametrize("kind,precise", KINDS)
def test_a_batch_on_views_that_do_not_fill_their_frames_runs_frame_by_frame(ctx, kind, precise):
    """B = 3 on buffers of h x w + 1 rows per frame, the op on their h x w views: the extra row of every frame keeps its sentinel and the views hold, bit for
    bit, what the dense run of the same frames gives.  (As one launch with frame b at b x h x w x pitch, frame 1 began on frame 0's extra row.)  The
    dense run is ONE launch, as it always was (the benchmark's plans are dense); the other one launch per frame.  mha and fold_queries carry explicit
    token strides instead: test_attention_result_does_not_depend_on_the_batch, test_fold_queries_is_within_its_fp32_bound."""
    from tests.gpu_util import run_plan
    got, before = {}, {}
    for extra in (0, 1):
        b, pack, ups, dsts = _frames_plan(kind, precise, extra)
        arrays = {}
        r = np.random.default_rng(23)                                           # the same frames in both runs; the destinations start with random values too
        for buf, (rows, width, dt) in ups.items():
            n = rows - extra
            a = np.empty((B3, rows, width), dt)
            a[:, :n] = r.standard_normal((B3, n, width)).astype(dt)
            if extra:
                a[:, n:] = -777.0
            arrays[buf] = a
        launches = ctx.stats().launches
        out = run_plan(ctx, pack, b, arrays, {d: (arrays[d].shape, arrays[d].dtype) for d in dsts}, B3)
        assert ctx.stats().launches - launches == (B3 if extra else 1), "launches of the op"
        got[extra], before[extra] = [out[d] for d in dsts], [arrays[d] for d in dsts]
        if extra:
            for d in dsts:
                assert (out[d][:, -1] == -777.0).all(), "the extra row of a frame was written"
    for dense, token, was in zip(got[0], got[1], before[0]):
        raw = lambda a: np.ascontiguousarray(a).view(np.uint8)                  # noqa: E731
        assert (raw(dense) != raw(was)).reshape(B3, -1).any(axis=1).all(), "the dense run left a frame as it was"
        same = raw(dense) == raw(token[:, :dense.shape[1]])
        assert same.all(), f"{kind}: {int((~same).sum())} of {same.size} bytes differ from the dense run; first (frame, row, byte): {np.argwhere(~same)[:5].tolist()}"
