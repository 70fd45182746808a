"""GPU: the 14 ColorMNet network kernels of csrc/colormnet_net.hip (ew, dwconv and its 3 x 3 strip form, chan_gram + chan_softmax and the conv that
applies their matrix, mha64, the four cbam kernels, gru, planar_in, planar_out, cmn_decoder_in) one op at a time against plain float64 -- each through a
one-op plan whose views sit at channel offsets of wider rows and whose destination starts as a sentinel (tests/colormnet_ops_util.py: the cases, the
inputs, the oracles, the rules and their derivations; tests/test_colormnet_ops_host.py shows on the CPU that the rules hold for the kernels' own order and
fail for wrong kernels).  The cases reach what the product plan launches and the six first op tests (tests/test_colormnet_net.py) do not: Gram tiles past
the first and a ragged last one, pixel splits and their staging chunks, c = 256, frames of their own data in every scratch buffer, live < tokens per frame,
every chunking of the cbam MLP, the strip tails of the 3 x 3 depthwise kernel.

HAVC_COLORMNET_OPS_OUT=<file> writes every measured figure and the time of every item (profiles/colormnet_ops.txt)."""
import os
import time

import numpy as np
import pytest

from tests import colormnet_ops_util as U

pytestmark = pytest.mark.gpu
REPORT, TIMES, RATIOS = [], [], {}
F = np.float32


def note(op, ratio, where, line, got=None, ref=None):
    """one line of the profile: the figure, the worst element's index, the GPU's value there and the float64 reference"""
    RATIOS[op] = max(RATIOS.get(op, 0.0), float(ratio))
    vals = f" (GPU {float(np.asarray(got)[where]):.9g}, float64 {float(np.asarray(ref)[where]):.9g})" if got is not None else ""
    REPORT.append(f"{line}: max |err| / bound {ratio:.4f} at {where}{vals}")
    print(REPORT[-1])


@pytest.fixture(scope="module", autouse=True)
def _profile():
    yield
    out = os.environ.get("HAVC_COLORMNET_OPS_OUT")
    if out and REPORT:
        over = sorted(k for k, v in RATIOS.items() if v > 1.0)
        with open(out, "w") as f:
            f.write("The ColorMNet network kernels (csrc/colormnet_net.hip) op by op against float64 on the MI355X\n"
                    "(tests/test_gpu_colormnet_ops.py; the rules and their derivations: tests/colormnet_ops_util.py).  Every figure is max |GPU - ref| / bound,\n"
                    f"the limit is {U.LIMIT} and a figure above 1.0 asks for an explanation.  Ops above 1.0 in this run: {', '.join(over) if over else 'none'}.\n"
                    "Copies, roundings, x^2 + 1 and the depthwise kernels against the same-order fp32 sum are bit-exact and have no figure.\n\n"
                    "largest figure per op\n" + "\n".join(f"{v:8.4f}  {k}" for k, v in sorted(RATIOS.items())) + "\n\n")
            f.write("\n".join(REPORT) + "\n\nseconds per item (host wall clock, inputs and reference included)\n" + "\n".join(TIMES) + "\n")


@pytest.fixture(autouse=True)
def _timed(request):
    t0 = time.perf_counter()
    yield
    TIMES.append(f"{time.perf_counter() - t0:7.3f}  {request.node.name}")


def _same(a, b, what):
    same = U.bits(a) == U.bits(b) if np.asarray(a).dtype == np.float16 else np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)
    assert same.all(), f"{what}: {int((~same).sum())} of {same.size} differ; first at {np.argwhere(~same)[:5].tolist()}"


def _held(op, line, got, ref, bound, half=True):
    fig, where = U.figure(got, ref, bound, half)
    note(op, fig, where, line, got, ref)
    assert fig <= U.LIMIT, (line, fig, where, np.asarray(got)[where], ref[where])


# ---- cross-channel attention ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", U.CCA_REGIMES)
@pytest.mark.parametrize("name", list(U.CCA_CASES))
def test_chan_attn_matrix_and_its_application(ctx, name, regime):
    case = U.CCA_CASES[name]
    q, k, v, temp = U.cca_inputs(case, regime)
    Wref, _ = U.cca_reference(q, k, temp, case.heads)
    bw = U.cca_bound(Wref, temp, case.per, case.S)
    Wfull, ofull = U.run_cca(ctx, case, q, k, v, temp)
    blocks = U.cca_blocks(Wfull, case.heads, case.c)
    tag = f"{name:5s} heads {case.heads} c {case.c:3d} P {case.P:4d} B {case.B} tiles {case.tiles} S {case.S} per {case.per:3d} {regime:5s}"
    _held("chan_attn", "chan_attn " + tag, blocks, Wref, bw)
    assert U.cca_matrix_untouched(Wfull, case), "off-diagonal blocks are not +0, or rows / columns past the matrix were written"
    if case.zero:                                                  # the eps path: an all-zero q channel gives a uniform row, 1 / c
        _same(blocks[:, 0, 3], np.full((case.B, case.c), 1.0 / case.c, np.float16), "the row of the all-zero q channel")
    if case.conv:
        lay = U.cca_layout(case)
        got = ofull[..., lay["o_coff"]:lay["o_coff"] + case.C2]
        ref, mag, extra = U.cca_apply_f64(Wref, v, bw)
        _held("attn@v vs float64 W", "attn@v vs float64 W " + tag, got, ref, U.ulp16(ref) / 2 + case.C2 * U.U32 * mag + extra)
        ref, mag, _ = U.cca_apply_f64(blocks, v)
        _held("attn@v vs own W", "attn@v vs own W     " + tag, got, ref, U.ulp16(ref) / 2 + case.C2 * U.U32 * mag)
        assert U.outside_is_sentinel(ofull, lay["o_coff"], case.C2)
    else:
        assert ofull is None


# ---- mha64 ------------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(U.MHA_CASES))
def test_mha64_is_within_the_attention_rule(ctx, name):
    case = U.MHA_CASES[name]
    for regime in case.regimes:
        q, k, v = U.mha64_inputs(case, regime)
        ref = U.mha64_reference(q, k, v, case.heads, U.mha64_targets(case, regime, k) if regime in ("sharp", "edges") else None)
        U.mha64_check_regime(case, regime, ref)
        got, full = U.run_mha64(ctx, case, q, k, v)
        ratio, worst = U.attn_ratio(got, ref["out"], ref["A"], 1.0)
        note("mha64", ratio, tuple(int(i) for i in worst), f"mha64 {name:8s} heads {case.heads} L {case.L:3d} B {case.B} {case.layout:5s} {regime:6s}", got, ref["out"])
        assert np.isfinite(got.astype(F)).all() and ratio <= U.LIMIT, (name, regime, ratio, worst)
        assert U.mha64_untouched(full, case), "rows past the live tokens or channels outside the view were written"


# ---- ew ------------------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", U.EW_CHANNELS)
@pytest.mark.parametrize("name", list(U.EW_CASES))
def test_ew_modes_and_flags(ctx, name, C):
    case = U.EW_CASES[name]
    for kind in ("random", "patterns"):
        x, res = U.ew_inputs(case, C, kind)
        y, full, y2, full2 = U.run_ew(ctx, case, x, res)
        assert U.outside_is_sentinel(full, 16, C) and (full2 is None or U.outside_is_sentinel(full2, 24, C))
        if case.exact:
            want = np.broadcast_to(x[:1], x.shape) if case.src_bcast else x
            _same(y, U.relu16(want) if case.relu else want, f"{name} C {C} {kind}")
            if case.dual:
                _same(y2, U.relu16(want), f"{name} C {C} {kind}: the rectified twin")
            continue
        best, shown = None, None
        for how in (("fma", "mul_add") if case.mode == 1 else ("fma",)):
            ref, bound = U.ew_f64(case, x, res, how)
            figs = [U.figure(y, np.maximum(ref, 0) if case.relu else ref, bound)]
            if case.dual:
                figs.append(U.figure(y2, np.maximum(ref, 0), bound))
            fig = max(figs)
            if best is None or fig + (how,) < best:
                best, shown = fig + (how,), (y2 if case.dual and figs[-1] == fig else y, np.maximum(ref, 0) if case.relu or (case.dual and figs[-1] == fig) else ref)
        note(f"ew {'bilinear' if case.mode == 1 else 'area' if case.mode == 2 else 'copy + residual'}", best[0], best[1],
             f"ew {name:20s} C {C:2d} {kind:8s}" + (f" (source coordinate: {best[2]})" if case.mode == 1 else ""), *shown)
        assert best[0] <= U.LIMIT, (name, C, kind, best)
        if case.dual:
            _same(y2, U.relu16(y), f"{name}: the twin is the rectified first output")


# ---- dwconv ---------------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", U.DW_CHANNELS)
@pytest.mark.parametrize("K", [3, 5])
def test_dwconv_strip_and_per_pixel(ctx, K, C):
    assert U.dw_kernel(K) == ("dwconv3_strip_kernel" if K == 3 else "dwconv_kernel<5>")
    w, bias = U.dw_params(C, K)
    for H, W in (U.DW_SHAPES if K == 3 else U.DW5_SHAPES):
        for kind in ("random", "patterns") if (H, W) in ((9, 5), (17, 9), (9, 11), (2, 3)) else ("random",):
            x = U.dw_inputs(H, W, C, kind)
            for bb in (bias, None):
                got, full = U.run_dwconv(ctx, x, w, bb)
                assert U.outside_is_sentinel(full, 16, C)
                _same(got, U.dw_emulate(x, w, bb), f"dwconv K {K} {H} x {W} C {C} {kind} bias {int(bb is not None)} against the same-order fp32 sum")
                if kind == "random":
                    ref, mag = U.dwconv_f64(x, w, bb)
                    _held(f"dwconv K {K}", f"dwconv K {K} {H:2d} x {W:2d} C {C:2d} bias {int(bb is not None)}", got, ref, U.dw_bound(ref, mag, K))


# ---- cbam -------------------------------------------------------------------------------------------------------------------------------------------------------------------------
def _cbam(ctx, C, H, W, dual):
    x, params = U.cbam_inputs(C, H, W), U.cbam_params(C)
    ref, bound = U.cbam_f64(x, params)
    y, full, y2, full2 = U.run_cbam(ctx, x, params, dual)
    NCH, clen = U.cbam_choice(C)
    _held("cbam", f"cbam C {C:4d} (Ch {C // 16:2d}, NCH {NCH:2d}, clen {clen:3d}) {H} x {W} B {U.CBAM_B} dual {int(dual)}", y, ref, bound)
    assert U.outside_is_sentinel(full, 16, C)
    if dual:
        _same(y2, U.relu16(y), "the rectified twin")
        assert U.outside_is_sentinel(full2, 24, C)


@pytest.mark.parametrize("C", U.CBAM_CHANNELS)
def test_cbam_every_mlp_chunking(ctx, C):
    assert U.cbam_choice(C) == U.CBAM_CHOICE[C], "cbam_mlp_kernel's chunking is no longer what this channel count is listed for"
    for H, W in U.CBAM_GRIDS:
        for dual in (False, True):
            _cbam(ctx, C, H, W, dual)


def test_cbam_pool_tail_for_every_pixel_count(ctx):
    for P in U.CBAM_TAIL_P:
        _cbam(ctx, 64, 1, P, False)


# ---- gru, planar in / out, decoder input -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hd", [8, 16])
def test_gru(ctx, hd):
    B, P = 2, 77
    vals = U.act_inputs((B, P, 3 * hd), [61, hd])
    h = (0.5 * np.random.default_rng(hd).standard_normal((B, hd, P))).astype(F)
    h.reshape(-1)[::13] = np.resize(np.array([0.0, -0.0, 1e4, -3.0], F), len(h.reshape(-1)[::13]))
    got = U.run_gru(ctx, vals, h, hd)
    ref, bound = U.gru_f64(vals, h, hd)
    assert np.isfinite(got).all()
    _held("gru", f"gru hd {hd:2d} P {P} B {B}", got, ref, bound, half=False)


@pytest.mark.parametrize("C,span", [(3, 8), (3, 16), (5, 8), (16, 16)])
def test_planar_in_is_one_rounding(ctx, C, span):
    B, P = 2, 45
    for pixel_major in (False, True):
        for bcast in (False, True):
            src = U.planar_values((B, P, C) if pixel_major else (B, C, P), [67, C, span])
            full = U.run_planar_in(ctx, src, P, C, span, pixel_major, bcast, B)
            want = np.zeros((B, P, span), np.float16)
            s = np.broadcast_to(src[:1], src.shape) if bcast else src
            want[..., :C] = U.to_half(s if pixel_major else s.transpose(0, 2, 1))
            _same(full[..., 16:16 + span], want, f"planar_in C {C} span {span} pixel_major {pixel_major} bcast {bcast}")
            assert U.outside_is_sentinel(full, 16, span)


@pytest.mark.parametrize("C", [1, 5, 64])
def test_planar_out_every_activation(ctx, C):
    B, P = 2, 45
    x = U.act_inputs((B, P, C), [71, C])
    for act in range(4):
        got = U.run_planar_out(ctx, x, act)
        ref, bound = U.planar_out_f64(x, act)
        if bound is None:
            with np.errstate(over="ignore"):
                _same(got, ref.astype(F), f"planar_out C {C} act {act}")
        else:
            assert np.isfinite(got).all()
            _held(f"planar_out act {act}", f"planar_out C {C:2d} act {act}", got, ref, bound, half=False)


def test_decoder_input_is_copies_and_roundings(ctx):
    B, P, Cg, CV, HD = 2, 35, 32, 24, 8
    g = U.special_halves((1, P, Cg), 73)
    ro, hid = U.planar_values((B, CV, P), 74), U.planar_values((B, HD, P), 75)
    dc, dcr = U.run_decoder_in(ctx, g, ro, hid)
    span = Cg + CV + HD
    want = np.concatenate([np.broadcast_to(g, (B, P, Cg)), U.to_half(ro.transpose(0, 2, 1)), U.to_half(hid.transpose(0, 2, 1))], -1)
    _same(dc[..., 16:16 + span], want, "decoder input")
    _same(dcr[..., 16:16 + span], U.relu16(want), "decoder input, rectified")
    assert U.outside_is_sentinel(dc, 16, span) and U.outside_is_sentinel(dcr, 16, span)
