"""CPU: that the oracles of tests/ddcolor_ops_util.py are the operations they are named for (torch.nn.functional in float64), that a numpy emulation of
each kernel's arithmetic stays inside its rule on every case, and that the rules can fail: wrong kernels, written as mutations of the oracle or of the
emulation, exceed them.  For the attention this file also records why the `edges` regime exists: a key dropped or weighed twice at a 256-key chunk
boundary exceeds the limit there and hides behind sharp scores."""
import numpy as np
import pytest

from tests import ddcolor_ops_util as U

F = np.float32


# ---- the cases select the paths they are named for ----------------------------------------------------------------------------------------------------------
def test_the_case_list_selects_every_launcher_choice():
    for name, c in U.MHA_CASES.items():
        assert U.launcher_choice(c.B, c.heads, c.Lk) == (c.nch, c.nsplit), name
    split = [c for c in U.MHA_CASES.values() if c.kernel == "split"]
    assert {c.Lk for c in split if c.name.startswith("k")} == set(U.LK_SWEEP) and {c.Lq for c in split if c.name.startswith("q")} == set(U.LQ_SWEEP)
    assert all(c.Lq <= 128 for c in split) and {c.Lq for c in U.MHA_CASES.values() if c.kernel == "plain" and c.name.startswith("q")} == {129, 200}
    assert {(c.nch, c.nsplit) for c in split if c.name in U.MANY_KEYS} == {(2, 9), (4, 5), (4, 1)}
    c = U.MHA_CASES["nch2"]                                        # the ragged last block: split 8 of 9 starts at chunk 16 of 17, its second chunk starts past Lk
    assert (c.nsplit - 1) * c.nch * 256 < c.Lk <= ((c.nsplit - 1) * c.nch + 1) * 256
    assert U.edge_keys(1) == [0] and U.edge_keys(257) == [0, 255, 256] and U.edge_keys(513) == [0, 255, 256, 511, 512] and U.edge_keys(256) == [0, 255]
    assert U.edge_keys(4097)[-3:] == [3840, 4095, 4096] and len(U.edge_keys(4097)) == 33 and U.edge_keys(1024) == [0, 255, 256, 511, 512, 767, 768, 1023]
    k2, _ = U.mha_kv(U.MHA_CASES["nch2"])
    k4, _ = U.mha_kv(U.MHA_CASES["nch4"])
    assert np.shares_memory(k2, k4) and np.array_equal(U.bits(k2), U.bits(k4[:16]))          # the nch = 2 case is the first 16 frames of the nch = 4 one
    # LayerNorm: every LP on both sides of each threshold, one C that is no multiple of 8, one pixel count per LP beyond one sweep of the capped grid
    assert {C: U.ln_lanes(C) for C in U.LN_CHANNELS} == U.LN_LP and sorted(set(U.LN_LP.values())) == [8, 16, 32, 64]
    assert [U.ln_lanes(C) for C in (256, 264, 512, 520, 1024, 1032)] == [8, 16, 16, 32, 32, 64] and any(C % 8 for C in U.LN_CHANNELS)
    for LP, C, npix in U.LN_SWEEPS:
        assert U.ln_lanes(C) == LP and U.ln_grid(npix, LP) == 1024 and npix == 1024 * 4 * (64 // LP) + 3
    assert U.ln_grid(1, 8) == 1 and U.ln_grid(257, 64) == 65 and U.ln_grid(32768, 8) == 1024
    assert U.ln_k(2048) == (39.0, 27.5) and U.ln_k(8) == (12.0, 14.0)


# ---- attention ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_attention_oracle_equals_torch_and_a_naive_loop():
    import math

    import torch
    case = U.MHA_CASES["q17"]
    q, k, v = U.mha_inputs(case, "sharp")
    ref = U.mha_reference(q, k, v, case.heads, cols=[0, 256])
    t = [torch.from_numpy(a.astype(np.float64).reshape(a.shape[0], a.shape[1], case.heads, 32).transpose(0, 2, 1, 3)) for a in (q, k, v)]
    want = torch.nn.functional.scaled_dot_product_attention(t[0], t[1], t[2], scale=float(U.SCALE)).numpy().transpose(0, 2, 1, 3).reshape(ref["out"].shape)
    assert np.allclose(ref["out"], want, rtol=1e-11, atol=1e-12)
    b, h = 2, 1
    for i in (0, 16):
        s = [float(U.SCALE) * sum(float(a) * float(c) for a, c in zip(q[b, i, h * 32:h * 32 + 32], kk[h * 32:h * 32 + 32])) for kk in k[b]]
        w = [math.exp(x - max(s)) for x in s]
        z = sum(w)
        o = sum((wi / z) * vv[h * 32:h * 32 + 32].astype(np.float64) for wi, vv in zip(w, v[b]))
        a = sum((wi / z) * np.abs(vv[h * 32:h * 32 + 32].astype(np.float64)) for wi, vv in zip(w, v[b]))
        assert np.allclose(o, ref["out"][b, i, h * 32:h * 32 + 32], rtol=1e-12, atol=1e-13) and np.allclose(a, ref["A"][b, i, h * 32:h * 32 + 32], rtol=1e-12)
        assert np.isclose(ref["pcols"][b, h, i, 1], w[256] / z, rtol=1e-12) and np.isclose(ref["pmax"][b, h, i], max(w) / z, rtol=1e-12)


@pytest.mark.parametrize("name", list(U.MHA_CASES))
def test_an_emulation_of_the_attention_kernels_stays_inside_the_bound(name):
    """256-key chunks, nch chunks per block, fp16 P into the second product, fp32 running sums, the merge, one fp16 store (split); one online softmax per
    lane in fp32, merged (plain): at or below 1.0 x bound in every regime of every case"""
    case = U.MHA_CASES[name]
    for regime in U.REGIMES:
        q, k, v = U.mha_inputs(case, regime)
        ref = U.mha_reference(q, k, v, case.heads, tgt=U.mha_targets(case, regime, k) if regime != "flat" else None)
        U.check_regime(case, regime, ref)
        ratio, worst = U.mha_ratio((U.emulate_split if case.kernel == "split" else U.emulate_plain)(case, q, k, v), ref)
        print(f"{name:14s} {regime:6s} emulation: max err / bound {ratio:.3f}")
        assert ratio <= 1.0, U.mha_worst_text(case, worst, ratio)


@pytest.mark.parametrize("name", U.MANY_KEYS)
def test_a_key_lost_or_doubled_at_a_chunk_edge_shows_in_edges_and_hides_in_sharp(name):
    """two wrong kernels as exact mutations of the reference: one that drops a key of the edge set (any one of them), one that weighs a phantom key at
    index Lk (an unmasked lane: the clamped K row of the last key, a zero V column).  With `edges` queries every one of them exceeds the limit in some
    output; with `sharp` queries -- and this is the recorded fact the regime answers -- none does; `flat` is printed for the record."""
    case = U.MHA_CASES[name]
    edges = U.edge_keys(case.Lk)
    for regime in ("edges", "sharp", "flat"):
        q, k, v = U.mha_inputs(case, regime)
        ref = U.mha_reference(q, k, v, case.heads, cols=edges)
        ratios = [U.mha_ratio(U.without_key(ref, v, case.heads, col, key), ref)[0] for col, key in enumerate(edges)]
        phantom = U.mha_ratio(U.with_phantom_key(ref, case.heads, len(edges) - 1), ref)[0]
        print(f"{name} {regime:6s}: a dropped edge key gives {min(ratios):.3g} .. {max(ratios):.3g} x bound, a phantom key {phantom:.3g} (limit {U.LIMIT})")
        if regime == "edges":
            assert min(ratios) > U.LIMIT and phantom > U.LIMIT, (min(ratios), phantom)
        elif regime == "sharp":
            assert max(ratios) <= U.LIMIT and phantom <= U.LIMIT, (max(ratios), phantom)


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_layernorm_oracle_equals_torch():
    import torch
    for C in (20, 264):
        x = U.ln_inputs("random", 9, C)
        g, b = U.ln_params(C)
        for relu in (False, True):
            ref, pre, mabs, rstd = U.ln_f64(x, g, b, 1e-5, relu)
            want = torch.nn.functional.layer_norm(torch.from_numpy(x.astype(np.float64)), (C,), torch.from_numpy(g.astype(np.float64)),
                                                  torch.from_numpy(b.astype(np.float64)), float(F(1e-5)))
            assert np.allclose(ref, (torch.relu(want) if relu else want).numpy(), rtol=1e-12, atol=1e-13)
            assert np.allclose(mabs[:, 0], np.abs(x.astype(np.float64)).mean(-1)) and np.allclose(rstd[:, 0] ** -2, x.astype(np.float64).var(-1) + float(F(1e-5)))


@pytest.mark.parametrize("C", U.LN_CHANNELS)
def test_layernorm_rule_passes_float32_in_two_summation_orders_and_fails_wrong_kernels(C):
    g, b = U.ln_params(C)
    for kind in ("random", "offset", "special"):
        x = U.ln_inputs(kind, 9, C)
        for eps in U.LN_EPS:
            for relu in (False, True):
                # (the +-60000 pixel of `special` is left to the kernel's own order: C equal squares added left to right drift the same way at every step,
                # by more than the 8 ceil(C8 / LP) + log2 LP roundings the rule counts -- 1.11 x at C = 1536)
                for order in ("lanes", "serial") if kind != "special" else ("lanes",):
                    e = U.ln_excess(U.ln_emulate(x, g, b, eps, relu, order), x, g, b, eps, relu)
                    print(f"layernorm C {C:4d} {kind:7s} eps {eps:g} relu {int(relu)} float32 {order:6s}: max excess {e.max():.3f}")
                    assert e.max() <= 1.0, (kind, eps, relu, order, float(e.max()), np.unravel_index(int(e.argmax()), e.shape))
        if kind == "special":
            got = U.ln_emulate(x, g, b, 1e-6, False, "lanes")
            assert np.array_equal(U.bits(got[4]), U.bits(b.astype(np.float16))) and np.isfinite(got[-1].astype(F)).all()
    if C < 16:
        return                                                     # the mutations below need more than a handful of channels to show
    x = U.ln_inputs("random", 9, C)
    x64 = x.astype(np.float64)
    ref, _, _, _ = U.ln_f64(x, g, b, 1e-6)
    d = x64 - x64.mean(-1, keepdims=True)
    wrong = {"unbiased variance": d / np.sqrt((d * d).sum(-1, keepdims=True) / (C - 1) + 1e-6) * g + b,
             "gamma and beta of the next chunk": U.ln_f64(x, np.roll(g, 8), np.roll(b, 8), 1e-6)[0],
             "the pad channel summed": U.ln_f64(np.concatenate([x64, np.full((9, 1), 0.5)], -1), np.append(g, F(1)), np.append(b, F(0)), 1e-6)[0][:, :C],
             "mean of the neighbouring pixel": (x64 - np.roll(x64.mean(-1, keepdims=True), 1, 0)) * U.ln_f64(x, g, b, 1e-6)[3] * g + b}
    for what, v in wrong.items():
        e = U.ln_excess(v.astype(np.float16), x, g, b, 1e-6)
        assert e.max() > 1.5, (what, float(e.max()))
    assert np.abs(ref).max() < 20


# ---- depthwise conv ----------------------------------------------------------------------------------------------------------------------------------------------
def test_dwconv7_oracle_equals_torch_and_the_rule_can_fail():
    import torch
    for (H, W), C in (((13, 10), 8), ((3, 7), 24), ((1, 1), 8)):
        w, bias, g, be = U.dw_params(C)
        x = U.f16(np.random.default_rng([H, W, C]).standard_normal((2, H, W, C)))
        ref, mag = U.dwconv7_f64(x, w, bias)
        xt = torch.from_numpy(x.astype(np.float64)).permute(0, 3, 1, 2)
        wt = torch.from_numpy(w.astype(np.float64))[:, None]
        want = torch.nn.functional.conv2d(xt, wt, torch.from_numpy(bias.astype(np.float64)), padding=3, groups=C)
        assert np.allclose(ref, want.permute(0, 2, 3, 1).numpy(), rtol=1e-12, atol=1e-13)
        assert np.allclose(mag, torch.nn.functional.conv2d(xt.abs(), wt.abs(), None, padding=3, groups=C).permute(0, 2, 3, 1).numpy(), rtol=1e-12)
        # the kernel's float32 chain (bias first, taps in row order) passes, with fma or without
        xp = np.zeros((2, H + 6, W + 6, C), F)
        xp[:, 3:3 + H, 3:3 + W] = x
        acc = np.broadcast_to(bias, (2, H, W, C)).astype(F)
        for dy in range(7):
            for dx in range(7):
                acc = acc + xp[:, dy:dy + H, dx:dx + W] * w[:, dy, dx]
        assert U.dw_excess(acc.astype(np.float16), ref, mag).max() <= 1.0
        if H > 1:
            flipped, _ = U.dwconv7_f64(x, w[:, ::-1, ::-1], bias)
            transposed, _ = U.dwconv7_f64(x, w.transpose(0, 2, 1), bias)
            assert U.dw_excess(flipped.astype(np.float16), ref, mag).max() > 100 and U.dw_excess(transposed.astype(np.float16), ref, mag).max() > 100
    # dwconv7 + LayerNorm: the composed oracle is torch's composition
    C = 64
    w, bias, g, be = U.dw_params(C)
    x = U.f16(np.random.default_rng(3).standard_normal((1, 3, 2, C)))
    conv, _ = U.dwconv7_f64(x, w, bias)
    want = torch.nn.functional.layer_norm(torch.from_numpy(conv), (C,), torch.from_numpy(g.astype(np.float64)), torch.from_numpy(be.astype(np.float64)), float(F(1e-6)))
    assert np.allclose(U.ln_f64(conv, g, be, 1e-6)[0], want.numpy(), rtol=1e-12, atol=1e-13)
    assert U.ln_excess(want.numpy().astype(F).astype(np.float16), conv, g, be, 1e-6).max() <= 1.0


# ---- PixelShuffle(4) + blur ----------------------------------------------------------------------------------------------------------------------------------------
def test_pixshuf4_blur_oracle_equals_torch_and_where_the_double_rounding_is():
    import torch
    import torch.nn.functional as TF
    r = np.random.default_rng(4)
    for Hi, Wi in U.PS_SHAPES:
        C = 8
        x = r.standard_normal((2, Hi, Wi, 16 * C))
        # torch's pixel_shuffle takes channel c 16 + (dy 4 + dx); the kernel's rows are (dy 4 + dx) C + c
        xt = torch.from_numpy(x.reshape(2, Hi, Wi, 16, C).transpose(0, 4, 3, 1, 2).reshape(2, 16 * C, Hi, Wi).copy())
        want = TF.avg_pool2d(torch.nn.ReplicationPad2d((1, 0, 1, 0))(TF.pixel_shuffle(xt, 4)), 2, stride=1).numpy().transpose(0, 2, 3, 1)
        got, mag = U.pixshuf4_blur_f64(x)
        assert got.shape == (2, 4 * Hi, 4 * Wi, C) and np.allclose(got, want, rtol=0, atol=1e-15) and (mag >= np.abs(got) - 1e-15).all()
    # on blur_inputs the kernel's float32 steps are exact, on the marks too: one rounding
    for x in (U.blur_inputs((2, 2, 3, 128), 1), U.ps_marks(2, 2, 3, 24)):
        up = U.pixshuf4_f64(x).astype(F)
        s32 = (((up[:, :-1, :-1] + up[:, :-1, 1:]) + up[:, 1:, :-1]) + up[:, 1:, 1:]) * F(0.25)
        assert np.array_equal(s32.astype(np.float64), U.pixshuf4_blur_f64(x)[0][:, 1:, 1:])
    m = U.ps_marks(1, 1, 1, 8)[0, 0, 0].astype(np.float64).reshape(16, 8)
    assert len(np.unique(m)) == 128 and (np.diff(m, axis=0) == 1).all()
    # ... and on arbitrary fp16 values they are not: the input named in the util's docstring
    v = np.array([4096.0, 2.0, 2.0 ** -14, 0.0], np.float16)
    assert (v.astype(np.float64) == [4096.0, 2.0, 2.0 ** -14, 0.0]).all()
    f32 = (((v[0].astype(F) + v[1].astype(F)) + v[2].astype(F)) + v[3].astype(F)) * F(0.25)
    assert np.float16(f32) == 1024.0 and np.float16(v.astype(np.float64).sum() / 4) == 1025.0
    p = U.ps_patterns((2, 2, 3, 16 * 24), 5)
    assert np.isfinite(p).all() and {0x0000, 0x8000, 0x0001, 0x7BFF, 0xFBFF} <= set(U.bits(p).reshape(-1).tolist())
    up = U.pixshuf4_f64(p).astype(F)
    y0, x0 = np.maximum(np.arange(8) - 1, 0), np.maximum(np.arange(12) - 1, 0)
    s32 = (((up[:, y0][:, :, x0] + up[:, y0]) + up[:, :, x0]) + up) * F(0.25)
    ref, mag = U.pixshuf4_blur_f64(p)
    assert (np.abs(s32.astype(np.float16).astype(np.float64) - ref) <= U.ulp16(ref) / 2 + 4 * U.U32 * mag).all()


# ---- Zhang ops -------------------------------------------------------------------------------------------------------------------------------------------------------
def test_bilinear_indices_from_the_float32_scale_equal_the_float64_ones_and_the_oracle_is_torch():
    import torch
    for (Hi, Wi), (Ho, Wo) in U.BILINEAR_SIZES:
        for n_in, n_out in ((Hi, Ho), (Wi, Wo)):
            i64 = U.bilinear_src(n_in, n_out, "f64")
            true = np.maximum((np.arange(n_out) + 0.5) * (n_in / n_out) - 0.5, 0)                   # the float64 scale
            assert np.array_equal(i64[0], np.minimum(true.astype(np.int64), n_in - 1))
            for how in ("fma", "mul_add"):
                i0, i1, lam = U.bilinear_src(n_in, n_out, how)
                assert np.array_equal(i0, i64[0]) and np.array_equal(i1, i64[1]) and np.abs(lam - i64[2]).max() < 1e-5 and lam.dtype == F, (n_in, n_out, how)
        x = np.random.default_rng([Hi, Wi, Ho]).standard_normal((2, Hi, Wi, 2)).astype(F)
        want = torch.nn.functional.interpolate(torch.from_numpy(x.astype(np.float64)).permute(0, 3, 1, 2), (Ho, Wo), mode="bilinear", align_corners=False)
        want = want.permute(0, 2, 3, 1).numpy() * float(F(U.AB_MUL))
        # torch's scale is the float64 one: equal where in / out is a power of two, within the float32 scale's 2^-24 x coordinate x slope x 110 elsewhere
        exact = Ho % Hi == 0 and Wo % Wi == 0
        assert np.allclose(U.bilinear2_f64(x, Ho, Wo, U.AB_MUL, "f64")[0], want, rtol=0, atol=1e-10 if exact else 5e-3), (Hi, Wi, Ho, Wo)
        assert np.allclose(U.bilinear2_f64(x, Ho, Wo, U.AB_MUL, "fma")[0], want, rtol=0, atol=1e-2)
        # the kernel's float32 expression passes the rule; an oracle with the float64 coordinate would not serve where the scale is inexact
        y0, y1, ly = U.bilinear_src(Hi, Ho, "fma")
        x0, x1, lx = U.bilinear_src(Wi, Wo, "fma")
        ly, lx = ly[None, :, None, None], lx[None, None, :, None]
        hy, hx = F(1) - ly, F(1) - lx
        got = (hy * (hx * x[:, y0][:, :, x0] + lx * x[:, y0][:, :, x1]) + ly * (hx * x[:, y1][:, :, x0] + lx * x[:, y1][:, :, x1])) * F(U.AB_MUL)
        fig, how = U.bilinear_excess(got, x, Ho, Wo, U.AB_MUL)
        assert got.dtype == F and fig <= 1.0, (Hi, Wi, Ho, Wo, fig)
        if (Hi, Ho) == (64, 135):
            ref, taps = U.bilinear2_f64(x, Ho, Wo, U.AB_MUL, "f64")
            assert (np.abs(got - ref) / (8 * U.U32 * taps * U.AB_MUL)).max() > 1.0
    x = np.arange(2 * 16 * 16 * 2, dtype=F).reshape(2, 16, 16, 2)
    assert U.bilinear_excess(U.bilinear2_f64(x, 64, 64, 1.0)[0].astype(F)[:, :, ::-1], x, 64, 64, 1.0)[0] > 1e3


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_proj2_oracle_and_rule(mode):
    import torch
    for C in U.PROJ_CHANNELS:
        x, w, bias = U.proj_inputs(C, 5, mode)
        ref, bound = U.proj2_f64(x, w, bias, mode, U.AB_MUL)
        xt, wt = torch.from_numpy(x.astype(np.float64)), torch.from_numpy(w.astype(np.float64))
        a = (torch.softmax(xt, -1) if mode == 1 else xt) @ wt.T
        want = (torch.tanh(a + torch.from_numpy(bias.astype(np.float64))) if mode == 2 else a) * float(F(U.AB_MUL))
        assert np.allclose(ref, want.numpy(), rtol=1e-12, atol=1e-13)
        if mode == 1:
            assert x[0].astype(F).max() - x[0].astype(F).min() >= 60 and np.allclose(ref[-1], w.astype(np.float64).mean(-1) * float(F(U.AB_MUL)), rtol=1e-12)
        # the kernel's float32 arithmetic: lanes stride the channels, a butterfly over 64 lanes
        def wave(v):                                               # v [npix][C] float32 -> per-lane serial sums, then the tree
            pad = np.zeros((v.shape[0], U.pad_to(C, 64)), F)
            pad[:, :C] = v
            acc = np.zeros((v.shape[0], 64), F)
            for t in pad.reshape(v.shape[0], -1, 64).transpose(1, 0, 2):
                acc = acc + t
            while acc.shape[1] > 1:
                acc = acc[:, 0::2] + acc[:, 1::2]
            return acc[:, 0]
        xf = x.astype(F)
        den = F(1)
        if mode == 1:
            xf = np.exp(xf - xf.max(-1, keepdims=True))
            den = wave(xf)
        got = np.stack([wave(xf * w[0]) / den, wave(xf * w[1]) / den], -1)
        if mode == 2:
            got = np.tanh(got + bias)
        got = got * F(U.AB_MUL)
        e = np.abs(got.astype(np.float64) - ref) / bound
        print(f"proj2 mode {mode} C {C:3d} float32 emulation: max excess {e.max():.3f}")
        assert got.dtype == F and e.max() <= 1.0, (C, float(e.max()))
        assert (np.abs(U.proj2_f64(x, w[::-1], bias, mode, U.AB_MUL)[0] - ref) / bound).max() > 1e3          # the two outputs exchanged
        if mode == 1 and C > 8:                                    # a softmax that forgets the last channel
            assert (np.abs(U.proj2_f64(x[:, :-1], w[:, :-1], bias, mode, U.AB_MUL)[0] - ref) / bound).max() > 10


def test_fold_queries_and_shuf4_blur_ab_oracles_and_rules():
    r = np.random.default_rng(6)
    e = U.f16(r.standard_normal((2, 112, 24)))
    rq = r.standard_normal((2, 104)).astype(F)
    ref, mag = U.fold_f64(e, rq, 100)
    naive = np.array([[[sum(float(rq[o, q]) * float(e[b, q, c]) for q in range(100)) for c in range(24)] for o in range(2)] for b in range(2)])
    assert np.allclose(ref, naive, rtol=1e-12, atol=1e-13)
    acc = np.zeros((2, 2, 24), F)
    for q in range(100):
        acc = acc + rq[:, q][None, :, None] * e[:, q].astype(F)[:, None, :]
    assert (np.abs(acc.astype(np.float64) - ref) <= 101 * U.U32 * mag).all()
    assert (np.abs(U.fold_f64(e, rq, 99)[0] - ref) > 101 * U.U32 * mag).any()                  # one query short
    proj = r.standard_normal((2, 2, 3, 16, 2)).astype(F)
    img = U.f16(r.standard_normal((2, 8, 12, 3)))
    rimg, bias = r.standard_normal((2, 3)).astype(F), r.standard_normal(2).astype(F)
    ref, mag = U.shuf_ab_f64(proj, img, rimg, bias)
    for ch in range(2):                                            # the blur of each plane is pixshuf4_blur_f64 of that plane
        plane, _ = U.pixshuf4_blur_f64(proj[..., ch].astype(np.float64))
        want = plane[..., 0] + img.astype(np.float64) @ rimg[ch].astype(np.float64) + float(bias[ch])
        assert np.allclose(ref[..., ch], want, rtol=1e-12, atol=1e-13)
    assert U.shuf_ab_excess(ref.astype(F).astype(np.float16), ref, mag).max() <= 1.0
    assert U.shuf_ab_excess(U.shuf_ab_f64(proj[:, :, :, ::-1], img, rimg, bias)[0].astype(np.float16), ref, mag).max() > 100
