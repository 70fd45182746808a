"""CPU: that the rules of tests/deoldify_ops_util.py can fail, and that its oracles are the operations they are named for.  Before a GPU result is
trusted against the attention bound, oracle.unet.self_attention_f64 is checked against a naive per-query loop and against the restated torch layer, an
emulation of the kernels' arithmetic is shown to stay inside the limit on every case, and five kinds of wrong kernel, written as mutations of the oracle's
inputs, are shown to exceed it on the named cases.  The element-wise rules are checked the same way: float32 restatements pass them, a truncating fp16
conversion does not; the numpy oracles of max-pool and blur + nearest resize equal torch's."""
import math

import numpy as np
import pytest

from oracle.unet import self_attention_f64
from tests import deoldify_ops_util as U

F = np.float32


def test_the_case_list_is_the_one_the_kernels_ask_for():
    assert len(U.CASES) == 6 * 11 + 3
    for d, c in U.PAIRS:
        for n in U.NS:
            case = U.CASES[f"d{d}c{c}n{n}"]
            assert case.B == (2 if n in (65, 129, 200) else 1) and "flat" in case.regimes and "negative" in case.regimes
            assert ("rising" in case.regimes) == (n > 64) == ("falling" in case.regimes)
    assert sorted(c % 256 == 0 for _, c in U.PAIRS) == [False] * 3 + [True] * 3 and {d for d, _ in U.PAIRS} == {32, 64, 96}
    assert U.CASES["d64c512n1225"].regimes == ("flat",)
    short = [c for c in U.CASES.values() if c.batch]
    assert {(c.B, c.batch, c.C % 256 == 0) for c in short} == {(3, 2, True), (3, 2, False)}
    x, f, g, h = U.attn_inputs(short[0], "flat")
    assert all((a[2] == 3000).all() and np.abs(a[:2].astype(np.float64)).max() < 100 for a in (x, f, g, h))


def test_oracle_attention_equals_a_naive_per_query_loop_and_the_torch_layer():
    import torch
    from oracle import unet as ou
    case = U.CASES["d32c128n65"]
    x, f, g, h = U.attn_inputs(case, "sharp")
    ref, A = U.attn_reference(case, x, f, g, h, -1.3)
    gm = float(np.float32(-1.3))
    for b in range(case.B):
        keys, vals = f[b].astype(np.float64), h[b].astype(np.float64)
        for j in range(0, case.N, 4):
            s = [sum(float(a) * float(c) for a, c in zip(g[b, j], kk)) for kk in keys]
            m = max(s)
            w = [math.exp(t - m) for t in s]
            z = sum(w)
            o = sum((wi / z) * vi for wi, vi in zip(w, vals))
            a = sum((wi / z) * np.abs(vi) for wi, vi in zip(w, vals))
            assert np.allclose(gm * o + x[b, j].astype(np.float64), ref[b, j], rtol=1e-12, atol=1e-12)
            assert np.allclose(a, A[b, j], rtol=1e-12, atol=1e-12)
    # the layer as oracle/unet.py restates it from the reference (float32 torch), fed 1x1 convs whose spectral fold is the identity: x -> (f, g, h)
    r = np.random.default_rng(5)
    C, d, N = 16, 4, 12
    xt = r.standard_normal((1, C, 3, 4))
    sd = {}
    ws = {}
    for nm, rows in (("query", d), ("key", d), ("value", C)):
        w = r.standard_normal((rows, C, 1)) / 4
        v = np.ones(C) / np.sqrt(C)
        t = w.reshape(rows, -1) @ v
        sd[f"a.{nm}.weight_orig"], sd[f"a.{nm}.weight_v"], sd[f"a.{nm}.weight_u"] = torch.from_numpy(w), torch.from_numpy(v), torch.from_numpy(t / t.dot(t))
        ws[nm] = w[..., 0]
    sd["a.gamma"] = torch.tensor([0.7], dtype=torch.float64)
    want = ou.self_attention(sd, "a", torch.from_numpy(xt)).numpy().reshape(C, N).T
    xs = xt.reshape(C, N).T
    got, _ = self_attention_f64(xs, xs @ ws["query"].T, xs @ ws["key"].T, xs @ ws["value"].T, 0.7)
    assert np.allclose(got, want, rtol=1e-10, atol=1e-10)


@pytest.mark.parametrize("name", list(U.CASES))
def test_an_emulation_of_the_kernels_arithmetic_stays_inside_the_limit(name):
    case = U.CASES[name]
    for regime in case.regimes:
        x, f, g, h = U.attn_inputs(case, regime)
        U.check_regime(case, regime, f, g)
        for gamma in U.GAMMAS:
            ref, A = U.attn_reference(case, x, f, g, h, gamma)
            ratio, worst = U.attn_ratio(U.emulate_attention(case, x, f, g, h, gamma), ref, A, gamma)
            print(f"{name:14s} {regime:8s} gamma {gamma:+.1f}  emulation: max err / bound {ratio:.3f}")
            assert ratio <= U.LIMIT, U.attn_worst_text(case, f, g, worst, ratio)


def _mutated(case, x, f, g, h, gamma, kind):
    """the oracle on inputs changed the way a wrong kernel would see them"""
    f, g, h = f.copy(), g.copy(), h.copy()
    if kind == "phantom":                      # a tail key that is not masked: score 0 (zero key), value 0
        f = np.concatenate([f, np.zeros((len(f), 1, case.D), np.float16)], 1)
        h = np.concatenate([h, np.zeros((len(h), 1, case.C), np.float16)], 1)
    elif kind == "drop_last":                  # the mask one key too early
        f, h = f[:, :-1], h[:, :-1]
    elif kind == "swap_blocks":                # two 16-channel output fragments exchanged
        h[..., 16:32], h[..., 32:48] = h[..., 32:48].copy(), h[..., 16:32].copy()
    elif kind == "shift_tile":                 # the second key tile's values read 8 keys off
        assert case.N >= 128
        h[:, 64:128] = np.roll(h[:, 64:128], -8, axis=1)
    elif kind == "transposed":                 # f and g exchanged: s^T, the softmax runs over the wrong index
        f, g = g, f
    gm = float(np.float32(gamma))
    return np.stack([self_attention_f64(x[b], f[b], g[b], h[b], gm)[0] for b in range(case.frames)])


@pytest.mark.parametrize("kind,names", [("phantom", ("d64c512n1", "d32c128n15", "d96c768n63", "d64c384n65", "d32c256n129", "d96c128n200")),
                                        ("drop_last", ("d32c128n15", "d64c512n64", "d96c128n65", "d32c256n128", "d64c384n129", "d96c768n323")),
                                        ("swap_blocks", ("d64c512n1", "d32c128n16", "d96c768n65", "d64c384n200")),
                                        ("shift_tile", ("d64c512n128", "d32c128n129", "d96c768n200", "d64c384n323")),
                                        ("transposed", ("d32c128n15", "d64c512n64", "d96c768n65", "d64c384n129", "d32c256n323"))])
def test_a_wrong_kernel_exceeds_the_limit_in_the_flat_regime(kind, names):
    for name in names:
        case = U.CASES[name]
        x, f, g, h = U.attn_inputs(case, "flat")
        for gamma in U.GAMMAS:
            ref, A = U.attn_reference(case, x, f, g, h, gamma)
            ratio, _ = U.attn_ratio(_mutated(case, x, f, g, h, gamma, kind), ref, A, gamma)
            print(f"{kind:12s} {name:14s} gamma {gamma:+.1f}: max err / bound {ratio:.1f}")
            assert ratio > U.LIMIT, (kind, name, gamma, ratio)


def test_a_phantom_key_hides_behind_sharp_scores_and_shows_with_negative_ones():
    """why the regimes exist: with |s| beyond 20 an unmasked zero-score key weighs e^-20 for most queries and passes there; with every true score <= -8
    it takes the output over"""
    case = U.CASES["d64c512n129"]
    for regime, caught in (("sharp", False), ("negative", True)):
        x, f, g, h = U.attn_inputs(case, regime)
        ref, A = U.attn_reference(case, x, f, g, h, 0.7)
        frac = (np.abs(_mutated(case, x, f, g, h, 0.7, "phantom") - ref) > U.LIMIT * U.attn_bound(ref, A, 0.7)).mean()
        print(f"phantom key, {regime}: elements over the limit {frac:.3f}")
        assert (frac > 0.9) if caught else (frac < 0.5), (regime, frac)


# ---- element-wise rules ----
def test_maxpool_and_blur_oracles_equal_torch():
    import torch
    import torch.nn.functional as TF
    r = np.random.default_rng(2)
    for H, W in U.SHAPES + ((9, 9), (36, 36)):
        x = r.standard_normal((2, H, W, 3))
        xt = torch.from_numpy(x.transpose(0, 3, 1, 2).copy())
        assert np.array_equal(U.maxpool_f64(x), TF.max_pool2d(xt, 3, 2, 1).numpy().transpose(0, 2, 3, 1))
        blur = TF.avg_pool2d(TF.pad(xt, (1, 0, 1, 0), mode="replicate"), 2, stride=1)
        for Ho, Wo in ((H, W), (max(H - 1, 1), W), (H, max(W - 1, 1)), (2 * H, 2 * W)):
            want = TF.interpolate(blur, (Ho, Wo), mode="nearest").numpy().transpose(0, 2, 3, 1)
            assert np.allclose(U.blur_resize_f64(x, Ho, Wo), want, rtol=0, atol=1e-15), (H, W, Ho, Wo)
    assert U.nearest_index(36, 35).tolist() == [min(int(np.floor(np.float32(i) * (np.float32(36) / np.float32(35)))), 35) for i in range(35)]
    v = U.blur_inputs((2, 18, 18, 8), 1)
    assert np.abs(v.astype(np.float64)).max() <= 16 and np.array_equal(v.astype(np.float64) * 256, np.round(v.astype(np.float64) * 256))
    # the kernel's float32 steps on such inputs are exact: one rounding, the store
    s32 = (v[:, :-1, :-1].astype(F) + v[:, :-1, 1:].astype(F) + v[:, 1:, :-1].astype(F) + v[:, 1:, 1:].astype(F)) * F(0.25)
    assert np.array_equal(s32.astype(np.float64), U.blur_resize_f64(v, 18, 18)[:, 1:, 1:])


def _toward_zero(v64):
    """float64 -> fp16 rounded toward zero"""
    h = v64.astype(np.float16)
    over = np.abs(h.astype(np.float64)) > np.abs(v64)
    return np.where(over, (U.bits(h) - 1).view(np.float16), h)


def test_affine_rule_passes_float32_with_and_without_fma_and_fails_truncation():
    r = np.random.default_rng(3)
    x = U.f16(2.0 * r.standard_normal((4096, 264)))
    scale, shift = (1.5 * r.standard_normal(264)).astype(F), (3.0 * r.standard_normal(264)).astype(F)
    for relu in (False, True):
        exact, mag = U.affine_exact(x, scale, shift, relu)
        assert np.abs(exact).max() < 1000
        plain = x.astype(F) * scale + shift                                                  # product rounded to float32, then the sum
        fused = (x.astype(np.float64) * scale.astype(np.float64) + shift.astype(np.float64)).astype(F)      # one rounding (the float64 product is exact)
        for label, v in (("mul + add", plain), ("fma", fused)):
            v = np.maximum(v, F(0)) if relu else v
            e = U.affine_excess(v.astype(np.float16), exact, mag)
            print(f"affine relu={relu} float32 {label}: max excess {e.max():.4f} (<= 1 passes)")
            assert e.max() <= 1.0
        assert (plain != fused).any()
        assert U.affine_excess(_toward_zero(exact), exact, mag).max() > 1.5
    # a scale / shift pair taken from the wrong channel fails as well
    exact, mag = U.affine_exact(x, scale, shift, False)
    assert U.affine_excess((x.astype(F) * np.roll(scale, 8) + np.roll(shift, 8)).astype(np.float16), exact, mag).max() > 100


def test_prep_rule_on_all_256_levels_in_float32():
    L = np.arange(256)
    exact = U.prep_exact(L)
    got = ((L.astype(F)[:, None] / F(255.0) - U.MEAN) / U.STD).astype(np.float16)
    e = U.prep_excess(got, exact)
    print(f"prep_rgb8, float32 restatement: max excess {e.max():.4f} at level {int(e.max(1).argmax())} (<= 1 passes)")
    assert e.max() <= 1.0
    assert U.prep_excess(_toward_zero(exact), exact).max() > 1.5
    # the 256 levels are separable in every channel's fp16 values: L can be read back through them
    assert all(len(np.unique(U.bits(got[:, c]))) == 256 for c in range(3))
    rgb = U.prep_images()
    g = np.arange(256)
    assert rgb.shape == (2, 66, 66, 3) and np.array_equal(U.gray_l(rgb[0].reshape(-1, 3)[:256]), g)
    assert np.array_equal(U.gray_l(np.array([[255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255]])), [255, 76, 150, 29])


def test_view_helpers():
    v = U.finite_patterns((2, 3, 8), 1)
    assert np.isfinite(v).all() and (v != 0).all() and (U.bits(v) != U.SENT).all()
    buf = U.in_view(v, 24, 8)
    assert np.array_equal(U.bits(buf[..., 8:16]), U.bits(v)) and U.outside_is_sentinel(buf, 8, 8)
    buf[0, 0, 3] = 1.0
    assert not U.outside_is_sentinel(buf, 8, 8)
    vT = U.value_rows(np.arange(2 * 3 * 4, dtype=np.float16).reshape(2, 3, 4), 64, 5.0)
    assert vT.shape == (2, 4, 64) and vT[1, 2, 1] == 12 + 4 + 2 and (vT[:, :, 3:] == 5).all()
