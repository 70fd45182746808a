"""CPU: that the rules of tests/remaster_util.py can fail.  Before a GPU result is trusted against the attention bound, the oracle is checked against a
naive per-query loop, an emulation of the kernel's arithmetic (64-key tiles, online softmax in float32, P rounded to fp16, float32 sums) is shown to
stay inside the limit on every case, and four kinds of wrong kernel, written as mutations of the oracle, are shown to exceed it on the named cases.
The element-wise rules are checked the same way: float32 restatements of prep and ELU pass them, a truncating fp16 conversion does not."""
import math

import numpy as np
import pytest

from oracle import remaster as O
from tests import remaster_util as U

F = np.float32


def test_oracle_attention_equals_a_naive_per_query_loop():
    case = U.CASES["cross"]
    x, q, k, v = U.attn_inputs(case, "sharp")
    ref, A = U.attn_reference(case, x, q, k, v, -1.3)
    g = float(np.float32(-1.3))
    keys, vals = k.reshape(-1, U.D).astype(np.float64), v.reshape(-1, U.DV).astype(np.float64)
    assert len(keys) == 5 * 40
    for f in range(case.T):
        for p in range(0, case.nq, 5):
            s = [sum(float(a) * float(b) for a, b in zip(q[f, p], kk)) for kk in keys]
            m = max(s)
            w = [math.exp(t - m) for t in s]
            z = sum(w)
            o = sum((wi / z) * vi for wi, vi in zip(w, vals))
            a = sum((wi / z) * np.abs(vi) for wi, vi in zip(w, vals))
            assert np.allclose(g * o + x[f, p].astype(np.float64), ref[f, p], rtol=1e-12, atol=1e-12)
            assert np.allclose(a, A[f, p], rtol=1e-12, atol=1e-12)


def emulate_kernel(case, x, q, k, v, gamma):
    """srcref_attention_kernel's arithmetic in numpy: per still, 64-key tiles, masked tail, float32 scores and running (m, l, O), P rounded to fp16"""
    n, s_n = case.frames, case.stills
    qq, xx = q[:n].reshape(-1, U.D).astype(F), x[:n].reshape(-1, U.DV).astype(F)
    NQ = len(qq)
    m, l, o = np.full(NQ, -1e30, F), np.zeros(NQ, F), np.zeros((NQ, U.DV), F)
    for r in range(s_n):
        for kv0 in range(0, case.nk, 64):
            kt, vt = k[r, kv0:kv0 + 64].astype(F), v[r, kv0:kv0 + 64].astype(F)
            s = np.full((NQ, 64), -1e30, F)
            s[:, :len(kt)] = qq @ kt.T
            m_new = np.maximum(m, s.max(1))
            alpha = np.exp(m - m_new, dtype=F)
            p = np.exp(s - m_new[:, None], dtype=F)
            l = l * alpha + p.sum(1, dtype=F)
            o = o * alpha[:, None] + p[:, :len(kt)].astype(np.float16).astype(F) @ vt
            m = m_new
    inv = F(gamma) / l
    return (o * inv[:, None] + xx).astype(np.float16).reshape(n, case.nq, U.DV)


@pytest.mark.parametrize("name", list(U.CASES))
def test_an_emulation_of_the_kernels_arithmetic_stays_inside_the_limit(name):
    case = U.CASES[name]
    for regime in case.regimes:
        x, q, k, v = U.attn_inputs(case, regime)
        U.check_regime(case, regime, q, k)
        for gamma in U.GAMMAS:
            ref, A = U.attn_reference(case, x, q, k, v, gamma)
            ratio, worst = U.attn_ratio(emulate_kernel(case, x, q, k, v, gamma), ref, A, gamma)
            print(f"{name:10s} {regime:8s} gamma {gamma:+.1f}  emulation: max err / bound {ratio:.3f}")
            assert ratio <= U.LIMIT, U.attn_worst_text(case, q, k, worst, ratio)


def _mutated(case, x, q, k, v, gamma, kind):
    """the oracle on inputs changed the way a wrong kernel would see them"""
    k, v = k.copy(), v.copy()
    S = case.stills
    if kind == "phantom":                      # a tail key that is not masked: score 0 (zero key), value 0
        k = np.concatenate([k, np.zeros((len(k), 1, U.D), np.float16)], 1)
        v = np.concatenate([v, np.zeros((len(v), 1, U.DV), np.float16)], 1)
    elif kind == "drop_last":                  # the mask one key too early
        k, v = k[:, :-1], v[:, :-1]
    elif kind == "swap_blocks":                # two 16-channel output fragments exchanged
        v[..., 16:32], v[..., 32:48] = v[..., 32:48].copy(), v[..., 16:32].copy()
    elif kind == "shift_tile":                 # the second key tile's values read 8 keys off
        assert case.nk >= 128
        v[:, 64:128] = np.roll(v[:, 64:128], -8, axis=1)
    out, _ = O.srcref_attention(x[:case.frames].reshape(-1, U.DV), q[:case.frames].reshape(-1, U.D), k[:S].reshape(-1, U.D), v[:S].reshape(-1, U.DV),
                                float(np.float32(gamma)))
    return out.reshape(case.frames, case.nq, U.DV)


@pytest.mark.parametrize("kind,names", [("phantom", ("one", "small", "edge63", "edge65", "three")),
                                        ("drop_last", ("small", "cross", "edge64", "edge65", "three", "self")),
                                        ("swap_blocks", ("one", "small", "cross", "three_wide")),
                                        ("shift_tile", ("three", "three_wide", "ring200"))])
def test_a_wrong_kernel_exceeds_the_limit_in_the_flat_regime(kind, names):
    for name in names:
        case = U.CASES[name]
        x, q, k, v = U.attn_inputs(case, "flat")
        for gamma in U.GAMMAS:
            ref, A = U.attn_reference(case, x, q, k, v, gamma)
            if kind == "drop_last" and case.nk == 1:
                continue
            ratio, _ = U.attn_ratio(_mutated(case, x, q, k, v, gamma, kind), ref, A, gamma)
            print(f"{kind:12s} {name:10s} gamma {gamma:+.1f}: max err / bound {ratio:.1f}")
            assert ratio > U.LIMIT, (kind, name, gamma, ratio)


def test_a_phantom_key_hides_behind_trained_size_scores_and_shows_with_negative_ones():
    """why the regimes exist: with |s| ~ 30 an unmasked zero-score key weighs e^-30 and passes; with every true score <= -8 it takes the output over"""
    case = U.CASES["three"]
    for regime, caught in (("sharp", False), ("negative", True)):
        x, q, k, v = U.attn_inputs(case, regime)
        ref, A = U.attn_reference(case, x, q, k, v, 0.7)
        ratio, _ = U.attn_ratio(_mutated(case, x, q, k, v, 0.7, "phantom"), ref, A, 0.7)
        frac = (np.abs(_mutated(case, x, q, k, v, 0.7, "phantom") - ref) > U.LIMIT * U.attn_bound(ref, A, 0.7)).mean()
        print(f"phantom key, {regime}: max err / bound {ratio:.1f}, elements over the limit {frac:.3f}")
        assert (frac > 0.9) if caught else (frac < 0.5), (regime, frac)


# ---- element-wise rules ----
def test_ulp_helpers_on_known_values():
    assert U.ulp16(1.0) == 2.0 ** -10 and U.ulp16(0.999) == 2.0 ** -11 and U.ulp16(2.0 ** -14) == 2.0 ** -24 and U.ulp16(1e-7) == 2.0 ** -24 and U.ulp16(0.0) == 2.0 ** -24
    assert U.ulp16(-1536.0) == 1.0 and U.ulp32(1.0) == 2.0 ** -23 and U.ulp32(0.75) == 2.0 ** -24 and U.ulp32(0.0) == 2.0 ** -149
    h = U.all_halves()
    fin = h[np.isfinite(h) & (h > 0) & (h < 65504)]
    assert np.array_equal(U.ulp16(fin.astype(np.float64)), np.spacing(fin).astype(np.float64))      # numpy's own spacing, every positive fp16 below the largest
    assert np.array_equal(U.ulp16(-fin.astype(np.float64)), U.ulp16(fin.astype(np.float64)))
    assert U.ulp16_error(np.float16(1.0), 1.0 + 2.0 ** -11) == 0.5


def test_elu_rule_passes_a_float32_restatement_and_fails_truncation():
    h = U.all_halves()
    neg = h[np.isfinite(h) & np.signbit(h)]
    exact = O.elu(neg.astype(np.float64))
    good = np.expm1(neg.astype(F)).astype(np.float16)                          # float32 expm1, then round to nearest even
    e = U.ulp16_error(good, exact)
    print(f"elu, float32 restatement: max |err| {e.max():.6f} ulp (limit {U.HALF_ULP_LIMIT:.6f})")
    assert e.max() <= U.HALF_ULP_LIMIT
    trunc = np.where(np.abs(good.astype(np.float64)) > np.abs(exact), (U.bits(good) - 1).view(np.float16), good)      # round toward zero
    assert U.ulp16_error(trunc, exact).max() > 0.9
    assert U.ulp16_error(np.exp(neg.astype(F)).astype(np.float16) - np.float16(1), exact).max() > U.HALF_ULP_LIMIT      # exp(x) - 1 in fp16: cancellation
    sp = O.elu(np.array([-0.0, -np.inf, np.inf, np.nan, 0.0, 3.5]))
    assert np.signbit(sp[0]) and sp[0] == 0 and sp[1] == -1 and sp[2] == np.inf and np.isnan(sp[3]) and not np.signbit(sp[4]) and sp[5] == 3.5


def test_prep_rule_on_all_256_levels_in_float32():
    """the kernel's float32 steps (byte / 255 - constant, rounded once to fp16) against the float64 oracle on every byte value.  Figures for the profile:
    the float32 steps put the value up to ~2^-25 from the exact one, which near the constant's zero crossing is a visible part of a (small) fp16 ulp."""
    g = np.arange(256, dtype=np.uint8)
    rgb = np.stack([g, g, g], -1)[None, None]                                   # [1][1][256][3]
    assert np.array_equal(O.gray_u8(rgb)[0, 0], g)
    for name, const, exact in (("frames", F(0.4462414), O.prep_frames(rgb)[0, 1, 1:-1]), ("refs", F(0.48), O.prep_refs(rgb)[0, 0, :, 0])):
        got = (g.astype(F) / F(255.0) - const).astype(np.float16)
        e = U.ulp16_error(got, exact)
        print(f"prep {name}, float32 restatement: max |err| {e.max():.6f} ulp at byte {int(e.argmax())} (limit {U.HALF_ULP_LIMIT:.6f})")
        assert e.max() <= U.HALF_ULP_LIMIT, (name, e.max(), int(e.argmax()))
    r = np.random.default_rng(3)
    img = r.integers(0, 256, (2, 3, 5, 3), dtype=np.uint8)
    p = O.prep_frames(img)
    assert p.shape == (2, 5, 7) and p[0, 0, 0] == p[0, 1, 1] and p[1, 4, 6] == p[1, 3, 5] and np.array_equal(p[:, 0, 1:-1], p[:, 1, 1:-1])
    c = img.astype(np.int64)
    assert np.array_equal(O.gray_u8(img), np.floor((4899 * c[..., 0] + 9617 * c[..., 1] + 1868 * c[..., 2] + 8192) / 16384.0).astype(np.uint8))


def test_tstack_oracle_is_the_temporal_window_of_a_3d_convolution():
    r = np.random.default_rng(1)
    T, H, W, C, Co = 3, 4, 5, 2, 3
    x = r.standard_normal((C, T, H, W))
    w = r.standard_normal((Co, C, 3, 3, 3))
    direct, mag = O.conv3d_same(x, w)
    from vsdeoldify_amd.remaster_net import repack_temporal
    st = O.tstack(x.transpose(1, 2, 3, 0).reshape(T, H * W, C)).reshape(T, H, W, 3 * C)
    sp = np.pad(st, ((0, 0), (1, 1), (1, 1), (0, 0)))
    w2 = repack_temporal(w)
    got = sum(np.einsum("oc,thwc->othw", w2[:, :, kh, kw], sp[:, kh:kh + H, kw:kw + W]) for kh in range(3) for kw in range(3))
    assert np.allclose(got, direct, rtol=0, atol=1e-12) and (mag >= np.abs(direct) - 1e-12).all()
    assert not O.tstack(np.ones((1, 2, 8)))[0, :, :8].any() and not O.tstack(np.ones((1, 2, 8)))[0, :, 16:].any()


def test_output_grid_and_the_share_of_bytes_left_out():
    """the 256 x 52 x 52 grid: the grey formula returns g for (g, g, g); with float64 sigmoids rounded to float32 no byte lies in the left-out window, and
    both the gamut clip and the fz < 0 clamp are well populated"""
    from tests import sweep_util as su
    rgb, ab = U.out_grid()
    assert rgb.shape == (256, 2704, 3) and ab.shape == (256, 2704, 2) and ab.dtype == np.float16
    assert np.array_equal(O.gray_u8(rgb), rgb[..., 0])
    assert len(np.unique(U.bits(ab[0]).astype(np.int64)[:, 0] * 65536 + U.bits(ab[0])[:, 1])) == 2704
    sg = O.sigmoid(ab.astype(np.float64)).astype(F)
    assert sg.min() == 0.0 and sg.max() == 1.0
    lab = O.lab_from_sigmoid(O.gray_u8(rgb), sg[..., 0], sg[..., 1])
    assert lab.dtype == F and lab[..., 1:].min() == -100 and lab[..., 1:].max() == 100 and lab[255, 0, 0] == 100
    want, v = U.out_bytes(lab)
    share = float(su.left_out(v).mean())
    clipped = float(((v <= 0) | (v >= 1)).mean())
    fz = (lab[..., 0].astype(np.float64) + 16) / 116 - lab[..., 2].astype(np.float64) / 200 < 0
    print(f"output grid: bytes left out {share:.3e}, bytes clipped {clipped:.3f}, pixels with fz < 0 {fz.mean():.3f}")
    assert share <= su.LEFT_OUT_CAP and 0.3 < clipped < 0.7 and 0.05 < fz.mean() < 0.3
    assert want.dtype == np.uint8 and want.shape == rgb.shape
