"""CPU side of tests/test_gpu_colormnet_ops.py (tests/colormnet_ops_util.py holds the cases, oracles and rules):
1. every float64 oracle agrees with the repository's fp32 oracle (oracle/colormnet_net.py: cbam, _gru, the Fuse cross-attention) and with torch
   (F.interpolate, F.conv2d(groups=C), softmax) to fp32 accuracy on the very cases the GPU file runs;
2. for every rule a numpy float32 emulation of the kernel's own order stays at or below 1.0 of the bound on every case -- the condition the reference
   alone satisfies, checked before any GPU run;
3. the same emulation with a seeded defect exceeds LIMIT: the rules can fail, and the `edges` regimes are what makes them;
4. the launcher choices restated in the util are those of vsdeoldify_amd.colormnet_net.chan_attn_splits."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from oracle import colormnet_net as ON
from tests import colormnet_ops_util as U

F = np.float32


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, F)))


def _nchw(a):
    return _t(a).permute(0, 3, 1, 2)


_CCA = {}


def cca(name, regime):
    if (name, regime) not in _CCA:
        case = U.CCA_CASES[name]
        q, k, v, temp = U.cca_inputs(case, regime)
        Wref, cos = U.cca_reference(q, k, temp, case.heads)
        _CCA[name, regime] = (case, q, k, v, temp, Wref, U.cca_bound(Wref, temp, case.per, case.S))
    return _CCA[name, regime]


# ---- 4. launcher choices ----------------------------------------------------------------------------------------------------------------------------------------------
def test_restated_launcher_choices_are_the_exported_ones():
    from vsdeoldify_amd.colormnet_net import HEADS_CCA, chan_attn_splits
    for case in U.CCA_CASES.values():
        assert U.cca_choice(case.P, case.heads, case.c) == (case.tiles, case.S, case.per), case.name
        assert chan_attn_splits(case.P, case.heads, case.c) == case.S, case.name
    for P in (1, 127, 128, 129, 392, 1568, 6272, 100000):
        for heads, c in ((8, 64), (8, 128), (8, 256), (2, 256), (1, 8), (8, 72)):
            assert U.cca_choice(P, heads, c)[1] == chan_attn_splits(P, heads, c), (P, heads, c)
    assert {2 * d // HEADS_CCA for d in (256, 512, 1024)} == {64, 128, 256} <= {c.c for c in U.CCA_CASES.values()}       # the product's channels per head
    assert [U.cbam_choice(C) for C in U.CBAM_CHANNELS] == [U.CBAM_CHOICE[C] for C in U.CBAM_CHANNELS]
    assert U.cbam_choice(4096) == (2, 2048) and U.cbam_choice(2048)[0] == 4
    for C in U.CBAM_CHANNELS:                                   # the chunks cover the channels and the partials fit the 2 Ch x 16 floats the launcher gives
        NCH, clen = U.cbam_choice(C)
        assert NCH * clen >= C and NCH <= 16 and clen % 4 == 0 and (C // 16) * NCH <= 512
    assert U.dw_kernel(3) == "dwconv3_strip_kernel" and U.dw_kernel(5) == "dwconv_kernel<5>"


def test_the_edge_pixels_are_what_the_kernel_splits_at():
    assert U.cca_edge_pixels(129, 2) == [0, 31, 32, 63, 64, 65, 96, 97, 128]
    for case in U.CCA_CASES.values():
        e = U.cca_edge_pixels(case.P, case.S)
        assert case.P - 1 in e and all(s * case.per - 1 in e and s * case.per in e for s in range(1, case.S)), case.name
    assert U.mha64_edge_keys(513) == [0, 63, 64, 127, 128, 191, 192, 255, 256, 319, 320, 383, 384, 447, 448, 511, 512]
    assert U.mha64_edge_keys(64) == [0, 63] and U.mha64_edge_keys(1) == [0] and U.mha64_edge_keys(65) == [0, 63, 64]


# ---- 1. the float64 oracles against torch and the fp32 oracle -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c64", "c72", "one"])
def test_channel_attention_oracle_is_the_fuse_cross_attention(name):
    """oracle.colormnet_net.cross_channel_attention with identity projections: softmax(normalize(q) normalize(k)^T temperature) @ v"""
    case, q, k, v, temp, Wref, _ = cca(name, "flat")
    C2, H, W = case.C2, case.H, case.W
    eye, dw = torch.eye(C2).view(C2, C2, 1, 1), torch.zeros(C2, 1, 3, 3)
    dw[:, 0, 1, 1] = 1
    sd = {"p.temperature": _t(temp).view(case.heads, 1, 1), "p.to_out.0.weight": eye}
    for n in "qkv":
        sd[f"p.to_{n}.weight"], sd[f"p.to_{n}_dw.weight"] = eye, dw
    enc = _t(q).reshape(case.B, H, W, C2).permute(0, 3, 1, 2)
    # keys and values come from ONE tensor in the module: run it twice, with dec = k for the matrix and dec = v for the values
    tq, tk, tv = (_t(a).reshape(case.B, case.P, case.heads, case.c).permute(0, 2, 3, 1) for a in (q, k, v))
    attn = ((TF.normalize(tq, dim=-1) @ TF.normalize(tk, dim=-1).transpose(-2, -1)) * sd["p.temperature"]).softmax(-1)
    assert np.abs(attn.numpy() - Wref).max() < 2e-5
    ref, _, _ = U.cca_apply_f64(Wref, v)
    want = (attn @ tv).permute(0, 3, 1, 2).reshape(case.B, case.P, C2)
    assert np.abs(want.numpy() - ref).max() < 1e-4
    if not case.zero:
        kk = k.copy()
        out = ON.cross_channel_attention(sd, "p", enc, _t(kk).reshape(case.B, H, W, C2).permute(0, 3, 1, 2), heads=case.heads)
        mine, _, _ = U.cca_apply_f64(Wref, kk)
        assert np.abs(out.permute(0, 2, 3, 1).reshape(case.B, case.P, C2).numpy() - mine).max() < 1e-4
    else:
        assert np.abs(Wref[:, 0, 3] - 1.0 / case.c).max() == 0                       # the eps path: uniform row, as F.normalize(eps=1e-12) gives
        assert np.abs(attn.numpy()[:, 0, 3] - 1.0 / case.c).max() < 1e-7


def test_mha64_oracle_is_torch_softmax_attention():
    case = U.MHA_CASES["h6l65"]
    q, k, v = U.mha64_inputs(case, "flat")
    ref = U.mha64_reference(q, k, v, case.heads)
    t = [_t(a).reshape(case.B, case.L, case.heads, 64).permute(0, 2, 1, 3) for a in (q, k, v)]
    want = (torch.softmax(t[0] * 0.125 @ t[1].transpose(-2, -1), -1) @ t[2]).transpose(1, 2).reshape(case.B, case.L, case.E)
    assert np.abs(want.numpy() - ref["out"]).max() < 1e-5


@pytest.mark.parametrize("name", list(U.EW_CASES))
def test_ew_oracle_is_torch_interpolate(name):
    case = U.EW_CASES[name]
    x, res = U.ew_inputs(case, 8, "random")
    ref, _ = U.ew_f64(case, x, res, "f64")
    xs = np.broadcast_to(x[:1], x.shape) if case.src_bcast else x
    if case.mode == 1:
        want = TF.interpolate(_nchw(xs), size=case.dst, mode="bilinear", align_corners=False)
    elif case.mode == 2:
        want = TF.interpolate(_nchw(xs), scale_factor=1.0 / case.factor, mode="area")
    else:
        want = _nchw(xs)
    if case.res:
        want = want + _nchw(np.broadcast_to(res[:1], res.shape) if case.res == "bcast" else res)
    assert np.abs(want.permute(0, 2, 3, 1).numpy() - ref).max() < 5e-6 * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("K", [3, 5])
def test_dwconv_oracle_is_torch_grouped_conv(K):
    C = 40
    w, bias = U.dw_params(C, K)
    for H, W in ((1, 1), (2, 3), (9, 5)):
        x = U.dw_inputs(H, W, C)
        ref, _ = U.dwconv_f64(x, w, bias)
        want = TF.conv2d(_nchw(x), _t(w).view(C, 1, K, K), _t(bias), padding=K // 2, groups=C)
        assert np.abs(want.permute(0, 2, 3, 1).numpy() - ref).max() < 1e-5


@pytest.mark.parametrize("C", [16, 64, 576])
def test_cbam_oracle_is_the_fp32_oracle(C):
    x, params = U.cbam_inputs(C, 6, 9), U.cbam_params(C)
    ref, bound = U.cbam_f64(x, params)
    names = ("ChannelGate.mlp.1.weight", "ChannelGate.mlp.1.bias", "ChannelGate.mlp.3.weight", "ChannelGate.mlp.3.bias", "SpatialGate.spatial.conv.weight",
             "SpatialGate.spatial.conv.bias")
    sd = {"a." + n: _t(p) for n, p in zip(names, params)}
    sd["a.SpatialGate.spatial.conv.weight"] = sd["a.SpatialGate.spatial.conv.weight"].view(1, 2, 7, 7)
    want = _nchw(x) + ON.cbam(sd, "a", _nchw(x))
    assert np.abs(want.permute(0, 2, 3, 1).numpy() - ref).max() < 1e-5 * max(1.0, np.abs(ref).max())
    assert (bound > 0).all() and (bound >= U.ulp16(ref) / 2).all()


def test_gru_oracle_is_the_fp32_oracle():
    hd = 8
    vals = U.f16(np.random.default_rng(1).standard_normal((2, 33, 3 * hd)))
    h = np.random.default_rng(2).standard_normal((2, hd, 33)).astype(F)
    ref, _ = U.gru_f64(vals, h, hd)
    want = ON._gru(_t(vals).permute(0, 2, 1).unsqueeze(0), _t(h).unsqueeze(0), hd)[0]
    assert np.abs(want.numpy() - ref).max() < 1e-6


# ---- 2. the float32 emulations of the kernels' own order stay inside the rules ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", U.CCA_REGIMES)
@pytest.mark.parametrize("name", list(U.CCA_CASES))
def test_channel_attention_emulation_is_within_the_rule(name, regime):
    case, q, k, v, temp, Wref, bw = cca(name, regime)
    em = U.cca_emulate(case, q, k, temp)
    fig, where = U.figure(em, Wref, bw)
    assert fig <= 1.0, (fig, where)
    if regime == "edges" and case.P > 1:                          # the regime's property: the edge pixels hold nearly all of the energy
        e = U.cca_edge_pixels(case.P, case.S)
        for a in (q, k):
            en = a.astype(np.float64) ** 2
            tot = en.sum(1)
            assert (en[:, e].sum(1)[tot > 0] / tot[tot > 0]).min() > 0.9
    if case.conv:                                                 # the fp16 matrix applied in float32, any order: inside both conv rules
        blocks = em.astype(F)
        vf = v.astype(F).reshape(case.B, case.P, case.heads, case.c)
        out = np.einsum("bhij,bphj->bphi", blocks, vf).reshape(v.shape).astype(np.float16)
        ref, mag, extra = U.cca_apply_f64(Wref, v, bw)
        assert U.figure(out, ref, U.ulp16(ref) / 2 + case.C2 * U.U32 * mag + extra)[0] <= 1.0
        ref, mag, _ = U.cca_apply_f64(em, v)
        assert U.figure(out, ref, U.ulp16(ref) / 2 + case.C2 * U.U32 * mag)[0] <= 1.0


_MHA = {}


def mha(name, regime):
    if (name, regime) not in _MHA:
        case = U.MHA_CASES[name]
        q, k, v = U.mha64_inputs(case, regime)
        ref = U.mha64_reference(q, k, v, case.heads, U.mha64_targets(case, regime, k) if regime in ("sharp", "edges") else None)
        U.mha64_check_regime(case, regime, ref)
        _MHA[name, regime] = (case, q, k, v, ref)
    return _MHA[name, regime]


@pytest.mark.parametrize("name", list(U.MHA_CASES))
def test_mha64_emulation_is_within_the_rule(name):
    for regime in U.MHA_CASES[name].regimes:
        case, q, k, v, ref = mha(name, regime)
        ratio, worst = U.attn_ratio(U.mha64_emulate(q, k, v, case.heads), ref["out"], ref["A"], 1.0)
        assert ratio <= 1.0, (regime, ratio, worst)


@pytest.mark.parametrize("name", list(U.EW_CASES))
def test_ew_emulation_is_within_the_rule(name):
    case = U.EW_CASES[name]
    for C in U.EW_CHANNELS:
        for kind in ("random", "patterns"):
            x, res = U.ew_inputs(case, C, kind)
            for how in ("fma", "mul_add") if case.mode == 1 else ("fma",):
                ref, bound = U.ew_f64(case, x, res, how)
                v = U.ew_emulate(case, x, res, how)
                with np.errstate(over="ignore"):
                    y = (np.maximum(v, F(0)) if case.relu else v).astype(np.float16)
                if case.exact:
                    want = np.broadcast_to(x[:1], x.shape) if case.src_bcast else x
                    assert np.array_equal(U.bits(y), U.bits(U.relu16(want) if case.relu else want))
                else:
                    fig, where = U.figure(y, np.maximum(ref, 0) if case.relu else ref, bound)
                    assert fig <= 1.0, (C, kind, how, fig, where)


@pytest.mark.parametrize("K", [3, 5])
def test_dwconv_emulation_is_within_the_rule(K):
    for C in U.DW_CHANNELS:
        w, bias = U.dw_params(C, K)
        for H, W in (U.DW_SHAPES if K == 3 else U.DW5_SHAPES):
            x = U.dw_inputs(H, W, C)
            for bb in (bias, None):
                ref, mag = U.dwconv_f64(x, w, bb)
                fig, where = U.figure(U.dw_emulate(x, w, bb), ref, U.dw_bound(ref, mag, K))
                assert fig <= 1.0, (H, W, C, fig, where)


@pytest.mark.parametrize("C", U.CBAM_CHANNELS)
def test_cbam_emulation_is_within_the_rule(C):
    params = U.cbam_params(C)
    for H, W in U.CBAM_GRIDS + (((1, 7), (1, 16), (1, 17)) if C == 64 else ()):
        x = U.cbam_inputs(C, H, W)
        ref, bound = U.cbam_f64(x, params)
        fig, where = U.figure(U.cbam_emulate(x, params), ref, bound)
        assert fig <= 1.0, (H, W, fig, where)


def test_gru_and_planar_out_emulations_are_within_their_rules():
    for hd in (8, 16):
        vals = U.act_inputs((2, 77, 3 * hd), [61, hd])
        h = (0.5 * np.random.default_rng(hd).standard_normal((2, hd, 77))).astype(F)
        ref, bound = U.gru_f64(vals, h, hd)
        fig, where = U.figure(U.gru_emulate(vals, h, hd), ref, bound, half=False)
        assert fig <= 1.0, (hd, fig, where)
    x = U.act_inputs((2, 45, 5), [71, 5])
    xf = x.astype(F).transpose(0, 2, 1)
    with np.errstate(over="ignore"):
        em = {0: xf, 1: xf * xf + F(1), 2: F(1) / (F(1) + np.exp(-xf, dtype=F)), 3: np.tanh(xf, dtype=F)}
    for act in range(4):
        ref, bound = U.planar_out_f64(x, act)
        if bound is None:
            assert np.array_equal(em[act].view(np.uint32), ref.astype(F).view(np.uint32)), act
        else:
            assert U.figure(em[act], ref, bound, half=False)[0] <= 1.0, act


# ---- 3. seeded defects are caught -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n, c in U.CCA_CASES.items() if c.P > 1])
def test_a_dropped_pixel_or_a_skipped_tile_exceeds_the_limit(name):
    case, q, k, v, temp, Wref, bw = cca(name, "edges")
    fig, _ = U.figure(U.cca_emulate(case, q, k, temp, "drop_last_pixel"), Wref, bw)
    assert fig > U.LIMIT, ("drop_last_pixel", fig)
    if case.tiles > 1:
        fig, _ = U.figure(U.cca_emulate(case, q, k, temp, "skip_tile_cols"), Wref, bw)
        assert fig > U.LIMIT, ("skip_tile_cols", fig)


@pytest.mark.parametrize("name", [n for n, c in U.MHA_CASES.items() if c.L > 64])
def test_an_omitted_rescale_or_a_dropped_tile_edge_key_exceeds_the_limit(name):
    for defect, regimes in (("no_rescale", ("edges", "rising")), ("drop_key64", ("edges",))):
        for regime in regimes:
            case, q, k, v, ref = mha(name, regime)
            ratio, _ = U.attn_ratio(U.mha64_emulate(q, k, v, case.heads, defect), ref["out"], ref["A"], 1.0)
            assert ratio > U.LIMIT, (defect, regime, ratio)


def test_a_skipped_strip_column_exceeds_the_limit():
    w, bias = U.dw_params(8, 3)
    for H, W in U.DW_SHAPES:
        if W < U.DW_COLS:
            continue
        x = U.dw_inputs(H, W, 8)
        ref, mag = U.dwconv_f64(x, w, bias)
        assert U.figure(U.dw_emulate(x, w, bias, "skip_last_col"), ref, U.dw_bound(ref, mag, 3))[0] > U.LIMIT, (H, W)


@pytest.mark.parametrize("C", U.CBAM_CHANNELS)
def test_a_dropped_cbam_chunk_exceeds_the_limit(C):
    params = U.cbam_params(C)
    x = U.cbam_inputs(C, 6, 9)
    ref, bound = U.cbam_f64(x, params)
    assert U.figure(U.cbam_emulate(x, params, "drop_chunk"), ref, bound)[0] > U.LIMIT
