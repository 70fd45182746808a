"""Shared by tests/test_gpu_colormnet_ops.py (GPU) and tests/test_colormnet_ops_host.py (CPU): the cases, inputs, float64 oracles, error rules, numpy
emulations and one-op plans by which the 14 ColorMNet network kernels of csrc/colormnet_net.hip are held, one op at a time, against plain float64.
Inputs are fp16-exact (fp32-exact where the op reads fp32) and every reference is computed from those very values, in numpy, without the code under test.
Every figure is max |GPU - ref| / bound; u = 2^-24 is the unit roundoff of fp32, ulp16 the fp16 ulp AT the exact value; the GPU limit is LIMIT = 2 x bound
(tests/remaster_util.py), the fp32 emulations of the kernels' own order stay at or below 1.0 (tests/test_colormnet_ops_host.py).  An fp16 result whose
exact value lies at or beyond 65520 - 2 bound may be +-inf.  Every view sits at a non-zero channel offset of a wider row that holds the sentinel.

kernel -> cases
    ew_kernel               EW_CASES (every mode x flag combination of the plan) on C = 8 and C = 24, B = 2, random and finite_patterns inputs
    dwconv3_strip_kernel    DW_SHAPES with K = 3 (launch_dwconv sends every K = 3 there; dwconv_kernel<3> is instantiated by no launcher)
    dwconv_kernel<5>        DW5_SHAPES with K = 5
    chan_gram / chan_softmax   CCA_CASES x ("flat", "edges"); the W_FROM_BUF conv that applies the matrix where C2 % 64 == 0
    mha64_kernel            MHA_CASES x MHA_REGIMES
    cbam_pool / cbam_mlp / cbam_spatial_pool / cbam_apply   CBAM_CASES (C 16 .. 1024 on three grids), CBAM_TAIL_P (P = 1 .. 17 at C = 64)
    gru_kernel              HD 8 and 16, values at a channel offset
    planar_in_kernel        C 3, 5, 16 x pixel_major x bcast;  planar_out_kernel  C 1, 5, 64 x act 0 .. 3;  cmn_decoder_in_kernel  one case, B = 2

Launcher choices, restated here and asserted before a case runs: cca_choice (tiles per side, S of chan_attn_splits, pixels per split), dw_kernel
(strip for K = 3, per-pixel for K = 5), cbam_choice (NCH, clen of cbam_mlp_kernel at 512 threads).

Rules
chan_attn (W fp16).  The Gram entry G_ij = sum_p q_ip k_jp is an fp32 sum (products of fp16 values are exact in fp32) of `per` pixels one after the
other, then S splits: |dG| <= (per + S) u sum|q k| <= (per + S) u |q_i| |k_j| (Cauchy-Schwarz), i.e. (per + S) u on the cosine.  Each squared norm is
summed likewise (relative (per + S) u, positive terms), sqrt halves that and adds u: the two norms move the cosine (|cos| <= 1) by (per + S + 2) u; the
product of the norms, the division and the temperature add 4 u.  Score error ds <= t (2 (per + S) + 6) u, t = |temperature|.  A softmax weight moves
by <= 2 max ds relative (its own score and the normaliser).  __expf(d), d = score - max in [-2 t, 0], is within (2 + 2 |d|) u relative (ddcolor_ops_util,
proj2 mode 1), for the weight and for the normaliser: 2 (2 + 4 t) u.  The tree sum over 256 lanes has 8 levels of positive terms, the division one more:
    bound = ulp16(ref) / 2 + u ref (2 t (2 (per + S) + 6) + 2 (2 + 4 t) + 9)
attn@v (the 1 x 1 conv with the matrix as weights, fp32 MFMA accumulation over C2 products, one fp16 store).  Against the GPU's own fp16 matrix W:
    bound = ulp16(ref) / 2 + C2 u sum_j |W_ij v_j|;     against the float64 matrix the matrix's own bound is added:  + sum_j bound(W_ij) |v_j|.
mha64: the project's attention rule, bound = 2^-11 (A + |ref|), A = sum_k P_k |V_k| (remaster_util).
ew.  copy, relu, dual, broadcasts: bit-exact.  + residual: one fp32 sum of two fp16 values: ulp16(ref) / 2 + u (|x| + |res|).  area, factor f: f^2 serial
fp32 adds, one product: ulp16(ref) / 2 + (f^2 + 1) u sum|v| / f^2 (with a residual u (sum|v| / f^2 + |res|) more).  bilinear: the source coordinate from the FLOAT32 ratio in fp32, fused or not (either is
accepted for a whole run, as for ddcolor_ops_util's bilinear2), four fp32 weights (3 roundings each), four products, three sums: 8 u max|taps|; with a
residual u (max|taps| + |res|) more; one fp16 store: ulp16(ref) / 2 + u (9 max|taps| + |res|).
dwconv, K x K: dwconv7's rule with K^2 terms, ulp16(ref) / 2 + (K^2 + 1) u sum|x w|.  Moreover bit-exact against the fp32 sum in the kernel's tap order
(bias, then ky, kx ascending; products of fp16 values are exact in fp32, so a fused multiply-add and a product-then-sum round alike; a tap outside the
image adds 0): dw_emulate.
cbam.  First-order propagation of every rounding point, evaluated in float64 next to the reference (cbam_f64):
    avg_c: ceil(P / 16) serial adds per lane, 1 + 8 to combine, the division: d_avg = (ceil(P / 16) + 10) u mean|x_c|;  max_c: exact
    hidden_k = relu(sum_c w1 v + b1), clen-term chunks, NCH partials: d_h = sum|w1| d_v + (clen + NCH + 1) u (sum|w1 v| + |b1|)
    att_c = 2 b2 + sum_k w2 (ha + hm): d_att = sum|w2| (d_ha + d_hm) + (Ch + 3) u (2 |b2| + sum|w2| (|ha| + |hm|))
    sigmoid s(a) through __expf(-a) (relative (2 + 2 |a|) u), 1 + e, 1 / (..): d_s = s (1 - s) (d_a + (2 + 2 |a|) u) + 2 u s
    t = x scale: d_t = |x| d_scale + u |t|;  comp max: max_c d_t;  comp mean: mean_c d_t + (8 ceil(C / 512) + 7) u mean_c|t|
    7 x 7 conv, two taps per lane, six butterfly steps, + bias: d_acc = sum|w7| d_comp + 9 u (sum|w7 comp| + |b7|)
    y = x (1 + scale sg): bound = ulp16(ref) / 2 + |x| (sg d_scale + scale d_sg + 3 u (1 + scale sg))
gru (fp32 out), new_h = f h (1 - u_) + u_ n: sigmoid as above, tanhf within 5 u |tanh| (ddcolor_ops_util, proj2 mode 2), four more roundings:
    bound = |h| (1 - u_) d_f + (f |h| + |n|) d_u + u_ 5 u |n| + 4 u (|f h (1 - u_)| + |u_ n|) + 2^-126 (1 + |h|)
(a sigmoid below the smallest normal fp32 number, 2^-126, may be flushed to zero, and __expf overflows before exp does in float64).
planar_out (fp32 out): act 0 bit-exact; act 1, x^2 + 1: x^2 is exact in fp32, the sum rounds once, so the result is float32(float64(x)^2 + 1) bit for bit;
act 2: d_s + 2^-126; act 3: 5 u |tanh|.  planar_in, cmn_decoder_in: one round-to-nearest-even fp32 -> fp16 conversion, bit-exact (pad channels +0)."""
from dataclasses import dataclass

import numpy as np

from tests.ddcolor_ops_util import bilinear_src
from tests.deoldify_ops_util import LIMIT, SENT, SENTINEL, attn_ratio, bits, f16, finite_patterns, in_view, outside_is_sentinel, pad_to, ulp16  # noqa: F401

U32 = 2.0 ** -24
TINY32 = 2.0 ** -126
F = np.float32
F64 = np.float64


def figure(got, ref, bound, half=True):
    """(max |got - ref| / bound, index of the worst element).  half: the output is fp16 -- an infinity of the reference's sign is accepted where the exact
    value lies within LIMIT x bound of 65520 or beyond"""
    g = np.asarray(got).astype(F64)
    with np.errstate(invalid="ignore"):
        err = np.abs(g - ref)
        err = np.where(np.isnan(err), np.inf, err)
        if half:
            ok_inf = np.isinf(g) & (np.sign(g) == np.sign(ref)) & (np.abs(ref) + LIMIT * bound >= 65520.0)
            err = np.where(ok_inf, 0.0, err)
        ratio = np.where(err == 0, 0.0, err / np.where(bound > 0, bound, np.finfo(F64).tiny))
    worst = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[worst]), tuple(int(i) for i in worst)


def sigmoid64(x):
    x = np.asarray(x, F64)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.where(x >= 0, 1.0 / (1.0 + np.exp(-x)), np.exp(x) / (1.0 + np.exp(x)))


def sigmoid_err(x, s, dx=0.0):
    """d_s of the docstring for the argument x (float64), its exact sigmoid s and an argument error dx"""
    return s * (1.0 - s) * (dx + (2.0 + 2.0 * np.abs(x)) * U32) + 2.0 * U32 * s


def special_halves(shape, seed):
    """finite_patterns with +-0, the smallest subnormals and +-65504 planted"""
    x = finite_patterns(shape, seed).copy()
    flat = x.reshape(-1)
    special = np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x7BFF, 0xFBFF], np.uint16).view(np.float16)
    idx = np.random.default_rng(seed).choice(flat.size, min(flat.size, 4 * len(special)), replace=False)
    flat[idx] = np.resize(special, len(idx))
    return x


# ---- cross-channel attention -------------------------------------------------------------------------------------------------------------------------------------
CG_T, CG_P = 64, 32
CCA_REGIMES = ("flat", "edges")


@dataclass(frozen=True)
class CcaCase:
    name: str
    heads: int
    c: int
    H: int
    W: int
    B: int
    tiles: int                   # what the launcher must choose (asserted before anything runs)
    S: int
    per: int
    zero: bool = False           # an all-zero q channel and an all-zero k channel

    @property
    def P(self):
        return self.H * self.W

    @property
    def C2(self):
        return self.heads * self.c

    @property
    def conv(self):
        return self.C2 % 64 == 0


CCA_CASES = {c.name: c for c in (
    CcaCase("c64", 8, 64, 3, 43, 2, 1, 2, 65, zero=True),          # chunks 32, 32, 1
    CcaCase("c72", 8, 72, 9, 15, 1, 2, 2, 68),                     # the last tile is 8 channels wide
    CcaCase("c128", 8, 128, 14, 28, 1, 2, 4, 98),                  # the product's smallest Fuse grid
    CcaCase("c256", 2, 256, 16, 24, 2, 4, 3, 128),                 # the upper limit of c
    CcaCase("c8", 1, 8, 25, 40, 1, 1, 8, 125),                     # many splits, no conv, a matrix row that is no multiple of 64
    CcaCase("one", 1, 8, 1, 1, 2, 1, 1, 1))}                       # degenerate: one pixel, every cosine is +-1


def cca_choice(P, heads, c):
    """(tiles per side, S, pixels per split) of launch_chan_attn / chan_attn_splits (csrc/colormnet_net.hip), restated"""
    tiles = (c + CG_T - 1) // CG_T
    blocks = heads * tiles * tiles
    S = max(1, min((512 + blocks - 1) // blocks, (P + 127) // 128))
    return tiles, S, (P + S - 1) // S


def cca_edge_pixels(P, S):
    """both sides of every split boundary, of every 32-pixel staging boundary inside a split, and the last pixel"""
    per = (P + S - 1) // S
    out = {P - 1}
    for sp in range(S):
        lo, hi = sp * per, min(P, sp * per + per)
        if lo >= hi:
            continue
        out |= {hi - 1, lo} | ({lo - 1} if lo else set())
        for p0 in range(lo + CG_P, hi, CG_P):
            out |= {p0 - 1, p0}
    return sorted(out)


def cca_inputs(case, regime):
    """fp16 q, k, v [B][P][C2] and float32 temperatures [heads] from 3 to 12.  edges: 98 % and more of every channel's energy on cca_edge_pixels"""
    r = np.random.default_rng([31, case.heads, case.c, case.P, sum(map(ord, regime))])
    shape = (case.B, case.P, case.C2)
    q, k, v = (r.standard_normal(shape) for _ in range(3))
    if regime == "edges" and case.P > 1:
        amp = np.full(case.P, 0.03)
        amp[cca_edge_pixels(case.P, case.S)] = 4.0
        q, k = q * amp[None, :, None], k * amp[None, :, None]
    q, k, v = f16(q), f16(k), f16(v)
    if case.zero:
        q[:, :, 3] = 0
        k[:, :, case.c + 5] = 0
        k[:, :, 3] = np.where(np.arange(case.P) % 2 == 0, 0.0, -0.0).astype(np.float16)[None]
    temp = np.linspace(3.0, 12.0, case.heads).astype(F) if case.heads > 1 else np.array([12.0], F)
    return q, k, v, temp


def cca_reference(q, k, temp, heads):
    """float64 softmax_j(normalize(q)_i . normalize(k)_j x temperature) per frame and head, F.normalize's eps -> (W [B][heads][c][c], cos)"""
    B, P, C2 = q.shape
    c = C2 // heads
    q64, k64 = (a.astype(F64).reshape(B, P, heads, c) for a in (q, k))
    eps = float(F(1e-12))
    qn = q64 / np.maximum(np.sqrt((q64 ** 2).sum(1, keepdims=True)), eps)
    kn = k64 / np.maximum(np.sqrt((k64 ** 2).sum(1, keepdims=True)), eps)
    cos = np.einsum("bphi,bphj->bhij", qn, kn)
    s = cos * temp.astype(F64)[None, :, None, None]
    e = np.exp(s - s.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True), cos


def cca_bound(W, temp, per, S):
    t = np.abs(temp.astype(F64))[None, :, None, None]
    return ulp16(W) / 2 + U32 * W * (2 * t * (2 * (per + S) + 6) + 2 * (2 + 4 * t) + 9)


def cca_blocks(Wfull, heads, c):
    """the diagonal blocks [B][heads][c][c] of a matrix image [B][rows][pitch]"""
    return np.stack([Wfull[:, h * c:(h + 1) * c, h * c:(h + 1) * c] for h in range(heads)], 1)


def cca_emulate(case, q, k, temp, defect=None):
    """chan_gram_kernel + chan_softmax_kernel in numpy float32: per split the pixels one after the other (the 32-pixel staging chunks change nothing about
    the order), the splits added in order, norms likewise, float32 softmax, one fp16 store.  defect: "drop_last_pixel" = split 0 stops one pixel early;
    "skip_tile_cols" = the Gram columns of the second 64-channel tile stay 0"""
    B, P, C2 = q.shape
    heads, c = case.heads, case.c
    tiles, S, per = cca_choice(P, heads, c)
    qf, kf = (a.astype(F).reshape(B, P, heads, c) for a in (q, k))
    G, nq, nk = np.zeros((B, heads, c, c), F), np.zeros((B, heads, c), F), np.zeros((B, heads, c), F)
    for sp in range(S):
        lo, hi = sp * per, min(P, sp * per + per)
        if defect == "drop_last_pixel" and sp == 0:
            hi -= 1
        g, a, b = np.zeros_like(G), np.zeros_like(nq), np.zeros_like(nk)
        for p in range(lo, hi):
            g += qf[:, p, :, :, None] * kf[:, p, :, None, :]
            a += qf[:, p] * qf[:, p]
            b += kf[:, p] * kf[:, p]
        G, nq, nk = G + g, nq + a, nk + b
    if defect == "skip_tile_cols":
        G[..., CG_T:2 * CG_T] = 0
    eps = F(1e-12)
    v = G / (np.maximum(np.sqrt(nq), eps)[..., None] * np.maximum(np.sqrt(nk), eps)[:, :, None, :]) * temp.astype(F)[None, :, None, None]
    ex = np.exp(v - v.max(-1, keepdims=True), dtype=F)
    return (ex / ex.sum(-1, keepdims=True, dtype=F)).astype(np.float16)


def cca_apply_f64(Wblocks, v, bound_w=None):
    """attn @ v per head: Wblocks [B][heads][c][c] (any dtype), v [B][P][C2] -> (ref [B][P][C2], sum |W v|, sum bound_w |v| or 0)"""
    B, heads, c, _ = Wblocks.shape
    v64 = v.astype(F64).reshape(B, -1, heads, c)
    W64 = np.asarray(Wblocks).astype(F64)
    ref = np.einsum("bhij,bphj->bphi", W64, v64).reshape(v.shape)
    mag = np.einsum("bhij,bphj->bphi", np.abs(W64), np.abs(v64)).reshape(v.shape)
    extra = np.einsum("bhij,bphj->bphi", bound_w, np.abs(v64)).reshape(v.shape) if bound_w is not None else 0.0
    return ref, mag, extra


def cca_layout(case):
    C2 = case.C2
    if case.conv:
        return dict(q_pitch=C2 + 16, q_coff=8, kv_pitch=2 * C2 + 64, k_coff=8, v_coff=C2 + 64, w_pitch=C2, w_rows=C2 + 8, o_pitch=C2 + 128, o_coff=64)
    return dict(q_pitch=C2 + 16, q_coff=8, kv_pitch=C2 + 24, k_coff=16, v_coff=0, w_pitch=C2 + 8, w_rows=C2 + 8, o_pitch=0, o_coff=0)


def run_cca(ctx, case, q, k, v, temp):
    """one HAVC_OP_CHAN_ATTN (+ the W_FROM_BUF conv where C2 % 64 == 0) -> (matrix image [B][C2 + 8][w_pitch], conv destination [B][P][o_pitch] or None).
    The matrix buffer starts as +0 off the diagonal blocks (the op never writes there and the conv reads it) and as the sentinel on the diagonal blocks, on the
    eight rows past the matrix and on the columns past it"""
    from tests.gpu_util import run_plan
    from vsdeoldify_amd.plan import PlanBuilder, View, WeightPack
    lay, C2, P, H, W = cca_layout(case), case.C2, case.P, case.H, case.W
    assert cca_choice(P, case.heads, case.c) == (case.tiles, case.S, case.per), "the launcher's rule no longer selects the path this case is named for"
    pack, b = WeightPack(), PlanBuilder()
    qv = View(b.buf(P * lay["q_pitch"]), lay["q_coff"], lay["q_pitch"], H, W, C2, C2)
    kvb = b.buf(P * lay["kv_pitch"])
    wbuf = b.buf(lay["w_rows"] * lay["w_pitch"])
    b.chan_attn("attn", qv, View(kvb, lay["k_coff"], lay["kv_pitch"], H, W, C2, C2), case.heads, pack.add(temp.astype(F)), wbuf, lay["w_pitch"] // 8,
                b.buf(case.heads * case.S * case.c * case.c, 4), b.buf(case.S * 2 * C2, 4))
    wimg = np.full((case.B, lay["w_rows"], lay["w_pitch"]), SENTINEL, np.float16)
    wimg[:, :C2, :C2] = 0
    for h in range(case.heads):
        wimg[:, h * case.c:(h + 1) * case.c, h * case.c:(h + 1) * case.c] = SENTINEL
    r = np.random.default_rng(9)
    kvimg = f16(r.standard_normal((case.B, P, lay["kv_pitch"])))
    kvimg[..., lay["k_coff"]:lay["k_coff"] + C2] = k
    ups = {qv.buf: in_view(q, lay["q_pitch"], lay["q_coff"], fill=np.float16(3.0)), kvb: kvimg, wbuf: wimg}
    dl = {wbuf: (wimg.shape, np.float16)}
    if case.conv:
        kvimg[..., lay["v_coff"]:lay["v_coff"] + C2] = v
        ov = View(b.buf(P * lay["o_pitch"]), lay["o_coff"], lay["o_pitch"], H, W, C2, C2)
        b.conv_dyn("attn@v", View(kvb, lay["v_coff"], lay["kv_pitch"], H, W, C2, C2), View(wbuf, 0, C2, 1, lay["w_rows"], C2, C2), ov, C2)
        oimg = np.full((case.B, P, lay["o_pitch"]), SENTINEL, np.float16)
        ups[ov.buf] = oimg
        dl[ov.buf] = (oimg.shape, np.float16)
    out = run_plan(ctx, pack, b, ups, dl, case.B)
    return out[wbuf], (out[ov.buf] if case.conv else None)


def cca_matrix_untouched(Wfull, case):
    """off the diagonal blocks the matrix still holds +0, past the matrix the sentinel"""
    C2, c = case.C2, case.c
    inner = bits(Wfull[:, :C2, :C2]).copy()
    for h in range(case.heads):
        inner[:, h * c:(h + 1) * c, h * c:(h + 1) * c] = 0
    return not inner.any() and bool((bits(Wfull[:, C2:]) == SENT).all()) and bool((bits(Wfull[:, :, C2:]) == SENT).all())


# ---- multi-head self-attention, head dim 64 --------------------------------------------------------------------------------------------------------------------------
M64_KT, D64 = 64, 64
MHA_SCALE = F(0.125)
MHA_REGIMES = ("flat", "sharp", "edges", "rising")
MHA_LS = (1, 15, 64, 65, 128, 513)


@dataclass(frozen=True)
class Mha64Case:
    name: str
    heads: int
    L: int
    B: int = 2
    layout: str = "wide"         # "wide": q / k / v at channel offsets of a wider row, L + 5 token rows per frame (live < tokens per frame, the surplus rows
    #                              hold +-60000), the output at channel offset 16; "dense": [q | k | v] rows of 3 E channels, live = tokens per frame

    @property
    def E(self):
        return self.heads * D64

    @property
    def regimes(self):
        return tuple(r for r in MHA_REGIMES if r != "rising" or self.L > M64_KT)


MHA_CASES = {c.name: c for c in [Mha64Case(f"h{h}l{L}", h, L) for h in (6, 2) for L in MHA_LS] + [Mha64Case("dense65", 6, 65, 2, "dense")]}


def mha64_edge_keys(L):
    """{0, 63, 64, 127, 128, ..., L - 1}"""
    return sorted({0, L - 1} | {k for m in range(M64_KT, L + 1, M64_KT) for k in (m - 1, m) if k < L})


def mha64_targets(case, regime, k):
    """int [B][heads][L]: the key that query (b, h, i) leans on -- edges: cycling over mha64_edge_keys; sharp: the keys of largest norm that are no edge"""
    B, H, L = case.B, case.heads, case.L
    edges = np.array(mha64_edge_keys(L))
    if regime == "edges":
        return edges[np.arange(B * H * L) % len(edges)].reshape(B, H, L)
    norm = (k.reshape(B, L, H, D64).astype(F64) ** 2).sum(-1).transpose(0, 2, 1)
    if L > len(edges):
        norm[:, :, edges] = -1.0
    order = np.argsort(-norm, axis=-1, kind="stable")[:, :, :max(1, min(L, L - len(edges) if L > len(edges) else L))]
    return order[:, :, np.arange(L) % order.shape[-1]]


def mha64_inputs(case, regime):
    """fp16 q, k, v [B][L][E].  flat: scores within +-1; sharp: one dominant key per query (score 60); edges: query i puts about half of its weight on
    edge key e(i); rising: the largest score of every 64-key tile lies 20 and more above the previous tile's, so every rescale matters"""
    B, H, L, E = case.B, case.heads, case.L, case.E
    r = np.random.default_rng([37, B, H, L, sum(map(ord, regime))])
    k, v = f16(r.standard_normal((B, L, E))), f16(r.standard_normal((B, L, E)))
    if regime == "flat":
        return f16(0.1 * r.standard_normal((B, L, E))), k, v
    if regime == "rising":
        u = r.standard_normal(D64)
        u /= np.linalg.norm(u)
        level = 24.0 * (np.arange(L) // M64_KT)[None, :, None, None]
        kk = level * u + 0.1 * r.standard_normal((B, L, H, D64))
        qq = (r.uniform(1.0, 1.1, (B, L, H, 1)) * u + 0.02 * r.standard_normal((B, L, H, D64))) / float(MHA_SCALE)
        return f16(qq.reshape(B, L, E)), f16(kk.reshape(B, L, E)), v
    tgt = mha64_targets(case, regime, k)
    kh = k.reshape(B, L, H, D64).transpose(0, 2, 1, 3)
    ksel = np.take_along_axis(kh, tgt[..., None], axis=2).astype(F64)
    unit = ksel / (ksel ** 2).sum(-1, keepdims=True)                   # k_t / |k_t|^2: the score of the target is a, exactly
    if regime == "sharp":
        a = np.full((B, H, L), 60.0)
    else:
        t = unit.astype(F) @ kh.astype(F).transpose(0, 1, 3, 2)
        np.put_along_axis(t, tgt[..., None], -np.inf, axis=-1)
        lo, hi = np.zeros((B, H, L), F), np.full((B, H, L), 30.0, F)
        if L > 1:
            for _ in range(14):                                        # a with exp(a) = sum_{j != e} exp(a t_j): half of the weight on key e
                mid = (lo + hi) / 2
                with np.errstate(over="ignore"):
                    more = np.exp(mid[..., None] * t).sum(-1) > np.exp(mid)
                lo, hi = np.where(more, mid, lo), np.where(more, hi, mid)
        a = ((lo + hi) / 2).astype(F64) if L > 1 else np.zeros((B, H, L))
    q = (a / float(MHA_SCALE))[..., None] * unit
    return f16(q.transpose(0, 2, 1, 3).reshape(B, L, E)), k, v


def mha64_reference(q, k, v, heads, tgt=None):
    """float64 softmax(scale q . k) v per head -> dict(out, A [B][L][E], smax, pmax [B][heads][L], ptgt, tmax [B][heads][L][tiles] = largest score per tile)"""
    B, L, E = q.shape
    qh, kh, vh = (a.astype(F64).reshape(B, L, heads, D64).transpose(0, 2, 1, 3) for a in (q, k, v))
    s = float(MHA_SCALE) * (qh @ kh.transpose(0, 1, 3, 2))
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    back = lambda a: a.transpose(0, 2, 1, 3).reshape(B, L, E)          # noqa: E731
    tiles = (L + M64_KT - 1) // M64_KT
    return dict(out=back(p @ vh), A=back(p @ np.abs(vh)), smax=float(np.abs(s).max()), pmax=p.max(-1),
                ptgt=np.take_along_axis(p, tgt[..., None], axis=-1)[..., 0] if tgt is not None else None,
                tmax=np.stack([s[..., t * M64_KT:(t + 1) * M64_KT].max(-1) for t in range(tiles)], -1))


def mha64_check_regime(case, regime, ref):
    """the property the regime is named for, from the reference alone"""
    if regime == "flat":
        assert ref["smax"] < 1.0, ref["smax"]
    elif regime == "sharp":
        assert case.L == 1 or (ref["pmax"].min() > 0.5 and np.median(ref["pmax"]) > 0.999), (ref["pmax"].min(), np.median(ref["pmax"]))
    elif regime == "rising":
        step = np.diff(ref["tmax"], axis=-1)
        assert case.L > M64_KT and (step >= 20.0).all(), step.min()
    elif case.L > 1:
        p = ref["ptgt"]
        half = (p > 0.4) & (p < 0.6)
        tgt = mha64_targets(case, "edges", None)
        assert half.mean() >= 0.98 and all(half[tgt == e].any() for e in mha64_edge_keys(case.L)), (float(half.mean()), float(p.min()), float(p.max()))


def mha64_emulate(q, k, v, heads, defect=None):
    """mha64_kernel in numpy: 64-key tiles, float32 scores and running (m, l, O), P rounded to fp16 into the second product, one fp16 store.
    defect: "no_rescale" = the last tile's rescale of (l, O) omitted (any earlier one is forgotten where a later tile dominates); "drop_key64" = key 64
    masked out"""
    B, L, E = q.shape
    qh, kh, vh = (a.astype(F).reshape(B, L, heads, D64).transpose(0, 2, 1, 3) for a in (q, k, v))
    m, l, o = np.full((B, heads, L), -np.inf, F), np.zeros((B, heads, L), F), np.zeros((B, heads, L, D64), F)
    last = (L - 1) // M64_KT
    for ti, k0 in enumerate(range(0, L, M64_KT)):
        s = (qh @ kh[:, :, k0:k0 + M64_KT].transpose(0, 1, 3, 2)) * MHA_SCALE
        if defect == "drop_key64" and ti == 1:
            s[..., 0] = -np.inf
        mn = np.maximum(m, s.max(-1))
        corr = np.exp(m - mn, dtype=F)
        if defect == "no_rescale" and ti == last:
            corr = np.ones_like(corr)
        p = np.exp(s - mn[..., None], dtype=F)
        l = l * corr + p.sum(-1, dtype=F)
        o = o * corr[..., None] + p.astype(np.float16).astype(F) @ vh[:, :, k0:k0 + M64_KT]
        m = mn
    return (o * (F(1.0) / l)[..., None]).astype(np.float16).transpose(0, 2, 1, 3).reshape(B, L, E)


def mha64_layout(case):
    E, L = case.E, case.L
    if case.layout == "dense":
        return dict(tok=L, pitch=3 * E, q_coff=0, k_coff=E, v_coff=2 * E, y_pitch=E + 24, y_coff=16)
    return dict(tok=L + 5, pitch=3 * E + 40, q_coff=8, k_coff=E + 16, v_coff=2 * E + 32, y_pitch=E + 24, y_coff=16)


def run_mha64(ctx, case, q, k, v):
    """one HAVC_OP_MHA64 -> (out [B][L][E], the whole destination [B][tok][y_pitch], sentinel-filled before the run).  Channels outside q / k / v hold random
    values, the token rows past L hold +-60000"""
    from tests.gpu_util import run_plan
    from vsdeoldify_amd.plan import PlanBuilder, View, WeightPack
    lay, E, L, B = mha64_layout(case), case.E, case.L, case.B
    b = PlanBuilder()
    qv = View(b.buf(lay["tok"] * lay["pitch"]), 0, lay["pitch"], 1, lay["tok"], lay["pitch"], lay["pitch"])
    yv = View(b.buf(lay["tok"] * lay["y_pitch"]), lay["y_coff"], lay["y_pitch"], 1, lay["tok"], E, E)
    b.mha64("mha64", qv, lay["q_coff"], lay["k_coff"], lay["v_coff"], yv, case.heads, L, float(MHA_SCALE))
    r = np.random.default_rng(7)
    img = f16(r.standard_normal((B, lay["tok"], lay["pitch"])))
    img[:, L:] = np.where(r.integers(0, 2, (B, lay["tok"] - L, lay["pitch"])) == 1, 60000.0, -60000.0)
    for a, off in ((q, lay["q_coff"]), (k, lay["k_coff"]), (v, lay["v_coff"])):
        img[:, :L, off:off + E] = a
    dst = np.full((B, lay["tok"], lay["y_pitch"]), SENTINEL, np.float16)
    full = run_plan(ctx, WeightPack(), b, {qv.buf: img, yv.buf: dst}, {yv.buf: (dst.shape, np.float16)}, B)[yv.buf]
    return full[:, :L, lay["y_coff"]:lay["y_coff"] + E], full


def mha64_untouched(full, case):
    return bool((bits(full[:, case.L:]) == SENT).all()) and outside_is_sentinel(full[:, :case.L], 16, case.E)


# ---- ew ------------------------------------------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class EwCase:
    name: str
    src: tuple
    dst: tuple
    mode: int = 0                # 0 copy, 1 bilinear, 2 area
    factor: int = 1
    res: str = ""                # "", "frame" (one residual per frame), "bcast" (frame 0's for every frame)
    src_bcast: bool = False
    relu: bool = False
    dual: bool = False

    @property
    def ratio(self):
        """source / destination in float32, as aten computes it for a given size (1 / scale_factor is the same number for 2 and 4)"""
        return (F(self.src[0]) / F(self.dst[0]), F(self.src[1]) / F(self.dst[1])) if self.mode == 1 else (F(1), F(1))

    @property
    def exact(self):
        return self.mode == 0 and not self.res


EW_CASES = {c.name: c for c in (
    EwCase("up2_res_bcast_dual", (5, 7), (10, 14), 1, res="bcast", dual=True),      # upsample_groups + skip, with the rectified copy
    EwCase("up2_res_frame", (5, 7), (10, 14), 1, res="frame"),
    EwCase("up4", (3, 5), (12, 20), 1),                                             # upsample4, logits_x4
    EwCase("frac_8_7", (8, 16), (7, 14), 1),                                        # the Segmentor's 1 / 14 -> 1 / 16 grid
    EwCase("down", (9, 11), (5, 6), 1),
    EwCase("area2", (6, 10), (3, 5), 2, 2),                                         # g8_area
    EwCase("area4", (12, 20), (3, 5), 2, 4),
    EwCase("area2_res", (6, 10), (3, 5), 2, 2, res="frame"),
    EwCase("copy", (5, 7), (5, 7)),                                                 # hidden_in: a copy between views at offsets
    EwCase("copy_relu", (5, 7), (5, 7), relu=True),                                 # pred.relu
    EwCase("copy_dual", (5, 7), (5, 7), dual=True),
    EwCase("copy_src_bcast_dual", (5, 7), (5, 7), src_bcast=True, dual=True),
    EwCase("copy_res_frame", (5, 7), (5, 7), res="frame"),
    EwCase("copy_res_bcast_relu", (5, 7), (5, 7), res="bcast", relu=True))}
EW_CHANNELS = (8, 24)
EW_B = 2


def ew_inputs(case, C, kind):
    """x [B][Hi][Wi][C], res [B][Ho][Wo][C] or None, fp16; kind "random" or "patterns" (special_halves: +-0, subnormals, +-65504, sums that overflow)"""
    seed = [41, C, sum(map(ord, case.name)), sum(map(ord, kind))]
    r = np.random.default_rng(seed)
    mk = (lambda shape, s: special_halves(shape, seed + [s])) if kind == "patterns" else (lambda shape, s: f16(2.0 * r.standard_normal(shape)))
    x = mk((EW_B,) + case.src + (C,), 0)
    res = mk((EW_B,) + case.dst + (C,), 1) if case.res else None
    return x, res


def ew_f64(case, x, res, how="fma"):
    """-> (ref of y before the fp16 store [B][Ho][Wo][C] float64, bound); the rectified twin is max(ref of the UNrectified value, 0)"""
    x64 = x.astype(F64)
    if case.src_bcast:
        x64 = np.broadcast_to(x64[:1], x64.shape)
    Ho, Wo = case.dst
    if case.mode == 1:
        y0, y1, ly = bilinear_src(case.src[0], Ho, how)
        x0, x1, lx = bilinear_src(case.src[1], Wo, how)
        ly, lx = ly.astype(F64)[None, :, None, None], lx.astype(F64)[None, None, :, None]
        p00, p01, p10, p11 = x64[:, y0][:, :, x0], x64[:, y0][:, :, x1], x64[:, y1][:, :, x0], x64[:, y1][:, :, x1]
        v = (1 - ly) * (1 - lx) * p00 + (1 - ly) * lx * p01 + ly * (1 - lx) * p10 + ly * lx * p11
        mag, k = np.max(np.abs([p00, p01, p10, p11]), axis=0), 8.0
    elif case.mode == 2:
        f = case.factor
        blk = x64.reshape(x64.shape[0], Ho, f, Wo, f, -1)
        v, mag, k = blk.mean((2, 4)), np.abs(blk).mean((2, 4)), f * f + 1.0
    else:
        v, mag, k = x64, np.abs(x64), 0.0
    err = U32 * k * mag
    if case.res:
        r64 = res.astype(F64)
        if case.res == "bcast":
            r64 = np.broadcast_to(r64[:1], r64.shape)
        err = err + U32 * (mag + np.abs(r64))
        v = v + r64
    return v, ulp16(v) / 2 + err


def ew_emulate(case, x, res, how="fma"):
    """ew_kernel's float32 arithmetic in numpy -> the value before the store as float32"""
    xf = x.astype(F)
    if case.src_bcast:
        xf = np.broadcast_to(xf[:1], xf.shape)
    Ho, Wo = case.dst
    if case.mode == 1:
        y0, y1, ly = bilinear_src(case.src[0], Ho, how)
        x0, x1, lx = bilinear_src(case.src[1], Wo, how)
        ly, lx = ly.astype(F)[None, :, None, None], lx.astype(F)[None, None, :, None]
        one = F(1)
        v = ((one - ly) * (one - lx)) * xf[:, y0][:, :, x0] + ((one - ly) * lx) * xf[:, y0][:, :, x1]
        v = v + (ly * (one - lx)) * xf[:, y1][:, :, x0]
        v = v + (ly * lx) * xf[:, y1][:, :, x1]
    elif case.mode == 2:
        f = case.factor
        blk = xf.reshape(xf.shape[0], Ho, f, Wo, f, -1)
        v = np.zeros((xf.shape[0], Ho, Wo, xf.shape[-1]), F)
        for dy in range(f):
            for dx in range(f):
                v = v + blk[:, :, dy, :, dx]
        v = v * (F(1) / F(f * f))
    else:
        v = xf
    if case.res:
        rf = res.astype(F)
        v = v + (np.broadcast_to(rf[:1], rf.shape) if case.res == "bcast" else rf)
    return v.astype(F)


def run_ew(ctx, case, x, res):
    """one HAVC_OP_EW: x at channel offset 8 of a C + 16 row, y at 16 of C + 24, the residual at 8 of C + 16, the rectified twin at 24 of C + 32.  A broadcast
    source / residual holds 3000 in its frames past the first (nothing may read them) -> (y, whole y buffer, y2 or None, whole y2 buffer or None)"""
    from tests.gpu_util import run_plan
    from vsdeoldify_amd.plan import PlanBuilder, View, WeightPack
    B, Hi, Wi, C = x.shape
    Ho, Wo = case.dst
    b = PlanBuilder()
    xv = View(b.buf(Hi * Wi * (C + 16)), 8, C + 16, Hi, Wi, C, C)
    yv = View(b.buf(Ho * Wo * (C + 24)), 16, C + 24, Ho, Wo, C, C)
    xs = x.copy()
    if case.src_bcast:
        xs[1:] = np.float16(3000.0)
    dst = np.full((B, Ho, Wo, C + 24), SENTINEL, np.float16)
    ups, dl = {xv.buf: in_view(xs, C + 16, 8), yv.buf: dst}, {yv.buf: (dst.shape, np.float16)}
    rv = dv = None
    if case.res:
        rv = View(b.buf(Ho * Wo * (C + 16)), 8, C + 16, Ho, Wo, C, C)
        rs = res.copy()
        if case.res == "bcast":
            rs[1:] = np.float16(3000.0)
        ups[rv.buf] = in_view(rs, C + 16, 8)
    if case.dual:
        dv = View(b.buf(Ho * Wo * (C + 32)), 24, C + 32, Ho, Wo, C, C)
        d2 = np.full((B, Ho, Wo, C + 32), SENTINEL, np.float16)
        ups[dv.buf], dl[dv.buf] = d2, (d2.shape, np.float16)
    b.ew("ew", xv, yv, mode=case.mode, ratio=tuple(float(t) for t in case.ratio), factor=case.factor, res=rv, src_bcast=case.src_bcast,
         res_bcast=case.res == "bcast", relu=case.relu, dual=dv)
    out = run_plan(ctx, WeightPack(), b, ups, dl, B)
    full = out[yv.buf]
    full2 = out[dv.buf] if case.dual else None
    return full[..., 16:16 + C], full, (full2[..., 24:24 + C] if case.dual else None), full2


def relu16(a):
    """fmaxf(v, 0) of a stored fp16 value: negative values and -0 become +0"""
    a = np.asarray(a, np.float16)
    return np.where(a > 0, a, np.float16(0.0)).astype(np.float16)


# ---- depthwise K x K -----------------------------------------------------------------------------------------------------------------------------------------------------
DW_COLS, DW_ROWS = 4, 8
DW_SHAPES = tuple((h, w) for h in (1, 7, 8, 9) for w in (1, 3, 4, 5)) + ((17, 9),)          # K = 3: the strip tails in both directions, a third row band
DW5_SHAPES = ((1, 1), (2, 3), (4, 4), (3, 9), (9, 11))                                        # K = 5: H and W below 5, and above
DW_CHANNELS = (8, 40)


def dw_kernel(K):
    """launch_dwconv's choice, restated: every 3 x 3 runs on the strip kernel, 5 x 5 on the per-pixel one, nothing else is launched"""
    return {3: "dwconv3_strip_kernel", 5: "dwconv_kernel<5>"}[K]


def dw_params(C, K, seed=0):
    """fp16-exact weights [C][K][K] (float32) and a float32 bias"""
    r = np.random.default_rng([43, C, K, seed])
    return f16(r.standard_normal((C, K, K)) / K).astype(F), (0.1 * r.standard_normal(C)).astype(F)


def dw_inputs(H, W, C, kind="random", B=2):
    if kind == "patterns":
        return special_halves((B, H, W, C), [47, H, W, C])
    return f16(np.random.default_rng([47, H, W, C]).standard_normal((B, H, W, C)))


def dwconv_f64(x, w, bias=None):
    """float64 depthwise K x K cross-correlation, zero padding K / 2: x [B][H][W][C], w [C][K][K] -> (ref, sum |x w|)"""
    B, H, W, C = x.shape
    K = w.shape[-1]
    xp = np.zeros((B, H + K - 1, W + K - 1, C))
    xp[:, K // 2:K // 2 + H, K // 2:K // 2 + W] = x.astype(F64)
    w64 = w.astype(F64)
    ref, mag = np.zeros((B, H, W, C)), np.zeros((B, H, W, C))
    for ky in range(K):
        for kx in range(K):
            win = xp[:, ky:ky + H, kx:kx + W]
            ref += win * w64[:, ky, kx]
            mag += np.abs(win * w64[:, ky, kx])
    return (ref + bias.astype(F64) if bias is not None else ref), mag


def dw_bound(ref, mag, K):
    return ulp16(ref) / 2 + (K * K + 1) * U32 * mag


def dw_emulate(x, w, bias=None, defect=None):
    """the kernels' float32 sum in their tap order (bias, then ky, kx ascending; a tap outside the image adds 0), one fp16 store.
    defect: "skip_last_col" = the last column of every 4-column strip group is not computed (stays 0)"""
    B, H, W, C = x.shape
    K = w.shape[-1]
    xp = np.zeros((B, H + K - 1, W + K - 1, C), F)
    xp[:, K // 2:K // 2 + H, K // 2:K // 2 + W] = x.astype(F)
    acc = np.zeros((B, H, W, C), F) + (bias.astype(F) if bias is not None else F(0))
    with np.errstate(over="ignore", invalid="ignore"):
        for ky in range(K):
            for kx in range(K):
                acc = acc + xp[:, ky:ky + H, kx:kx + W] * w[:, ky, kx].astype(F)
        out = acc.astype(np.float16)
    if defect == "skip_last_col":
        out[:, :, DW_COLS - 1::DW_COLS] = 0
    return out


def run_dwconv(ctx, x, w, bias=None):
    """one HAVC_OP_DWCONV: x at channel offset 8 of a C + 16 row, y at 16 of C + 24; weights fp16 [K K][C + 8] (tap-major, a pitch wider than C), bias fp32"""
    from tests.gpu_util import run_plan
    from vsdeoldify_amd.plan import PlanBuilder, View, WeightPack
    B, H, W, C = x.shape
    K = w.shape[-1]
    pack, b = WeightPack(), PlanBuilder()
    xv, yv = View(b.buf(H * W * (C + 16)), 8, C + 16, H, W, C, C), View(b.buf(H * W * (C + 24)), 16, C + 24, H, W, C, C)
    wp = np.full((K * K, C + 8), 1000.0, np.float16)
    wp[:, :C] = w.reshape(C, K * K).T
    b.dwconv("dw", xv, yv, pack.add(wp), pack.add(bias.astype(F)) if bias is not None else -1, C + 8, K)
    dst = np.full((B, H, W, C + 24), SENTINEL, np.float16)
    full = run_plan(ctx, pack, b, {xv.buf: in_view(x, C + 16, 8), yv.buf: dst}, {yv.buf: (dst.shape, np.float16)}, B)[yv.buf]
    return full[..., 16:16 + C], full


# ---- cbam ------------------------------------------------------------------------------------------------------------------------------------------------------------------
CBAM_CHANNELS = (16, 48, 64, 576, 1024)
CBAM_CHOICE = {16: (16, 4), 48: (16, 4), 64: (16, 4), 576: (14, 44), 1024: (8, 128)}          # C -> (NCH, clen) that cbam_mlp_kernel must arrive at
CBAM_GRIDS = ((1, 1), (3, 5), (6, 9))
CBAM_TAIL_P = tuple(range(1, 18))
CBAM_B = 2


def cbam_choice(C, threads=512):
    """(NCH, clen) of cbam_mlp_kernel, restated: chunks per hidden unit (<= 16) and channels per chunk (a multiple of 4)"""
    Ch = C // 16
    n = threads // Ch
    NCH = (16 if n > 16 else n) if n > 0 else 1
    return NCH, ((C + NCH - 1) // NCH + 3) & ~3


def cbam_params(C, seed=0):
    """float32 (w1 [Ch][C], b1 [Ch], w2 [C][Ch], b2 [C], w7 [2][7][7], b7 [1])"""
    r = np.random.default_rng([53, C, seed])
    Ch = C // 16
    g = lambda s, *shape: (s * r.standard_normal(shape)).astype(F)          # noqa: E731
    return g(1.5 / np.sqrt(C), Ch, C), g(0.1, Ch), g(1.0 / np.sqrt(Ch), C, Ch), g(0.1, C), g(0.2, 2, 7, 7), g(0.1, 1)


def cbam_inputs(C, H, W, B=CBAM_B):
    """fp16 [B][H][W][C], different data per frame, a few +-0 among them"""
    r = np.random.default_rng([59, C, H, W])
    x = f16(r.standard_normal((B, H, W, C)))
    x.reshape(-1)[::97] = np.float16(-0.0)
    return x


def _conv7_f64(comp, w7):
    """comp [B][H][W][2] float64, w7 [2][7][7] -> (sum over the valid taps, sum of |terms|)"""
    B, H, W, _ = comp.shape
    cp = np.zeros((B, H + 6, W + 6, 2))
    cp[:, 3:3 + H, 3:3 + W] = comp
    acc, mag = np.zeros((B, H, W)), np.zeros((B, H, W))
    for ch in range(2):
        for ky in range(7):
            for kx in range(7):
                t = cp[:, ky:ky + H, kx:kx + W, ch] * float(w7[ch, ky, kx])
                acc += t
                mag += np.abs(t)
    return acc, mag


def cbam_f64(x, params):
    """float64 x + CBAM(x) = x (1 + scale_c sg_p) and the bound of the module docstring -> (ref [B][H][W][C], bound)"""
    w1, b1, w2, b2, w7, b7 = (np.asarray(a, F64) for a in params)
    B, H, W, C = x.shape
    P, Ch = H * W, C // 16
    NCH, clen = cbam_choice(C)
    x64 = x.astype(F64)
    xa = np.abs(x64)
    avg, mx = x64.mean((1, 2)), x64.max((1, 2))
    d_avg = ((P + 15) // 16 + 10) * U32 * xa.mean((1, 2))
    k1 = (clen + NCH + 1) * U32
    ha, hm = np.maximum(avg @ w1.T + b1, 0), np.maximum(mx @ w1.T + b1, 0)
    d_ha = d_avg @ np.abs(w1).T + k1 * (np.abs(avg) @ np.abs(w1).T + np.abs(b1))
    d_hm = k1 * (np.abs(mx) @ np.abs(w1).T + np.abs(b1))
    att = 2 * b2 + (ha + hm) @ w2.T
    d_att = (d_ha + d_hm) @ np.abs(w2).T + (Ch + 3) * U32 * (2 * np.abs(b2) + (ha + hm) @ np.abs(w2).T)
    scale = sigmoid64(att)
    d_scale = sigmoid_err(att, scale, d_att)
    t = x64 * scale[:, None, None]
    d_t = xa * d_scale[:, None, None] + U32 * np.abs(t)
    comp = np.stack([t.max(-1), t.mean(-1)], -1)
    d_comp = np.stack([d_t.max(-1), d_t.mean(-1) + (8 * ((C + 511) // 512) + 7) * U32 * np.abs(t).mean(-1)], -1)
    acc, mag = _conv7_f64(comp, w7)
    d_acc = _conv7_f64(d_comp, np.abs(w7))[0] + 9 * U32 * (mag + abs(float(b7[0])))
    acc = acc + float(b7[0])
    sg = sigmoid64(acc)
    d_sg = sigmoid_err(acc, sg, d_acc)
    gate = scale[:, None, None] * sg[..., None]
    ref = x64 * (1 + gate)
    bound = ulp16(ref) / 2 + xa * (sg[..., None] * d_scale[:, None, None] + scale[:, None, None] * d_sg[..., None] + 3 * U32 * (1 + gate))
    return ref, bound


def cbam_emulate(x, params, defect=None):
    """the four cbam kernels in numpy float32: pooled sums per pixel lane (p, p + 8 alternately into two partials, 8 lanes combined in order), the MLP's
    first layer as NCH chunk partials of clen channels added in order, float32 sigmoids, one fp16 store.  defect: "drop_chunk" = the last chunk that holds
    channels is left out of the first layer"""
    w1, b1, w2, b2, w7, b7 = (np.asarray(a, F) for a in params)
    B, H, W, C = x.shape
    P, Ch = H * W, C // 16
    NCH, clen = cbam_choice(C)
    xf = x.astype(F).reshape(B, P, C)
    lanes = []
    for pl in range(8):
        s0, s1 = np.zeros((B, C), F), np.zeros((B, C), F)
        p = pl
        while p + 8 < P:
            s0, s1 = s0 + xf[:, p], s1 + xf[:, p + 8]
            p += 16
        if p < P:
            s0 = s0 + xf[:, p]
        lanes.append(s0 + s1)
    tot = np.zeros((B, C), F)
    for s in lanes:
        tot = tot + s
    avg, mx = tot / F(P), xf.max(1)
    used = [j for j in range(NCH) if j * clen < C]

    def hidden(v):
        acc = np.zeros((B, Ch), F)
        for j in used:
            if defect == "drop_chunk" and j == used[-1]:
                continue
            part = np.zeros((B, Ch), F)
            for c0 in range(j * clen, min(C, j * clen + clen), 4):
                part = part + (v[:, None, c0:c0 + 4] * w1[None, :, c0:c0 + 4]).sum(-1, dtype=F)
            acc = acc + part
        return np.maximum(acc + b1, F(0))
    hs = hidden(avg) + hidden(mx)
    att = F(2) * b2 + (hs[:, None, :] * w2[None]).sum(-1, dtype=F)
    scale = F(1) / (F(1) + np.exp(-att, dtype=F))
    t = xf * scale[:, None]
    comp = np.stack([t.max(-1), t.sum(-1, dtype=F) / F(C)], -1).reshape(B, H, W, 2)
    cp = np.zeros((B, H + 6, W + 6, 2), F)
    cp[:, 3:3 + H, 3:3 + W] = comp
    acc = np.zeros((B, H, W), F)
    for ch in range(2):
        for ky in range(7):
            for kx in range(7):
                acc = acc + cp[:, ky:ky + H, kx:kx + W, ch] * w7[ch, ky, kx]
    sg = F(1) / (F(1) + np.exp(-(acc + b7[0]), dtype=F))
    return (x.astype(F) * (F(1) + scale[:, None, None] * sg[..., None])).astype(np.float16)


def run_cbam(ctx, x, params, dual):
    """one HAVC_OP_CBAM: x at channel offset 8 of a C + 16 row, y at 16 of C + 24, the rectified twin at 24 of C + 32 -> (y, whole y, y2 or None, whole y2 or None)"""
    from tests.gpu_util import run_plan
    from vsdeoldify_amd.plan import PlanBuilder, View, WeightPack
    B, H, W, C = x.shape
    assert cbam_choice(C) == CBAM_CHOICE.get(C, cbam_choice(C)), "cbam_mlp_kernel's chunking is no longer what this channel count is listed for"
    pack, b = WeightPack(), PlanBuilder()
    xv, yv = View(b.buf(H * W * (C + 16)), 8, C + 16, H, W, C, C), View(b.buf(H * W * (C + 24)), 16, C + 24, H, W, C, C)
    dv = View(b.buf(H * W * (C + 32)), 24, C + 32, H, W, C, C) if dual else None
    b.cbam("cbam", xv, yv, pack.add(np.concatenate([np.asarray(a, F).reshape(-1) for a in params])), b.buf(3 * C, 4), b.buf(H * W * 2, 4), dual=dv)
    dst = np.full((B, H, W, C + 24), SENTINEL, np.float16)
    ups, dl = {xv.buf: in_view(x, C + 16, 8), yv.buf: dst}, {yv.buf: (dst.shape, np.float16)}
    if dual:
        d2 = np.full((B, H, W, C + 32), SENTINEL, np.float16)
        ups[dv.buf], dl[dv.buf] = d2, (d2.shape, np.float16)
    out = run_plan(ctx, pack, b, ups, dl, B)
    full, full2 = out[yv.buf], (out[dv.buf] if dual else None)
    return full[..., 16:16 + C], full, (full2[..., 24:24 + C] if dual else None), full2


# ---- gru, planar in / out, decoder input ---------------------------------------------------------------------------------------------------------------------------------
ACT_VALUES = np.array([0.0, -0.0, 65504.0, -65504.0, 2.0 ** -24, -2.0 ** -24, 6.1e-5, 1.0, -1.0, 8.0, -8.0, 12.0, -12.0, 17.0, -17.0, 30.0, -30.0, 88.0, -88.0,
                       90.0, -90.0, 104.0, -104.0, 1000.0, -1000.0, 0.5, -0.5, 255.875], np.float16)


def act_inputs(shape, seed):
    """fp16 N(0, 2) with ACT_VALUES (+-0, +-65504, a subnormal, arguments at which sigmoid and tanh saturate in fp16, fp32 and beyond) planted"""
    r = np.random.default_rng(seed)
    x = f16(2.0 * r.standard_normal(shape))
    flat = x.reshape(-1)
    idx = r.choice(flat.size, min(flat.size, 3 * len(ACT_VALUES)), replace=False)
    flat[idx] = np.resize(ACT_VALUES, len(idx))
    return x


def gru_f64(vals, h, hd):
    """vals [B][P][3 hd] fp16 (forget | update | new), h float32 [B][hd][P] -> (ref [B][hd][P], bound)"""
    v64 = vals.astype(F64).transpose(0, 2, 1)
    xf, xu, xn = v64[:, :hd], v64[:, hd:2 * hd], v64[:, 2 * hd:]
    h64 = h.astype(F64)
    f, u_, n = sigmoid64(xf), sigmoid64(xu), np.tanh(xn)
    a, c = f * h64 * (1 - u_), u_ * n
    bound = (np.abs(h64) * (1 - u_) * sigmoid_err(xf, f) + (f * np.abs(h64) + np.abs(n)) * sigmoid_err(xu, u_) + u_ * 5 * U32 * np.abs(n) +
             4 * U32 * (np.abs(a) + np.abs(c)) + TINY32 * (1 + np.abs(h64)))
    return a + c, bound


def gru_emulate(vals, h, hd):
    vf = vals.astype(F).transpose(0, 2, 1)
    with np.errstate(over="ignore"):
        f, u_ = (F(1) / (F(1) + np.exp(-vf[:, i * hd:(i + 1) * hd], dtype=F)) for i in (0, 1))
    n = np.tanh(vf[:, 2 * hd:], dtype=F)
    return (f * h * (F(1) - u_) + u_ * n).astype(F)


def run_gru(ctx, vals, h, hd):
    """one HAVC_OP_GRU: values [B][P][3 hd] at channel offset 8 of a 3 hd + 16 row (the rest holds 3000) -> fp32 [B][hd][P]"""
    from tests.gpu_util import run_plan
    from vsdeoldify_amd.plan import PlanBuilder, View, WeightPack
    B, P, C = vals.shape
    b = PlanBuilder()
    vv = View(b.buf(P * (C + 16)), 8, C + 16, 1, P, C, C)
    hb, ho = b.buf(hd * P, 4), b.buf(hd * P, 4)
    b.gru("gru", vv, hb, ho, hd)
    return run_plan(ctx, WeightPack(), b, {vv.buf: in_view(vals, C + 16, 8, fill=np.float16(3000.0)), hb: h.astype(F), ho: np.full((B, hd, P), -777.0, F)},
                    {ho: ((B, hd, P), F)}, B)[ho]


PLANAR_VALUES = np.array([0.0, -0.0, 65504.0, -65504.0, 65519.0, 65520.0, -65520.0, 1e6, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25, -2.0 ** -26, 1e-8, 1.0 + 2.0 ** -11,
                          1.0 + 2.0 ** -11 + 2.0 ** -23, 1.0 + 3 * 2.0 ** -11, 6.1e-5, 0.1], F)


def planar_values(shape, seed):
    """float32 N(0, 1) with PLANAR_VALUES (+-0, the fp16 overflow threshold from both sides, ties and near-ties of the conversion, subnormal results) planted"""
    r = np.random.default_rng(seed)
    x = r.standard_normal(shape).astype(F)
    flat = x.reshape(-1)
    idx = r.choice(flat.size, min(flat.size, 2 * len(PLANAR_VALUES)), replace=False)
    flat[idx] = np.resize(PLANAR_VALUES, len(idx))
    return x


def to_half(a):
    with np.errstate(over="ignore"):
        return np.asarray(a, F).astype(np.float16)


def run_planar_in(ctx, src, P, C, span, pixel_major, bcast, B=2):
    """one HAVC_OP_PLANAR_IN: src float32 [B][C][P] (or [B][P][C]) -> the whole destination [B][P][span + 24], the view at channel offset 16.  A broadcast
    source holds 3000 in its frames past the first"""
    from tests.gpu_util import run_plan
    from vsdeoldify_amd.plan import PlanBuilder, View, WeightPack
    b = PlanBuilder()
    sb = b.buf(C * P, 4)
    yv = View(b.buf(P * (span + 24)), 16, span + 24, 1, P, C, span)
    b.planar_in("pin", sb, C, yv, pixel_major=pixel_major, bcast=bcast)
    s = src.copy()
    if bcast:
        s[1:] = 3000.0
    dst = np.full((B, P, span + 24), SENTINEL, np.float16)
    return run_plan(ctx, WeightPack(), b, {sb: s, yv.buf: dst}, {yv.buf: (dst.shape, np.float16)}, B)[yv.buf]


def planar_out_f64(x, act):
    """x [B][P][C] fp16 -> (ref [B][C][P] float64, bound or None where the op is bit-exact against float32(ref))"""
    x64 = x.astype(F64).transpose(0, 2, 1)
    if act == 0:
        return x64, None
    if act == 1:
        return x64 * x64 + 1.0, None
    if act == 2:
        s = sigmoid64(x64)
        return s, sigmoid_err(x64, s) + TINY32
    t = np.tanh(x64)
    return t, 5 * U32 * np.abs(t)


def run_planar_out(ctx, x, act, coff=40):
    """one HAVC_OP_PLANAR_OUT: x [B][P][C] fp16 at channel offset `coff` of a coff + C + 11 row (3000 elsewhere) -> fp32 [B][C][P]"""
    from tests.gpu_util import run_plan
    from vsdeoldify_amd.plan import PlanBuilder, View, WeightPack
    B, P, C = x.shape
    pitch = pad_to(coff + C + 11, 8)
    b = PlanBuilder()
    xv = View(b.buf(P * pitch), 0, pitch, 1, P, pitch, pitch)
    ob = b.buf(C * P, 4)
    b.planar_out("pout", xv, coff, C, ob, act)
    return run_plan(ctx, WeightPack(), b, {xv.buf: in_view(x, pitch, coff, fill=np.float16(3000.0)), ob: np.full((B, C, P), -777.0, F)}, {ob: ((B, C, P), F)}, B)[ob]


def run_decoder_in(ctx, g, ro, hid):
    """one HAVC_OP_CMN_DECODER_IN: g fp16 [Bg][P][Cg] (frame 0 is read for every object; at channel offset 8 of a Cg + 16 row), ro float32 [B][CV][P],
    hid float32 [B][HD][P] -> (dc, dcr: the whole destinations [B][P][pitch], the row [g | readout | hidden] at channel offset 16 of both)"""
    from tests.gpu_util import run_plan
    from vsdeoldify_amd.plan import PlanBuilder, View, WeightPack
    _, P, Cg = g.shape
    B, CV, HD = ro.shape[0], ro.shape[1], hid.shape[1]
    span = Cg + CV + HD
    pitch = span + 24
    b = PlanBuilder()
    gv = View(b.buf(P * (Cg + 16)), 8, Cg + 16, 1, P, Cg, Cg)
    dc, dcr = b.buf(P * pitch), b.buf(P * pitch)
    rb, hb = b.buf(CV * P, 4), b.buf(HD * P, 4)
    b.cmn_decoder_in("dec_in", gv, rb, CV, hb, HD, View(dc, 16, pitch, 1, P, span, span), dcr)
    gs = np.full((B, P, Cg), 3000.0, np.float16)
    gs[0] = g[0]
    dst = np.full((B, P, pitch), SENTINEL, np.float16)
    out = run_plan(ctx, WeightPack(), b, {gv.buf: in_view(gs, Cg + 16, 8), rb: ro, hb: hid, dc: dst, dcr: dst.copy()},
                   {dc: (dst.shape, np.float16), dcr: (dst.shape, np.float16)}, B)
    return out[dc], out[dcr]
