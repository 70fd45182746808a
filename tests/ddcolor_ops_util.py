"""Shared by tests/test_gpu_ddcolor_ops.py (GPU) and tests/test_ddcolor_ops_host.py (CPU): the cases, inputs, float64 oracles, error rules and one-op plans
by which the fast-mode non-conv kernels of DDColor (csrc/ddcolor.hip) and of the Zhang colorizers (the last third of csrc/elementwise.hip) are held, one op
at a time, against plain float64.  Inputs are fp16-exact (fp32-exact where the op reads fp32) and every reference is computed from those very values.
Every figure is max |GPU - ref| / bound; u = 2^-24 is the unit roundoff of fp32, ulp16 the fp16 ulp AT the exact value.

Multi-head attention, D = 32 (mha32_split_mfma_kernel + mha32_merge_kernel, mha32_kernel).  The rule of tests/remaster_util.py:
    bound = 2^-11 (A + |ref|),  A = sum_k P_k |V_k|,  limit 2 x bound, a figure above 1 asks for an explanation
(P rounded to fp16 moves the weighted mean by <= 2^-11 A, the fp16 store adds <= 2^-11 |ref|; fp32 sums, __expf and the rescale between 256-key chunks
are second order).  Three regimes, all with the SAME random keys and values (the queries make the regime): `flat` scores within +-1; `sharp` one
dominant key per query (score 60, a key that is no chunk edge); `edges` query i puts half of its weight on key e(i), e cycling through
{0, 255, 256, 511, 512, ..., Lk - 1}: every chunk boundary and the last key carry weight, so a key dropped or weighed twice at a boundary moves an
output by a third, where random scores move it by 1 / Lk (below the bound from a few thousand keys on).

LayerNorm over C channels (layernorm_c_kernel<LP>): y = (x - mean) rstd gamma + beta in fp32, one fp16 store.
    bound = ulp16(ref) / 2 + u (k1 mean|x| rstd |gamma| + k2 |ref - beta| + |beta|)
A lane adds its n = 8 ceil(C8 / LP) values serially, log2(LP) butterfly steps follow: the sum carries <= (n + log2 LP) u sum|x|, the division by C one
more u, so the mean is off by <= k1 u mean|x| with k1 = n + log2 LP + 1, and that error is multiplied by rstd |gamma|.  d = x - mean (1 u); d^2 (3 u
relative: twice d's, one product), summed like the mean (n + log2 LP more; the terms are positive, so the error stays relative), / C, + eps, sqrt (halves
what came before, adds 1), 1 / (1): rstd is off by <= ((n + log2 LP + 5) / 2 + 2) u relative; two products and the final sum add 3 u, the sum's last u
also acts on beta: k2 = (n + log2 LP) / 2 + 8.5.  A mean error moves the variance in second order only (two passes).  With ReLU the terms are those of the
value before the ReLU.

dwconv7 (fp16 weights, fp32 fma chain from the bias):  bound = ulp16(ref) / 2 + 50 u sum|x w|  (at most 49 roundings, each on a partial sum no larger
than |bias| + sum|x w|; where |bias| dominates, so does half an fp16 ulp of the result).
dwconv7_ln (fast): the two oracles composed, the LayerNorm rule with x := the float64 conv result.
pixshuf4_blur: ((a + b) + c) + d in fp32, x 0.25, one fp16 store.  On tests/deoldify_ops_util.py blur_inputs the fp32 steps are exact and the result is
float16(float64 mean) bit for bit.  On arbitrary fp16 values it is not: (4096, 2, 2^-14, 0) sums to 4098 in fp32 (2^-14 is below the fp32 ulp 2^-11 at
4096), x 0.25 = 1024.5, a tie that rounds to 1024, where the exact mean 1024.5 + 2^-16 rounds to 1025.  Such inputs (finite_patterns, +-0, subnormals,
+-65504) are held to ulp16(ref) / 2 + 4 u sum|v| / 4.
subsample2: a copy, bit-exact.
fold_queries (fp32 out): nq fmas per output:  bound = (nq + 1) u sum|r e|.
shuf4_blur_ab (fp16 out): four proj values, x 0.25, three image products, bias: bound = ulp16(ref) / 2 + 8 u (sum of |terms|).
proj2 (fp32 out), all terms absolute and x |mul|.  A lane adds ceil(C / 64) products, six butterfly steps follow: ks = ceil(C / 64) + 7 roundings on sums.
    mode 0: ks u sum|x w| + u |a|.
    mode 1 (softmax first): __expf(d), d = x - max <= 0, is v_exp_f32 (1 ulp) of d log2(e) rounded to fp32, d itself rounded where the two fp16 values lie
    far apart: relative error <= (2 + 2 |d|) u.  With P the exact softmax:  u (sum_c P_c |w_c| (2 + 2 |d_c| + ks) + |a| sum_c P_c (2 + 2 |d_c| + ks) + 2 |a|).
    mode 2 (+ bias, tanh): tanhf within 4 ulp, its slope <= 1:  (mode 0's bound) + u |a + bias| + 5 u |tanh|.
bilinear2 (fp32 out): PyTorch's align_corners=False formula in float64 on the same fp32 map, source coordinate (dst + 0.5) scale - 0.5 from the FLOAT32
scale in fp32 as the kernel does: bound = 8 u max|taps| |mul|.  The unit is built with floating-point contraction, so the coordinate is one fma (seen in
the code object); the rule accepts either fp32 evaluation, fused or not, for a whole run."""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

from tests.deoldify_ops_util import (LIMIT, SENT, SENTINEL, attn_ratio, bits, blur_inputs, f16, finite_patterns, in_view,  # noqa: F401  (re-exported)
                                     outside_is_sentinel, pad_to, ulp16)

U32 = 2.0 ** -24
F = np.float32


# ---- multi-head attention, head dim 32 ------------------------------------------------------------------------------------------------------------------------
MHA_KC, TOK = 256, 112
SCALE = F(1.0 / np.sqrt(32.0))
REGIMES = ("flat", "sharp", "edges")
POOL_FRAMES, POOL_KEYS, POOL_E = 32, 4097, 256


def launcher_choice(B, heads, Lk):
    """(nch, nsplit) of launch_mha32_split (csrc/ddcolor.hip), restated: chunks of 256 keys, as many per block (<= 4) as keep 1 024 blocks"""
    nchunks = (Lk + MHA_KC - 1) // MHA_KC
    nch = max(1, min(4, nchunks * heads * B // 1024, nchunks))
    return nch, (nchunks + nch - 1) // nch


@dataclass(frozen=True)
class MhaCase:
    name: str
    B: int
    heads: int
    Lq: int
    Lk: int
    nch: int = 1                 # what launch_mha32_split must choose (asserted before anything runs)
    nsplit: int = 1
    layout: str = "cross"        # "cross": K / V at channel offsets of a wider row with kv_tok = Lk + 3; "pool": the same at the exact pitch 2 E (the large
    #                              cases); "self": Q, K and V in ONE token buffer, View(qkv.buf, 0, ...)
    kernel: str = "split"        # "split" = mha32_split_mfma_kernel + merge; "plain" = mha32_kernel (aux1 = -1, or more than 128 queries)

    @property
    def E(self):
        return self.heads * 32

    @property
    def q_tok(self):
        return TOK if self.Lq <= TOK else pad_to(self.Lq, 16)


LK_SWEEP = (1, 7, 31, 32, 33, 100, 255, 256, 257, 511, 513)
LQ_SWEEP = (1, 15, 16, 17, 112, 127, 128)
PLAIN_LK, PLAIN_LQ = (1, 63, 64, 65, 300), (1, 100, 200)
MHA_CASES = {c.name: c for c in
             [MhaCase(f"k{lk}", 1, 8, 100, lk, 1, (lk + 255) // 256) for lk in LK_SWEEP] +
             [MhaCase(f"q{lq}", 3, 2, lq, 257, 1, 2) for lq in LQ_SWEEP] +
             [MhaCase("self100", 2, 8, 100, 100, 1, 1, "self"),
              MhaCase("nch2", 16, 8, 17, 4097, 2, 9, "pool"),            # 17 chunks, 2 176 one-chunk blocks: two chunks per block, the ninth block has one
              MhaCase("nch4", 32, 8, 17, 4097, 4, 5, "pool"),            # 4 352: four chunks per block, the fifth block has one
              MhaCase("oneblock", 128, 8, 17, 1024, 4, 1, "pool")] +      # the benchmark's coarse level: one block walks all four chunks, nothing to merge
             [MhaCase(f"q{lq}", 2, 2, lq, 257, 1, 2, "cross", "plain") for lq in (129, 200)] +      # HAVC_OP_MHA sends more than 128 queries to mha32_kernel
             [MhaCase(f"plain_k{lk}q{lq}", 2, 2, lq, lk, 1, (lk + 255) // 256, "cross", "plain") for lk in PLAIN_LK for lq in PLAIN_LQ]}
MANY_KEYS = ("nch2", "nch4", "oneblock")


def edge_keys(Lk):
    """{0, 255, 256, 511, 512, ..., Lk - 1}: both sides of every 256-key chunk boundary, the first and the last key"""
    return sorted({0, Lk - 1} | {k for m in range(MHA_KC, Lk + 1, MHA_KC) for k in (m - 1, m) if k < Lk})


@lru_cache(maxsize=None)
def kv_pool():
    """the random K and V rows of the large cases, fp16 [32 x 4097][256] each, made once per process and never written to"""
    r = np.random.default_rng(2024)
    out = []
    for _ in range(2):
        a = r.standard_normal((POOL_FRAMES * POOL_KEYS, POOL_E), dtype=F).astype(np.float16)
        a.setflags(write=False)
        out.append(a)
    return tuple(out)


def mha_kv(case):
    """fp16 k, v [B][Lk][E]; the large cases slice the pool (nch2 = the first 16 frames of nch4)"""
    if case.layout == "pool":
        assert case.E == POOL_E and case.B * case.Lk <= POOL_FRAMES * POOL_KEYS
        return tuple(a[:case.B * case.Lk].reshape(case.B, case.Lk, POOL_E) for a in kv_pool())
    r = np.random.default_rng([5, case.B, case.heads, case.Lk])
    return f16(r.standard_normal((case.B, case.Lk, case.E))), f16(r.standard_normal((case.B, case.Lk, case.E)))


def mha_targets(case, regime, k):
    """int [B][heads][Lq]: the key that query (b, h, i) leans on -- edges: e cycling over edge_keys with the running query number; sharp: the keys of
    largest norm that are no edge (so that no other key's score comes near)"""
    B, H, Lq, Lk = case.B, case.heads, case.Lq, case.Lk
    edges = np.array(edge_keys(Lk))
    if regime == "edges":
        return edges[np.arange(B * H * Lq) % len(edges)].reshape(B, H, Lq)
    norm = (k.reshape(B, Lk, H, 32).astype(np.float64) ** 2).sum(-1).transpose(0, 2, 1)          # [B][H][Lk]
    if Lk > len(edges):
        norm[:, :, edges] = -1.0
    order = np.argsort(-norm, axis=-1, kind="stable")[:, :, :max(1, min(Lq, Lk - len(edges) if Lk > len(edges) else Lk))]
    return order[:, :, np.arange(Lq) % order.shape[-1]]


def mha_queries(case, regime, k, seed=0):
    """fp16 q [B][Lq][E] for the regime, from the keys k [B][Lk][E]"""
    B, H, Lq, Lk = case.B, case.heads, case.Lq, case.Lk
    r = np.random.default_rng([seed, B, H, Lq, Lk, sum(map(ord, regime))])
    if regime == "flat":
        return f16(0.1 * r.standard_normal((B, Lq, case.E)))
    tgt = mha_targets(case, regime, k)
    kh = k.reshape(B, Lk, H, 32).transpose(0, 2, 1, 3)                                            # [B][H][Lk][32]
    ksel = np.take_along_axis(kh, tgt[..., None], axis=2).astype(np.float64)                       # [B][H][Lq][32]
    unit = ksel / (ksel ** 2).sum(-1, keepdims=True)                                               # k_t / |k_t|^2: the score of the target is a, exactly
    if regime == "sharp":
        a = np.full((B, H, Lq), 60.0)
    else:
        # a with exp(a) = sum_{j != e} exp(a t_j), t_j = k_e . k_j / |k_e|^2: half of the weight on key e.  Bisection on [0, 30] in float32.
        t = (unit.astype(F) @ kh.astype(F).transpose(0, 1, 3, 2))                                  # [B][H][Lq][Lk]
        np.put_along_axis(t, tgt[..., None], -np.inf, axis=-1)
        lo, hi = np.zeros((B, H, Lq), F), np.full((B, H, Lq), 30.0, F)
        if Lk > 1:
            for _ in range(14):
                mid = (lo + hi) / 2
                with np.errstate(over="ignore"):
                    more = np.exp(mid[..., None] * t).sum(-1) > np.exp(mid)                         # the others still outweigh the target: a must grow
                lo, hi = np.where(more, mid, lo), np.where(more, hi, mid)
        a = ((lo + hi) / 2).astype(np.float64) if Lk > 1 else np.zeros((B, H, Lq))
    q = (a / float(SCALE))[..., None] * unit
    return f16(q.transpose(0, 2, 1, 3).reshape(B, Lq, case.E))


def mha_inputs(case, regime):
    k, v = mha_kv(case)
    return mha_queries(case, regime, k), k, v


def mha_reference(q, k, v, heads, cols=None, tgt=None):
    """float64 softmax(scale q . k) v per head, scale as the float32 the op carries -> dict(out, A [B][Lq][E]; smax = max |score|; pmax [B][heads][Lq] = the
    largest weight of every query; pcols [B][heads][Lq][len(cols)] = the weights of the keys `cols`; ptgt = the weight of key tgt[b][h][i])"""
    B, Lq, E = q.shape
    Lk = k.shape[1]
    out, A = np.empty((B, Lq, E)), np.empty((B, Lq, E))
    pmax, smax = np.empty((B, heads, Lq)), 0.0
    pcols = np.empty((B, heads, Lq, len(cols))) if cols is not None else None
    ptgt = np.empty((B, heads, Lq)) if tgt is not None else None
    for b in range(B):
        qh = q[b].reshape(Lq, heads, 32).transpose(1, 0, 2).astype(np.float64)
        kh = k[b].reshape(Lk, heads, 32).transpose(1, 2, 0).astype(np.float64)
        vh = v[b].reshape(Lk, heads, 32).transpose(1, 0, 2).astype(np.float64)
        s = float(SCALE) * (qh @ kh)
        smax = max(smax, float(np.abs(s).max()))
        p = np.exp(s - s.max(-1, keepdims=True))
        p /= p.sum(-1, keepdims=True)
        out[b] = (p @ vh).transpose(1, 0, 2).reshape(Lq, E)
        A[b] = (p @ np.abs(vh)).transpose(1, 0, 2).reshape(Lq, E)
        pmax[b] = p.max(-1)
        if cols is not None:
            pcols[b] = p[:, :, cols]
        if tgt is not None:
            ptgt[b] = np.take_along_axis(p, tgt[b][..., None], axis=-1)[..., 0]
    return dict(out=out, A=A, smax=smax, pmax=pmax, pcols=pcols, ptgt=ptgt)


def check_regime(case, regime, ref):
    """the property the regime is named for, from the reference alone (so that a test cannot run on inputs that miss it)"""
    if regime == "flat":
        assert ref["smax"] < 1.0, ref["smax"]
    elif regime == "sharp":
        assert case.Lk == 1 or (ref["pmax"].min() > 0.5 and np.median(ref["pmax"]) > 0.999), (ref["pmax"].min(), np.median(ref["pmax"]))
    else:
        # half of the weight on e(i) -- for 98 % of the queries at least (a key of small norm can have a neighbour whose score outgrows its own: no
        # query length puts half of the weight on such a key), and every edge key has queries that do
        p = ref["ptgt"]
        if case.Lk == 1:
            assert (p == 1.0).all()
            return
        half = (p > 0.4) & (p < 0.6)
        tgt = mha_targets(case, "edges", None)
        assert half.mean() >= 0.98 and all(half[tgt == e].any() for e in edge_keys(case.Lk) if (tgt == e).any()), (float(half.mean()), float(p.min()), float(p.max()))


def mha_ratio(got, ref):
    """(max |got - ref| / (2^-11 (A + |ref|)), index of the worst element)"""
    return attn_ratio(got, ref["out"], ref["A"], 1.0)


def mha_worst_text(case, worst, ratio):
    b, i, c = (int(t) for t in worst)
    return (f"err / bound {ratio:.3f} (limit {LIMIT}) at frame {b}, query {i} (16-query fragment {i // 16}, wave {i // 16 % 4} slot {i // 64}, lane column {i % 16}), "
            f"head {c // 32}, channel {c % 32}")


def without_key(ref, v, heads, col, key):
    """the exact output had key `key` (column `col` of ref['pcols']) not been weighed: (out - P_key v_key) / (1 - P_key)"""
    B, Lq, E = ref["out"].shape
    p = ref["pcols"][..., col].transpose(0, 2, 1)[..., None]                                        # [B][Lq][heads][1]
    o = ref["out"].reshape(B, Lq, heads, 32)
    vk = v[:, key].reshape(B, 1, heads, 32).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        res = np.where(p < 1.0, (o - p * vk) / (1.0 - p), 0.0)
    return res.reshape(B, Lq, E)


def with_phantom_key(ref, heads, col_last):
    """the exact output had one more key been weighed at index Lk the way an unmasked lane of the split kernel would: its K row is the clamped load
    (the last key's, so its score is the last key's) and its V column of the LDS image is zero: out / (1 + P_last)"""
    B, Lq, E = ref["out"].shape
    p = ref["pcols"][..., col_last].transpose(0, 2, 1)[..., None]
    return (ref["out"].reshape(B, Lq, heads, 32) / (1.0 + p)).reshape(B, Lq, E)


def emulate_split(case, q, k, v):
    """mha32_split_mfma_kernel + mha32_merge_kernel in numpy: fp32 scores, 256-key chunks, nch chunks per block with a running (max, sum, acc), P rounded
    to fp16 into the second product, fp32 sums, the merge over the splits, one fp16 store"""
    B, Lq, E = q.shape
    H, Lk = case.heads, k.shape[1]
    nch, nsplit = launcher_choice(B, H, Lk)
    qh = q.reshape(B, Lq, H, 32).transpose(0, 2, 1, 3).astype(F)
    kh = k.reshape(B, Lk, H, 32).transpose(0, 2, 3, 1).astype(F)
    vh = v.reshape(B, Lk, H, 32).transpose(0, 2, 1, 3).astype(F)
    parts = []
    for c in range(nsplit):
        m, l, o = np.full((B, H, Lq), -np.inf, F), np.zeros((B, H, Lq), F), np.zeros((B, H, Lq, 32), F)
        for chk in range(nch):
            k0 = (c * nch + chk) * MHA_KC
            if k0 >= Lk:
                break
            s = (qh @ kh[..., k0:k0 + MHA_KC]) * SCALE
            m_new = np.maximum(m, s.max(-1))
            alpha = np.exp(m - m_new)
            p = np.exp(s - m_new[..., None])
            l = l * alpha + p.sum(-1, dtype=F)
            o = o * alpha[..., None] + p.astype(np.float16).astype(F) @ vh[:, :, k0:k0 + MHA_KC]
            m = m_new
        parts.append((m, l, o))
    M = np.max([p[0] for p in parts], axis=0)
    L, acc = np.zeros((B, H, Lq), F), np.zeros((B, H, Lq, 32), F)
    for m, l, o in parts:
        w = np.exp(m - M)
        L += l * w
        acc += o * w[..., None]
    return (acc * (F(1.0) / L)[..., None]).astype(np.float16).transpose(0, 2, 1, 3).reshape(B, Lq, E)


def emulate_plain(case, q, k, v):
    """mha32_kernel in numpy: lane j of 64 walks keys j, j + 64, ... with an online softmax in fp32 (P stays fp32), the lanes' states are merged, one fp16 store"""
    B, Lq, E = q.shape
    H, Lk = case.heads, k.shape[1]
    qh = q.reshape(B, Lq, H, 32).transpose(0, 2, 1, 3).astype(F) * SCALE
    kh = k.reshape(B, Lk, H, 32).transpose(0, 2, 3, 1).astype(F)
    vh = v.reshape(B, Lk, H, 32).transpose(0, 2, 1, 3).astype(F)
    s = qh @ kh                                                                                     # [B][H][Lq][Lk]
    pad = pad_to(Lk, 64) - Lk
    s = np.concatenate([s, np.full(s.shape[:-1] + (pad,), -np.inf, F)], -1).reshape(B, H, Lq, -1, 64)
    vv = np.concatenate([vh, np.zeros((B, H, pad, 32), F)], 2).reshape(B, H, 1, -1, 64, 32)
    m, l, acc = np.full((B, H, Lq, 64), -np.inf, F), np.zeros((B, H, Lq, 64), F), np.zeros((B, H, Lq, 64, 32), F)
    with np.errstate(invalid="ignore"):
        for t in range(s.shape[3]):
            mn = np.maximum(m, s[..., t, :])
            corr = np.where(np.isneginf(mn), F(0), np.exp(m - mn)).astype(F)
            pj = np.where(np.isneginf(mn), F(0), np.exp(s[..., t, :] - mn)).astype(F)
            l = l * corr + pj
            acc = acc * corr[..., None] + pj[..., None] * vv[:, :, :, t]
            m = mn
        w = np.where(np.isneginf(m), F(0), np.exp(m - m.max(-1, keepdims=True))).astype(F)
    L = (l * w).sum(-1, dtype=F)
    o = (acc * w[..., None]).sum(-2, dtype=F) * (F(1.0) / L)[..., None]
    return o.astype(np.float16).transpose(0, 2, 1, 3).reshape(B, Lq, E)


def mha_layout(heads, Lq, Lk, layout):
    """channel pitches and offsets of the one-op plan (all multiples of 8: the kernels load 16 bytes)"""
    E = heads * 32
    q_tok = TOK if Lq <= TOK else pad_to(Lq, 16)
    if layout == "self":
        assert Lk <= TOK and Lq <= TOK
        return dict(q_tok=TOK, q_pitch=3 * E, q_coff=0, kv_tok=TOK, kv_pitch=3 * E, k_coff=E, v_coff=2 * E, y_pitch=E + 24, y_coff=16)
    if layout == "pool":
        return dict(q_tok=q_tok, q_pitch=E + 16, q_coff=8, kv_tok=Lk, kv_pitch=2 * E, k_coff=0, v_coff=E, y_pitch=E + 24, y_coff=16)
    return dict(q_tok=q_tok, q_pitch=E + 16, q_coff=8, kv_tok=Lk + 3, kv_pitch=2 * E + 32, k_coff=8, v_coff=E + 24, y_pitch=E + 24, y_coff=16)


def mha_plan(heads, Lq, Lk, layout="cross", plain=False):
    """one HAVC_OP_MHA on buffers of its own -> (PlanBuilder, layout dict, q buffer, kv buffer, y buffer); plain: aux1 = -1, which sends the op to mha32_kernel"""
    from vsdeoldify_amd.plan import PlanBuilder, View
    lay = mha_layout(heads, Lq, Lk, layout)
    E = heads * 32
    b = PlanBuilder()
    qb = b.buf(lay["q_tok"] * lay["q_pitch"])
    kvb = qb if layout == "self" else b.buf(lay["kv_tok"] * lay["kv_pitch"])
    yv = View(b.buf(lay["q_tok"] * lay["y_pitch"]), lay["y_coff"], lay["y_pitch"], 1, lay["q_tok"], E, E)
    i = b.mha("mha", View(qb, lay["q_coff"], lay["q_pitch"], 1, lay["q_tok"], E, E), View(kvb, 0, lay["kv_pitch"], 1, lay["kv_tok"], lay["kv_pitch"], lay["kv_pitch"]),
              lay["k_coff"], lay["v_coff"], yv, heads, Lq, Lk, float(SCALE))
    if plain:
        b.ops[i]["aux1"] = -1
    return b, lay, qb, kvb, yv.buf


def run_mha(ctx, q, k, v, heads, layout="cross", plain=False, pad=0.0):
    """q [B][Lq][E], k / v [B][Lk][E] fp16 -> (out [B][Lq][E], the whole destination [B][q_tok][y_pitch], sentinel-filled before the run).
    Rows Lq .. q_tok of the query buffer and channels outside Q / K / V hold random values; rows Lk .. kv_tok of K and V hold `pad` (a scalar, or "big":
    +-60000 at random)."""
    from tests.gpu_util import run_plan
    from vsdeoldify_amd.plan import WeightPack
    B, Lq, E = q.shape
    Lk = k.shape[1]
    b, lay, qb, kvb, yb = mha_plan(heads, Lq, Lk, layout, plain)
    r = np.random.default_rng(7)
    qbuf = f16(r.standard_normal((B, lay["q_tok"], lay["q_pitch"])))
    qbuf[:, :Lq, lay["q_coff"]:lay["q_coff"] + E] = q
    if layout == "self":
        kvbuf = qbuf
    elif layout == "pool":
        kvbuf = np.empty((B, Lk, 2 * E), np.float16)
    else:
        kvbuf = f16(r.standard_normal((B, lay["kv_tok"], lay["kv_pitch"])))
    for a, off in ((k, lay["k_coff"]), (v, lay["v_coff"])):
        kvbuf[:, :Lk, off:off + E] = a
        if lay["kv_tok"] > Lk:
            n = lay["kv_tok"] - Lk
            kvbuf[:, Lk:, off:off + E] = np.where(r.integers(0, 2, (B, n, E)) == 1, 60000.0, -60000.0) if isinstance(pad, str) else pad
    ybuf = np.full((B, lay["q_tok"], lay["y_pitch"]), SENTINEL, np.float16)
    ups = {qb: qbuf, yb: ybuf}
    if kvb != qb:
        ups[kvb] = kvbuf
    full = run_plan(ctx, WeightPack(), b, ups, {yb: (ybuf.shape, np.float16)}, B)[yb]
    return full[:, :Lq, lay["y_coff"]:lay["y_coff"] + E], full


def mha_untouched(full, Lq, E, y_coff=16):
    """rows Lq .. q_tok and every channel outside the E of the destination kept the sentinel"""
    return bool((bits(full[:, Lq:]) == SENT).all()) and outside_is_sentinel(full[:, :Lq], y_coff, E)


# ---- LayerNorm --------------------------------------------------------------------------------------------------------------------------------------------------
LN_CHANNELS = (8, 20, 192, 256, 264, 384, 512, 520, 768, 1024, 1032, 1536, 2048)
LN_LP = dict(zip(LN_CHANNELS, (8, 8, 8, 8, 16, 16, 16, 32, 32, 32, 64, 64, 64)))       # what launch_layernorm_c must choose
LN_PIXELS = (1, 7, 9, 257)
LN_SWEEPS = ((8, 8, 32771), (16, 264, 16387), (32, 520, 8195), (64, 1536, 4099))          # (LP, C, pixels): one sweep of the capped grid and three more
LN_EPS = (1e-6, 1e-5)


def ln_lanes(C):
    """LP of launch_layernorm_c (csrc/ddcolor.hip), restated: lanes per pixel at four 8-channel chunks per lane"""
    need = ((C + 7) // 8 + 3) // 4
    return 8 if need <= 8 else 16 if need <= 16 else 32 if need <= 32 else 64


def ln_grid(npix, LP):
    """blocks of that launch: four waves of 64 / LP pixels per block, at most 1 024 blocks"""
    ppw = 64 // LP
    return min(max(1, ((npix + ppw - 1) // ppw + 3) // 4), 1024)


def ln_k(C):
    LP = ln_lanes(C)
    n = 8 * (((C + 7) // 8 + LP - 1) // LP)
    return n + np.log2(LP) + 1, (n + np.log2(LP)) / 2 + 8.5


def ln_f64(x, gamma, beta, eps, relu=False):
    """float64 LayerNorm over the last axis (biased variance), eps as the float32 the op carries -> (ref, the value before the ReLU, mean|x|, rstd)"""
    x = np.asarray(x, np.float64)
    mean = x.mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(((x - mean) ** 2).mean(-1, keepdims=True) + float(F(eps)))
    pre = (x - mean) * rstd * gamma.astype(np.float64) + beta.astype(np.float64)
    return (np.maximum(pre, 0.0) if relu else pre), pre, np.abs(x).mean(-1, keepdims=True), rstd


def ln_excess(got, x, gamma, beta, eps, relu=False, C=None):
    """|got - ref| / (ulp16(ref) / 2 + u (k1 mean|x| rstd |gamma| + k2 |pre - beta| + |beta|)), k1 / k2 of the C-channel launch (default: x's width)"""
    ref, pre, mabs, rstd = ln_f64(x, gamma, beta, eps, relu)
    k1, k2 = ln_k(C or x.shape[-1])
    g, b = np.abs(gamma.astype(np.float64)), np.abs(beta.astype(np.float64))
    bound = ulp16(ref) / 2 + U32 * (k1 * mabs * rstd * g + k2 * np.abs(pre - beta.astype(np.float64)) + b)
    return np.abs(np.asarray(got).astype(np.float64) - ref) / bound


def ln_params(C, seed=0):
    r = np.random.default_rng([11, C, seed])
    return (1.0 + 0.3 * r.standard_normal(C)).astype(F), (0.2 * r.standard_normal(C)).astype(F)


def ln_inputs(kind, npix, C, seed=0):
    """fp16 [npix][C].  random: 2 N(0, 1); offset: mean 30, std 0.5 (the mean cancels 60 standard deviations); special (npix >= 3): random, but pixel
    npix // 2 holds 1.5 everywhere (reference = beta exactly) and the last pixel +-60000 alternating"""
    r = np.random.default_rng([13, npix, C, seed, sum(map(ord, kind))])
    if kind == "offset":
        return f16(30.0 + 0.5 * r.standard_normal((npix, C)))
    x = f16(2.0 * r.standard_normal((npix, C)))
    if kind == "special":
        assert npix >= 3 and C % 2 == 0
        x[npix // 2] = np.float16(1.5)
        x[-1] = np.where(np.arange(C) % 2 == 0, 60000.0, -60000.0).astype(np.float16)
    return x


def ln_emulate(x, gamma, beta, eps, relu, order):
    """the kernel's float32 arithmetic in numpy, the two sums in one of two orders: "lanes" = a lane's values serially (chunk l, l + LP, ..), then a
    pairwise tree over the LP lanes; "serial" = plain left to right"""
    npix, C = x.shape
    LP = ln_lanes(C)
    xf = x.astype(F)

    def total(v):
        if order == "serial":
            return np.cumsum(v, axis=-1, dtype=F)[:, -1]
        w = np.zeros((npix, 4 * LP * 8), F)
        w[:, :C] = v
        w = w.reshape(npix, 4, LP, 8)
        acc = np.zeros((npix, LP), F)
        for kk in range(4):
            for e in range(8):
                acc = acc + w[:, kk, :, e]
        while acc.shape[1] > 1:
            acc = acc[:, 0::2] + acc[:, 1::2]
        return acc[:, 0]
    mean = total(xf) / F(C)
    d = xf - mean[:, None]
    rstd = F(1.0) / np.sqrt(total(d * d) / F(C) + F(eps))
    t = d * rstd[:, None] * gamma + beta
    return (np.maximum(t, F(0)) if relu else t).astype(np.float16)


def run_layernorm(ctx, x, gamma, beta, eps, relu=False, views=True, B=1):
    """one HAVC_OP_LAYERNORM on x [B * npix][C] fp16 (B frames of 1 x npix tokens).  views: x at channel offset 8 of a C8 8 + 16 pitch buffer, y at offset 16
    of a C8 8 + 24 pitch buffer.  The input's pad channels C .. C8 8 hold 1000 (the kernel may not sum them), everything else the sentinel.
    -> (y [B * npix][C8 8], the whole destination [B * npix][pitch])"""
    from tests.gpu_util import run_plan
    from vsdeoldify_amd.plan import PlanBuilder, View, WeightPack
    n, C = x.shape
    npix, C8 = n // B, pad_to(C, 8)
    xo, xp, yo, yp = (8, C8 + 16, 16, C8 + 24) if views else (0, C8, 0, C8)
    pack, b = WeightPack(), PlanBuilder()
    xv = View(b.buf(npix * xp), xo, xp, 1, npix, C, C8)
    yv = View(b.buf(npix * yp), yo, yp, 1, npix, C, C8)
    b.layernorm("ln", xv, yv, pack.add(gamma.astype(F)), pack.add(beta.astype(F)), eps, relu)
    xs = np.full((n, C8), 1000.0, np.float16)
    xs[:, :C] = x
    dst = np.full((n, yp), SENTINEL, np.float16)
    full = run_plan(ctx, pack, b, {xv.buf: in_view(xs, xp, xo), yv.buf: dst}, {yv.buf: (dst.shape, np.float16)}, B)[yv.buf]
    return full[:, yo:yo + C8], full


# ---- depthwise 7 x 7 ----------------------------------------------------------------------------------------------------------------------------------------------
DW_SHAPES = ((1, 1), (2, 3), (3, 7), (7, 7), (8, 5), (13, 10))
DW_CHANNELS = (8, 192, 200)
DWLN_SHAPES = ((192, 13, 10, 3), (384, 8, 8, 3), (768, 7, 9, 3), (1536, 5, 6, 3), (64, 3, 2, 3), (192, 64, 64, 17))      # tests/test_ddcolor.py's


def dw_params(C, seed=0):
    """fp16-exact weights [C][7][7] (as float32), float32 bias, gamma, beta"""
    r = np.random.default_rng([17, C, seed])
    w = f16(r.standard_normal((C, 7, 7)) / 7).astype(F)
    bias, gamma, beta = (r.standard_normal(C).astype(F) * s + o for s, o in ((0.1, 0), (0.2, 1), (0.1, 0)))
    return w, bias.astype(F), gamma.astype(F), beta.astype(F)


def dwconv7_f64(x, w, bias=None):
    """float64 depthwise 7 x 7 cross-correlation, pad 3: x [B][H][W][C], w [C][7][7] -> (ref, sum |x w|).  (torch tensors: 49 fused multiply-adds over the
    whole array, on all cores)"""
    import torch
    B, H, W, C = x.shape
    xp = torch.zeros((B, H + 6, W + 6, C), dtype=torch.float64)
    xp[:, 3:3 + H, 3:3 + W] = torch.from_numpy(np.asarray(x, np.float64))
    wt = torch.from_numpy(np.asarray(w, np.float64))
    ref, mag = torch.zeros((B, H, W, C), dtype=torch.float64), torch.zeros((B, H, W, C), dtype=torch.float64)
    for dy in range(7):
        for dx in range(7):
            win = xp[:, dy:dy + H, dx:dx + W]
            ref.addcmul_(win, wt[:, dy, dx])
            mag.addcmul_(win.abs(), wt[:, dy, dx].abs())
    if bias is not None:
        ref += torch.from_numpy(np.asarray(bias, np.float64))
    return ref.numpy(), mag.numpy()


def dw_excess(got, ref, mag):
    return np.abs(np.asarray(got).astype(np.float64) - ref) / (ulp16(ref) / 2 + U32 * 50 * mag)


def run_dwconv7(ctx, x, w, bias=None, ln=None, views=True):
    """one HAVC_OP_DWCONV7 -- or, with ln = (gamma, beta, eps), one HAVC_OP_DWCONV7_LN -- on x [B][H][W][C] fp16 with the production weight packing
    (DDColorGenerator._dw_pack, fp16 [49][C]).  views: x at offset 8 of a C + 16 pitch buffer, y at offset 16 of a C + 24 pitch buffer.
    -> (y [B][H][W][C], the whole destination)"""
    from tests.gpu_util import run_plan
    from vsdeoldify_amd.ddcolor_net import DDColorGenerator
    from vsdeoldify_amd.plan import PlanBuilder, View, WeightPack
    B, H, W, C = x.shape
    xo, xp, yo, yp = (8, C + 16, 16, C + 24) if views else (0, C, 0, C)
    pack, b = WeightPack(), PlanBuilder()
    xv, yv = View(b.buf(H * W * xp), xo, xp, H, W, C, C), View(b.buf(H * W * yp), yo, yp, H, W, C, C)
    w_off = pack.add(DDColorGenerator._dw_pack(w.reshape(C, 1, 7, 7), C))
    b_off = pack.add(bias.astype(F)) if bias is not None else -1
    if ln is None:
        b.dwconv7("dw", xv, yv, w_off, b_off, C)
    else:
        b.dwconv7_ln("dwln", xv, yv, w_off, b_off, C, pack.add(ln[0].astype(F)), pack.add(ln[1].astype(F)), ln[2])
    dst = np.full((B, H, W, yp), SENTINEL, np.float16)
    full = run_plan(ctx, pack, b, {xv.buf: in_view(x, xp, xo), yv.buf: dst}, {yv.buf: (dst.shape, np.float16)}, B)[yv.buf]
    return full[..., yo:yo + C], full


# ---- PixelShuffle(4) + blur ---------------------------------------------------------------------------------------------------------------------------------------
PS_SHAPES = ((1, 1), (2, 3), (5, 4))
PS_CHANNELS = (8, 24, 256)


def pixshuf4_f64(x):
    """x [B][Hi][Wi][16 C], channel (dy 4 + dx) C + c -> float64 [B][4 Hi][4 Wi][C]"""
    B, Hi, Wi, C16 = x.shape
    C = C16 // 16
    return np.asarray(x, np.float64).reshape(B, Hi, Wi, 4, 4, C).transpose(0, 1, 3, 2, 4, 5).reshape(B, 4 * Hi, 4 * Wi, C)


def blur_f64(up):
    """ReplicationPad2d((1, 0, 1, 0)) + AvgPool2d(2, stride 1) on [B][H][W][C] float64 -> (mean, sum |v| / 4)"""
    H, W = up.shape[1:3]
    y0, x0 = np.maximum(np.arange(H) - 1, 0), np.maximum(np.arange(W) - 1, 0)
    taps = (up[:, y0][:, :, x0], up[:, y0], up[:, :, x0], up)
    return sum(taps) / 4.0, sum(np.abs(t) for t in taps) / 4.0


def pixshuf4_blur_f64(x):
    return blur_f64(pixshuf4_f64(x))


def ps_marks(B, Hi, Wi, C):
    """every (sub-pixel group g, channel c) its own constant 16 (c % 64) + g + a per-pixel step of 1024: a wrong (dy 4 + dx) C + c order is a wrong byte"""
    g, c = np.meshgrid(np.arange(16), np.arange(C), indexing="ij")
    base = (16 * (c % 64) + g).reshape(-1).astype(np.float64)
    pix = 1024.0 * (np.arange(B * Hi * Wi) % 3).reshape(B, Hi, Wi, 1)
    return f16(base + pix)


def ps_patterns(shape, seed):
    """finite_patterns with +0, -0, the smallest subnormals and +-65504 planted"""
    x = finite_patterns(shape, seed).copy()
    flat = x.reshape(-1)
    special = np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x7BFF, 0xFBFF], np.uint16).view(np.float16)
    idx = np.random.default_rng(seed).choice(flat.size, min(flat.size, 4 * len(special)), replace=False)
    flat[idx] = np.resize(special, len(idx))
    return x


def run_pixshuf4_blur(ctx, x, views=True):
    """one HAVC_OP_PIXSHUF4_BLUR on x [B][Hi][Wi][16 C]: x at offset 8 of a 16 C + 16 pitch buffer, y at offset 16 of a C + 24 pitch buffer"""
    from tests.gpu_util import run_plan
    from vsdeoldify_amd.plan import PlanBuilder, View, WeightPack
    B, Hi, Wi, C16 = x.shape
    C = C16 // 16
    xo, xp, yo, yp = (8, C16 + 16, 16, C + 24) if views else (0, C16, 0, C)
    b = PlanBuilder()
    xv, yv = View(b.buf(Hi * Wi * xp), xo, xp, Hi, Wi, C16, C16), View(b.buf(16 * Hi * Wi * yp), yo, yp, 4 * Hi, 4 * Wi, C, C)
    b.pixshuf4_blur("ps", xv, yv)
    dst = np.full((B, 4 * Hi, 4 * Wi, yp), SENTINEL, np.float16)
    full = run_plan(ctx, WeightPack(), b, {xv.buf: in_view(x, xp, xo), yv.buf: dst}, {yv.buf: (dst.shape, np.float16)}, B)[yv.buf]
    return full[..., yo:yo + C], full


# ---- Zhang: subsample2, proj2, bilinear2 ----------------------------------------------------------------------------------------------------------------------------
SUB_SHAPES = ((1, 1), (2, 2), (2, 3), (5, 4), (8, 8), (17, 31))
SUB_CHANNELS = (8, 264)
PROJ_CHANNELS = (8, 64, 128, 313, 512)
PROJ_PIXELS = (1, 5, 4099)
BILINEAR_SIZES = (((1, 1), (4, 4)), ((3, 5), (12, 20)), ((16, 16), (64, 64)), ((7, 9), (20, 13)), ((64, 64), (135, 240)), ((5, 5), (5, 5)))
AB_MUL = 110.0


def run_subsample2(ctx, x):
    """one HAVC_OP_SUBSAMPLE2 on x [B][H][W][C]: x at offset 8 of a C + 16 pitch buffer, y at offset 16 of a C + 24 pitch buffer"""
    from tests.gpu_util import run_plan
    from vsdeoldify_amd.plan import PlanBuilder, View, WeightPack
    B, H, W, C = x.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    b = PlanBuilder()
    xv, yv = View(b.buf(H * W * (C + 16)), 8, C + 16, H, W, C, C), View(b.buf(Ho * Wo * (C + 24)), 16, C + 24, Ho, Wo, C, C)
    b.subsample2("sub", xv, yv)
    dst = np.full((B, Ho, Wo, C + 24), SENTINEL, np.float16)
    full = run_plan(ctx, WeightPack(), b, {xv.buf: in_view(x, C + 16, 8), yv.buf: dst}, {yv.buf: (dst.shape, np.float16)}, B)[yv.buf]
    return full[..., 16:16 + C], full


def proj_inputs(C, npix, mode, seed=0):
    """x fp16 [npix][C], w float32 [2][C], bias float32 [2].  Softmax mode: logits of spread 3, pixel 0 spans 60 and more (a ramp from -40 to +40), the
    last pixel holds C equal logits (the result is the mean of the weights)"""
    r = np.random.default_rng([19, C, npix, mode, seed])
    w = r.standard_normal((2, C)).astype(F) / F(np.sqrt(C) if mode != 1 else 1.0)
    bias = (0.3 * r.standard_normal(2)).astype(F)
    x = f16((3.0 if mode == 1 else 1.0) * r.standard_normal((npix, C)))
    if mode == 1:
        x[0] = f16(np.linspace(-40.0, 40.0, C)[r.permutation(C)])
        if npix > 1:
            x[-1] = np.float16(2.5)
    return x, w, bias


def proj2_f64(x, w, bias, mode, mul):
    """-> (ref [npix][2], bound [npix][2]) of proj2_kernel's three modes"""
    x64, w64 = np.asarray(x, np.float64), np.asarray(w, np.float64)
    C = x64.shape[-1]
    ks = (C + 63) // 64 + 7
    m = abs(float(F(mul)))
    if mode == 1:
        d = x64 - x64.max(-1, keepdims=True)
        P = np.exp(d)
        P /= P.sum(-1, keepdims=True)
        a = P @ w64.T
        cond = 2.0 + 2.0 * np.abs(d) + ks
        bound = U32 * ((P * cond) @ np.abs(w64).T + np.abs(a) * (P * cond).sum(-1, keepdims=True) + 2 * np.abs(a))
        return a * float(F(mul)), bound * m
    a = x64 @ w64.T
    bound = U32 * (ks * (np.abs(x64) @ np.abs(w64).T) + np.abs(a))
    if mode == 2:
        s = a + np.asarray(bias, np.float64)
        t = np.tanh(s)
        return t * float(F(mul)), (bound + U32 * np.abs(s) + 5 * U32 * np.abs(t)) * m
    return a * float(F(mul)), bound * m


def run_proj2(ctx, x, w, bias, mode, mul, B=1):
    """one HAVC_OP_PROJ2 on x [B * npix][C] fp16 at offset 8 of a C8 8 + 16 pitch buffer -> fp32 [B * npix][2]"""
    from tests.gpu_util import run_plan
    from vsdeoldify_amd.plan import PlanBuilder, View, WeightPack
    n, C = x.shape
    npix, C8 = n // B, pad_to(C, 8)
    pack, b = WeightPack(), PlanBuilder()
    xv = View(b.buf(npix * (C8 + 16)), 8, C8 + 16, 1, npix, C, C8)
    out = b.buf(npix * 2, 4)
    b.proj2("proj", xv, pack.add(w.astype(F)), pack.add(bias.astype(F)) if mode & 2 else -1, mode, mul, out)
    xs = np.full((n, C8), 1000.0, np.float16)
    xs[:, :C] = x
    return run_plan(ctx, pack, b, {xv.buf: in_view(xs, C8 + 16, 8), out: np.full((n, 2), -777.0, F)}, {out: ((n, 2), F)}, B)[out]


def bilinear_src(n_in, n_out, how="fma"):
    """(i0, i1, lambda as float32) of bilin_src for every destination index: src = (dst + 0.5) scale - 0.5 with the float32 scale n_in / n_out, in float32
    ("fma": product and sum rounded once; "mul_add": twice) or exactly ("f64": the float64 value of the same expression with the same float32 scale)"""
    scale = F(n_in) / F(n_out)
    d = np.arange(n_out, dtype=F) + F(0.5)
    exact = d.astype(np.float64) * float(scale) - 0.5                   # the float64 product of two float32 values is exact
    src = {"fma": exact.astype(F), "mul_add": (d * scale - F(0.5)).astype(F), "f64": exact}[how]
    src = np.maximum(src, 0)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    return i0, i1, src - i0.astype(src.dtype)


def bilinear2_f64(x, Ho, Wo, mul, how="fma"):
    """x fp32 [B][Hi][Wi][2] -> (ref float64 [B][Ho][Wo][2], max |taps| per output)"""
    Hi, Wi = x.shape[1:3]
    y0, y1, ly = bilinear_src(Hi, Ho, how)
    x0, x1, lx = bilinear_src(Wi, Wo, how)
    x64 = np.asarray(x, np.float64)
    ly, lx = ly.astype(np.float64)[None, :, None, None], lx.astype(np.float64)[None, None, :, None]
    p00, p01, p10, p11 = x64[:, y0][:, :, x0], x64[:, y0][:, :, x1], x64[:, y1][:, :, x0], x64[:, y1][:, :, x1]
    ref = ((1 - ly) * ((1 - lx) * p00 + lx * p01) + ly * ((1 - lx) * p10 + lx * p11)) * float(F(mul))
    return ref, np.max(np.abs([p00, p01, p10, p11]), axis=0)


def bilinear_excess(got, x, Ho, Wo, mul):
    """the smaller of the two maxima of |got - ref| / (8 u max|taps| |mul|), the source coordinate fused or not -> (figure, which)"""
    res = {}
    for how in ("fma", "mul_add"):
        ref, taps = bilinear2_f64(x, Ho, Wo, mul, how)
        res[how] = float((np.abs(np.asarray(got, np.float64) - ref) / (8 * U32 * taps * abs(float(F(mul))))).max())
    how = min(res, key=res.get)
    return res[how], how


def run_bilinear2(ctx, x, Ho, Wo, mul):
    from tests.gpu_util import run_plan
    from vsdeoldify_amd.plan import PlanBuilder, WeightPack
    B, Hi, Wi, _ = x.shape
    b = PlanBuilder()
    src, dst = b.buf(Hi * Wi * 2, 4), b.buf(Ho * Wo * 2, 4)
    b.bilinear2("up", src, Hi, Wi, dst, Ho, Wo, mul)
    return run_plan(ctx, WeightPack(), b, {src: x.astype(F), dst: np.full((B, Ho, Wo, 2), -777.0, F)}, {dst: ((B, Ho, Wo, 2), F)}, B)[dst]


# ---- DDColor tail: fold_queries, shuf4_blur_ab -------------------------------------------------------------------------------------------------------------------------
def fold_f64(e, r, nq):
    """e [B][tok][C] fp16, r float32 [2][r_pitch] -> (ref [B][2][C], sum |r e|)"""
    e64, r64 = np.asarray(e, np.float64)[:, :nq], np.asarray(r, np.float64)[:, :nq]
    return np.einsum("oq,bqc->boc", r64, e64), np.einsum("oq,bqc->boc", np.abs(r64), np.abs(e64))


def run_fold_queries(ctx, e, r, nq):
    """one HAVC_OP_FOLD_QUERIES: e [B][tok][C] as a view at offset 8 of a C + 16 pitch token buffer -> fp32 [B][2][C]"""
    from tests.gpu_util import run_plan
    from vsdeoldify_amd.plan import PlanBuilder, View, WeightPack
    B, tok, C = e.shape
    pack, b = WeightPack(), PlanBuilder()
    ev = View(b.buf(tok * (C + 16)), 8, C + 16, 1, tok, C, C)
    out = b.buf(2 * C, 4)
    b.fold_queries("fold", ev, nq, pack.add(r.astype(F)), r.shape[1], out)
    return run_plan(ctx, pack, b, {ev.buf: in_view(e, C + 16, 8), out: np.full((B, 2, C), -777.0, F)}, {out: ((B, 2, C), F)}, B)[out]


def shuf_ab_f64(proj, img, rimg, bias):
    """proj fp32 [B][Hi][Wi][16][2], img fp16 [B][4 Hi][4 Wi][3], rimg float32 [2][3], bias float32 [2] -> (ref [B][4 Hi][4 Wi][2], sum of |terms|)"""
    B, Hi, Wi = proj.shape[:3]
    mean, mag = blur_f64(pixshuf4_f64(np.asarray(proj, np.float64).reshape(B, Hi, Wi, 32)))
    i64, r64, b64 = np.asarray(img, np.float64), np.asarray(rimg, np.float64), np.asarray(bias, np.float64)
    return mean + i64 @ r64.T + b64, mag + np.abs(i64) @ np.abs(r64).T + np.abs(b64)


def shuf_ab_excess(got, ref, mag):
    return np.abs(np.asarray(got).astype(np.float64) - ref) / (ulp16(ref) / 2 + 8 * U32 * mag)


def run_shuf4_blur_ab(ctx, proj, img, rimg, bias, y_coff):
    """one HAVC_OP_SHUF4_BLUR_AB: the image at offset 8 of a 24-pitch buffer, y at offset y_coff of a 24-pitch buffer -> the whole destination [B][Ho][Wo][24]"""
    from tests.gpu_util import run_plan
    from vsdeoldify_amd.plan import PlanBuilder, View, WeightPack
    B, Hi, Wi = proj.shape[:3]
    Ho, Wo = 4 * Hi, 4 * Wi
    pack, b = WeightPack(), PlanBuilder()
    pb = b.buf(Hi * Wi * 32, 4)
    iv, yv = View(b.buf(Ho * Wo * 24), 8, 24, Ho, Wo, 3, 8), View(b.buf(Ho * Wo * 24), y_coff, 24, Ho, Wo, 2, 8)
    b.shuf4_blur_ab("ab", pb, Hi, Wi, iv, pack.add(rimg.astype(F)), pack.add(bias.astype(F)), yv)
    i8 = np.full((B, Ho, Wo, 8), 1000.0, np.float16)
    i8[..., :3] = img
    dst = np.full((B, Ho, Wo, 24), SENTINEL, np.float16)
    return run_plan(ctx, pack, b, {pb: proj.astype(F), iv.buf: in_view(i8, 24, 8), yv.buf: dst}, {yv.buf: (dst.shape, np.float16)}, B)[yv.buf]
