"""Shared by tests/test_gpu_remaster_ops.py (GPU) and tests/test_remaster_ops_host.py (CPU): the cases, inputs and error rules by which the kernels of
csrc/remaster.hip are held, one op at a time, against oracle/remaster.py.

Source-reference attention.  Inputs are fp16-exact, the float64 reference is computed from those very values, so no input rounding is in the error.
    bound = 2^-11 (|gamma| A + |ref|),   A = softmax . |v|,   limit = 2 x bound            (LIMIT)
P rounded to fp16 moves every weight by <= 2^-11 relative and the weighted mean by <= 2^-11 A; the fp16 store adds <= 2^-11 |ref|; the factor 2 is for
what is second order: fp32 accumulation order, __expf, the fp32 score error, the online rescale.  tests/test_remaster_ops_host.py shows that an
emulation of the kernel's arithmetic stays inside and that four kinds of wrong kernel do not.

fp16 / fp32 results of element-wise kernels: |got - exact| in units of the format's ulp AT the exact value (subnormal fp16 results: 2^-24).
"""
from dataclasses import dataclass

import numpy as np

from oracle import remaster as O

D, DV = 64, 512
LIMIT = 2.0                      # x bound
GAMMAS = (0.7, -1.3)


@dataclass(frozen=True)
class AttnCase:
    name: str
    T: int                       # frames of queries
    nq: int                      # queries per frame
    Tr: int                      # stills; 0 = the keys are the batch's own frames (self-attention)
    nk: int                      # keys per still
    npitch: int
    regimes: tuple
    batch: int = 0               # frames actually run (0 = T): a short batch on a net of max_batch T

    @property
    def stills(self):
        return self.Tr or (self.batch or self.T)

    @property
    def frames(self):
        return self.batch or self.T


CASES = {c.name: c for c in (
    AttnCase("one", 1, 1, 1, 1, 64, ("flat",)),
    AttnCase("small", 2, 12, 2, 15, 64, ("flat", "negative")),
    AttnCase("cross", 3, 24, 5, 40, 64, ("flat", "sharp", "rising", "falling")),
    AttnCase("edge63", 2, 32, 1, 63, 64, ("flat", "negative")),
    AttnCase("edge64", 2, 32, 1, 64, 64, ("flat",)),
    AttnCase("edge65", 2, 32, 1, 65, 128, ("flat", "negative")),
    AttnCase("three", 2, 35, 2, 129, 192, ("flat", "sharp", "negative", "rising", "falling")),
    AttnCase("three_wide", 2, 35, 2, 129, 256, ("flat", "sharp", "negative", "rising", "falling")),
    AttnCase("ring200", 2, 24, 3, 200, 256, ("flat",)),
    AttnCase("tiles29", 1, 8, 1, 1824, 1856, ("flat", "sharp")),         # the 32 x 57 key grid of the operating point: 28 full tiles and a 32-key tail
    AttnCase("self", 3, 96, 0, 96, 128, ("flat",)),
    AttnCase("self_short", 3, 96, 0, 96, 128, ("flat",), batch=2),
)}


def f16(a):
    return np.asarray(a, np.float64).astype(np.float16)


def attn_inputs(case, regime, seed=0):
    """fp16 arrays x [T][nq][512], q [T][nq][64], k [S][nk][64], v [S][nk][512] (S = stills; self form: one entry per frame of the net, nk == nq).
    Frames past case.frames (the short batch) hold large values everywhere: nothing may read them."""
    r = np.random.default_rng([seed, sum(map(ord, case.name)), sum(map(ord, regime))])
    T, nq, nk = case.T, case.nq, case.nk
    S = case.Tr or case.T
    x = r.standard_normal((T, nq, DV))
    v = r.standard_normal((S, nk, DV))
    tiles = (nk + 63) // 64
    if regime in ("flat", "sharp"):
        sigma = 0.25 if regime == "flat" else 0.9
        q, k = sigma * r.standard_normal((T, nq, D)), sigma * r.standard_normal((S, nk, D))
    else:
        # all queries lean the same way, so that the sign / the order of the scores holds for every (query, key) pair
        u = r.standard_normal(D)
        u /= np.linalg.norm(u)
        if regime == "negative":
            q = r.uniform(2.0, 3.0, (T, nq, 1)) * u + 0.05 * r.standard_normal((T, nq, D))
            k = -r.uniform(5.0, 8.0, (S, nk, 1)) * u + 0.05 * r.standard_normal((S, nk, D))
        else:
            order = np.arange(S * tiles).reshape(S, tiles)
            if regime == "falling":
                order = order.max() - order
            level = 24.0 * np.repeat(order, 64, axis=1)[:, :nk, None]            # per (still, key): 24 x the rank of its tile
            q = r.uniform(1.0, 1.1, (T, nq, 1)) * u + 0.02 * r.standard_normal((T, nq, D))
            k = level * u + 0.1 * r.standard_normal((S, nk, D))
    x, q, k, v = f16(x), f16(q), f16(k), f16(v)
    if case.batch:
        for a in (x, q, k, v):
            a[case.batch:] = np.float16(3000.0)
    return x, q, k, v


def scores(case, q, k):
    """float64 [NQ][S][nk] of the frames / stills that take part"""
    n, s = case.frames, case.stills
    return np.einsum("qd,skd->qsk", q[:n].reshape(-1, D).astype(np.float64), k[:s].astype(np.float64))


def check_regime(case, regime, q, k):
    """the property the regime is named for, on the true scores (so that a test cannot run on inputs that miss it)"""
    s = scores(case, q, k)
    if regime == "flat":
        assert np.abs(s).max() < 4.0, np.abs(s).max()
    elif regime == "sharp":
        assert case.nk < 16 or np.abs(s).max() > 20.0, np.abs(s).max()
    elif regime == "negative":
        assert s.max() <= -8.0, s.max()
    else:
        tiles = (case.nk + 63) // 64
        mx = np.stack([s[:, :, t * 64:(t + 1) * 64].max(-1) for t in range(tiles)], -1).reshape(len(s), -1)      # [NQ][still x tile] in walking order
        step = np.diff(mx, axis=1)
        assert (step >= 20.0).all() if regime == "rising" else (step <= -20.0).all(), (step.min(), step.max())


def attn_reference(case, x, q, k, v, gamma):
    """(out, A) of oracle.remaster.srcref_attention as [frames][nq][512]; gamma as the float32 the op carries"""
    n, s = case.frames, case.stills
    g = float(np.float32(gamma))
    out, A = O.srcref_attention(x[:n].reshape(-1, DV), q[:n].reshape(-1, D), k[:s].reshape(-1, D), v[:s].reshape(-1, DV), g)
    return out.reshape(n, case.nq, DV), A.reshape(n, case.nq, DV)


def attn_bound(ref, A, gamma):
    return 2.0 ** -11 * (abs(float(np.float32(gamma))) * A + np.abs(ref))


def attn_ratio(got, ref, A, gamma):
    """(max err / bound, index of the worst element); err 0 on a zero bound counts as 0"""
    err, bound = np.abs(np.asarray(got, np.float64) - ref), attn_bound(ref, A, gamma)
    ratio = np.where(err == 0, 0.0, err / np.where(bound > 0, bound, np.finfo(np.float64).tiny))
    worst = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[worst]), worst


def attn_worst_text(case, q, k, worst, ratio):
    """the worst element as (query, channel) and the (still, tile) that holds most of its softmax weight"""
    f, p, c = (int(i) for i in worst)
    s = scores(case, q, k)[f * case.nq + p]
    st, key = np.unravel_index(int(np.argmax(s)), s.shape)
    return f"err / bound {ratio:.3f} (limit {LIMIT}) at query {f * case.nq + p} (frame {f}, token {p}), channel {c}; heaviest key: still {st}, tile {key // 64}, key {key}"


def value_rows(case, v, pad=0.0):
    """v [S][nk][512] -> V^T [S][512][npitch] fp16, columns nk .. npitch filled with `pad` (scalar or array [S][512][npitch - nk])"""
    S = v.shape[0]
    vT = np.empty((S, DV, case.npitch), np.float16)
    vT[:, :, :case.nk] = v.transpose(0, 2, 1)
    vT[:, :, case.nk:] = pad
    return vT


def run_attention(ctx, case, x, q, k, vT, gamma, views=False, still_order=None):
    """one HAVC_OP_SRCREF_ATTN on uploaded buffers -> (y [frames][nq][512] fp16, the whole y buffer [T][nq][pitch] fp16).
    views: q is a 64-channel view at offset 64 of a 128-wide buffer, x a view at offset 512 of a 1024-pitch buffer, y at offset 0 of a 1024-pitch
    buffer whose other half (like every frame past the batch) keeps the sentinel it was filled with.
    still_order: the slots in which the stills are placed.  Key / value buffers that hold more stills than the net has frames are bound ones."""
    from tests.gpu_util import run_plan
    from vsdeoldify_amd.plan import PlanBuilder, View, WeightPack
    T, nq, nk, n = case.T, case.nq, case.nk, case.frames
    qp, qo, xp, xo, yp, yo = (128, 64, 1024, 512, 1024, 0) if views else (64, 0, 512, 0, 512, 0)
    b = PlanBuilder()
    xv = View(b.buf(nq * xp), xo, xp, 1, nq, DV, DV)
    qv = View(b.buf(nq * qp), qo, qp, 1, nq, D, D)
    yv = View(b.buf(nq * yp), yo, yp, 1, nq, DV, DV)
    kb, vb = b.buf(nk * D), b.buf(DV * case.npitch)
    b.srcref_attn("attn", xv, qv, kb, vb, case.npitch, (1, nk), yv, gamma, case.Tr)
    r = np.random.default_rng(7)
    xbuf = f16(r.standard_normal((T, nq, xp)))
    qbuf = f16(r.standard_normal((T, nq, qp)))
    xbuf[..., xo:xo + DV], qbuf[..., qo:qo + D] = x, q
    ybuf = np.full((T, nq, yp), SENTINEL, np.float16)
    if still_order is not None:
        k, vT = k[list(still_order)], vT[list(still_order)]
    ups, bound = {xv.buf: xbuf, qv.buf: qbuf, yv.buf: ybuf}, {}
    (bound if case.Tr > T else ups).update({kb: k, vb: vT})
    full = run_plan(ctx, WeightPack(), b, ups, {yv.buf: ((T, nq, yp), np.float16)}, n, max_batch=T, bound=bound)[yv.buf]
    return full[:n, :, yo:yo + DV], full


SENTINEL = np.float16(-777.0)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


# ---- ulp rules ----
def ulp16(exact):
    """the fp16 ulp at |exact| (float64): 2^(floor(log2 |exact|) - 10), 2^-24 below the smallest normal number"""
    a = np.abs(np.asarray(exact, np.float64))
    e = np.floor(np.log2(np.where(a > 0, a, 1.0)))
    return np.where(a < 2.0 ** -14, 2.0 ** -24, 2.0 ** (e - 10))


def ulp32(exact):
    a = np.abs(np.asarray(exact, np.float64))
    e = np.floor(np.log2(np.where(a > 0, a, 1.0)))
    return np.where(a < 2.0 ** -126, 2.0 ** -149, 2.0 ** (e - 23))


HALF_ULP_LIMIT = 0.5 + 2.0 ** -10         # a correctly rounded fp16 result of an fp32 value that is itself within 2^-10 fp16 ulp of the exact one


def ulp16_error(got, exact):
    """|got - exact| / ulp16(exact), element-wise (finite values)"""
    exact = np.asarray(exact, np.float64)
    return np.abs(np.asarray(got).astype(np.float64) - exact) / ulp16(exact)


def ulp32_error(got, exact):
    exact = np.asarray(exact, np.float64)
    return np.abs(np.asarray(got).astype(np.float64) - exact) / ulp32(exact)


def all_halves():
    """every fp16 bit pattern once, as a float16 array [65536]"""
    return np.arange(65536, dtype=np.uint16).view(np.float16)


# ---- the output kernel's grid ----
def out_logits():
    """the 52 fp16 logits of the grid: linspace(-4, 4, 45), +-8, +-12, +-65504, -0"""
    v = np.concatenate([np.linspace(-4.0, 4.0, 45), [8.0, -8.0, 12.0, -12.0, 65504.0, -65504.0, -0.0]]).astype(np.float16)
    assert len(v) == 52 and np.signbit(v[-1])
    return v


def out_grid():
    """(rgb uint8 [256][2704][3], ab fp16 [256][2704][2]): row g = grey level g as the pixel (g, g, g), column = every pair of the 52 logits"""
    lg = out_logits()
    a, b = np.meshgrid(lg, lg, indexing="ij")
    ab = np.broadcast_to(np.stack([a.reshape(-1), b.reshape(-1)], -1), (256, 2704, 2)).copy()
    g = np.arange(256, dtype=np.uint8)
    rgb = np.broadcast_to(g[:, None, None], (256, 2704, 3)).copy()
    return rgb, ab


def out_bytes(lab):
    """float32 Lab [..., 3] -> (uint8 RGB as the reference truncates it, the float64 sRGB value before the clip)"""
    from tests.sweep_util import lab2rgb_unclipped
    v = lab2rgb_unclipped(lab)
    return (np.clip(v, 0.0, 1.0) * 255.0).astype(np.int64).astype(np.uint8), v
