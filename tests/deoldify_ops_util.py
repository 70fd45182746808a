"""Shared by tests/test_gpu_deoldify_ops.py (GPU) and tests/test_deoldify_ops_host.py (CPU): the cases, inputs, one-op plans and error rules by which the
fast-mode non-conv kernels of the DeOldify generator (csrc/attention.hip, the DeOldify half of csrc/elementwise.hip) are held, one op at a time, against
plain float64 (oracle.unet.self_attention_f64 and the few lines of numpy below).

Self-attention.  The kernels have the arithmetic of the DeepRemaster one (64-key tiles, online softmax in fp32, P rounded to fp16, fp32 sums, one fp16
store), so the bound is tests/remaster_util.py's:  2^-11 (|gamma| A + |ref|), A = softmax . |h|, limit 2 x bound.  Inputs are fp16-exact and the reference
is computed from those very values.  In the layer's own names: f = query(x) are the KEYS of the flash kernel, g = key(x) its QUERIES, h its values;
s[j][i] = g_j . f_i, softmax over i.

Element-wise rules are stated with each function; ulp16 is the fp16 ulp AT the exact value."""
from dataclasses import dataclass

import numpy as np

from tests.remaster_util import LIMIT, SENTINEL, attn_bound, attn_ratio, bits, f16, ulp16, ulp16_error  # noqa: F401  (re-exported to the two test files)

GAMMAS = (0.7, -1.3)
PAIRS = ((32, 256), (64, 512), (96, 768),        # C % 256 == 0: self_attention_kernel2 (128 queries x 256 channels per block)
         (32, 128), (64, 384), (96, 128))        # otherwise:    self_attention_kernel  (64 queries x 128 channels per block)
NS = (1, 15, 16, 63, 64, 65, 127, 128, 129, 200, 323)     # around the 64-key tile, the 64-query block of kernel 1 and the 128-query block of kernel 2
TWO_FRAMES = (65, 129, 200)


def pad_to(n, m):
    return (n + m - 1) // m * m


@dataclass(frozen=True)
class AttnCase:
    D: int
    C: int
    N: int
    B: int = 1                   # frames of the net
    batch: int = 0               # frames actually run (0 = B): a short batch on a net of max_batch B
    only: tuple = ()             # regimes, () = every regime the size allows

    @property
    def name(self):
        return f"d{self.D}c{self.C}n{self.N}" + (f"b{self.batch}of{self.B}" if self.batch else "")

    @property
    def frames(self):
        return self.batch or self.B

    @property
    def regimes(self):
        if self.only:
            return self.only
        return ("flat", "sharp", "negative") + (("rising", "falling") if self.N > 64 else ())


CASES = {c.name: c for c in
         [AttnCase(d, c, n, 2 if n in TWO_FRAMES else 1) for d, c in PAIRS for n in NS] +
         [AttnCase(64, 512, 1225, 1, only=("flat",)),                                   # the 35 x 35 grid of render_factor 35: 19 full tiles and a 9-key tail
          AttnCase(64, 512, 129, 3, batch=2), AttnCase(64, 384, 65, 3, batch=2)]}       # short batches, one per kernel


def attn_inputs(case, regime, seed=0):
    """fp16 arrays x [B][N][C], f [B][N][D], g [B][N][D], h [B][N][C].  Frames past case.frames (the short batch) hold 3000 everywhere: nothing may read them."""
    r = np.random.default_rng([seed, case.D, case.C, case.N, case.B, sum(map(ord, regime))])
    B, N, D, C = case.B, case.N, case.D, case.C
    x = r.standard_normal((B, N, C))
    h = r.standard_normal((B, N, C))
    tiles = (N + 63) // 64
    if regime in ("flat", "sharp"):
        sigma = (0.25 if regime == "flat" else 0.9) * (64.0 / D) ** 0.25          # the scores' spread sigma^2 sqrt(D) does not depend on D
        g, f = sigma * r.standard_normal((B, N, D)), sigma * r.standard_normal((B, N, D))
    else:
        # all queries lean the same way, so that the sign / the order of the scores holds for every (query, key) pair
        u = r.standard_normal(D)
        u /= np.linalg.norm(u)
        if regime == "negative":
            g = r.uniform(2.0, 3.0, (B, N, 1)) * u + 0.05 * r.standard_normal((B, N, D))
            f = -r.uniform(5.0, 8.0, (B, N, 1)) * u + 0.05 * r.standard_normal((B, N, D))
        else:
            order = np.arange(tiles)
            if regime == "falling":
                order = order[::-1]
            level = 24.0 * np.repeat(order, 64)[:N, None]                           # per key: 24 x the rank of its tile
            g = r.uniform(1.0, 1.1, (B, N, 1)) * u + 0.02 * r.standard_normal((B, N, D))
            f = level * u + 0.1 * r.standard_normal((B, N, D))
    x, f, g, h = f16(x), f16(f), f16(g), f16(h)
    if case.batch:
        for a in (x, f, g, h):
            a[case.batch:] = np.float16(3000.0)
    return x, f, g, h


def scores(case, f, g):
    """float64 [frames][N queries][N keys]"""
    n = case.frames
    return np.einsum("bjd,bid->bji", g[:n].astype(np.float64), f[:n].astype(np.float64))


def check_regime(case, regime, f, g):
    """the property the regime is named for, on the true scores (so that a test cannot run on inputs that miss it)"""
    s = scores(case, f, g)
    if regime == "flat":
        assert np.abs(s).max() < 4.0, np.abs(s).max()
    elif regime == "sharp":
        assert case.N < 63 or np.abs(s).max() > 20.0, np.abs(s).max()
    elif regime == "negative":
        assert s.max() <= -8.0, s.max()
    else:
        assert case.N > 64
        tiles = (case.N + 63) // 64
        mx = np.stack([s[:, :, t * 64:(t + 1) * 64].max(-1) for t in range(tiles)], -1)          # [frames][N][tile] in walking order
        step = np.diff(mx, axis=-1)
        assert (step >= 20.0).all() if regime == "rising" else (step <= -20.0).all(), (step.min(), step.max())


def attn_reference(case, x, f, g, h, gamma):
    """(out, A) of oracle.unet.self_attention_f64 as [frames][N][C]; gamma as the float32 the op carries"""
    from oracle.unet import self_attention_f64
    gm = float(np.float32(gamma))
    res = [self_attention_f64(x[b], f[b], g[b], h[b], gm) for b in range(case.frames)]
    return np.stack([o for o, _ in res]), np.stack([a for _, a in res])


def attn_worst_text(case, f, g, worst, ratio):
    """the worst element as (frame, query, channel) and the key tile that holds most of its softmax weight"""
    b, j, c = (int(i) for i in worst)
    s = scores(case, f, g)[b, j]
    key = int(np.argmax(s))
    kernel = "kernel 2, block %d wave %d" % (j // 128, j % 128 // 32) if case.C % 256 == 0 else "kernel 1, block %d wave %d" % (j // 64, j % 64 // 16)
    return (f"err / bound {ratio:.3f} (limit {LIMIT}) at frame {b}, query {j} ({kernel}, lane column {j % 16}), channel {c} (16-channel fragment {c // 16}, "
            f"lane group {c % 16 // 4}); heaviest key {key} in tile {key // 64}" + (" (the tail tile)" if key // 64 == (case.N - 1) // 64 and case.N % 64 else ""))


def value_rows(h, npitch, pad=0.0):
    """h [B][N][C] -> V^T [B][C][npitch] fp16, columns N .. npitch filled with `pad` (scalar or array [B][C][npitch - N])"""
    B, N, C = h.shape
    vT = np.empty((B, C, npitch), np.float16)
    vT[:, :, :N] = h.transpose(0, 2, 1)
    vT[:, :, N:] = pad
    return vT


def attention_plan(N, d, C, npitch, gamma, views=False, rows=None):
    """one fast HAVC_OP_ATTENTION on buffers of its own -> (PlanBuilder, x view, qk view, V^T buffer id, y view).
    views: qk at channel offset 64 of a 256-wide row, x at offset C of a 2 C-pitch buffer, y at offset 0 of a 2 C-pitch buffer.
    rows: rows per frame of the qk / x / y buffers (default N; N + 1 = the token-buffer shape: a view that does not fill its buffer's frame)"""
    from vsdeoldify_amd.plan import PlanBuilder, View
    rows = rows or N
    qp, qo, xp, xo, yp, yo = (256, 64, 2 * C, C, 2 * C, 0) if views else (2 * d, 0, C, 0, C, 0)
    b = PlanBuilder()
    xv = View(b.buf(rows * xp), xo, xp, 1, N, C, C)
    qv = View(b.buf(rows * qp), qo, qp, 1, N, 2 * d, 2 * d)
    yv = View(b.buf(rows * yp), yo, yp, 1, N, C, C)
    vb = b.buf(C * npitch + (64 if rows != N else 0))
    b.attention("attn", xv, qv, d, vb, npitch, yv, gamma)
    return b, xv, qv, vb, yv


def run_attention(ctx, x, f, g, vT, gamma, batch=None, views=False):
    """x [B][N][C], f / g [B][N][d], vT [B][C][npitch] (fp16; B = max_batch of the net), the first `batch` frames run
    -> (y [batch][N][C] fp16, the whole y buffer [B][N][pitch] fp16, sentinel-filled before the run)"""
    from tests.gpu_util import run_plan
    from vsdeoldify_amd.plan import WeightPack
    B, N, C = x.shape
    d, npitch = f.shape[-1], vT.shape[-1]
    n = batch or B
    b, xv, qv, vb, yv = attention_plan(N, d, C, npitch, gamma, views)
    r = np.random.default_rng(7)
    xbuf = f16(r.standard_normal((B, N, xv.cpitch)))
    qbuf = f16(r.standard_normal((B, N, qv.cpitch)))
    xbuf[..., xv.coff:xv.coff + C] = x
    qbuf[..., qv.coff:qv.coff + d], qbuf[..., qv.coff + d:qv.coff + 2 * d] = f, g
    ybuf = np.full((B, N, yv.cpitch), SENTINEL, np.float16)
    full = run_plan(ctx, WeightPack(), b, {xv.buf: xbuf, qv.buf: qbuf, yv.buf: ybuf, vb: vT}, {yv.buf: (ybuf.shape, np.float16)}, n, max_batch=B)[yv.buf]
    return full[:n, :, yv.coff:yv.coff + C], full


def emulate_attention(case, x, f, g, h, gamma):
    """self_attention_kernel's / self_attention_kernel2's arithmetic in numpy: per frame, 64-key tiles, masked tail, float32 scores and running
    (m, l, O), P rounded to fp16, one fp16 store (tests/test_remaster_ops_host.py emulate_kernel, for any D and C)"""
    F = np.float32
    out = np.empty((case.frames, case.N, case.C), np.float16)
    for b in range(case.frames):
        qq, xx = g[b].astype(F), x[b].astype(F)
        m, l, o = np.full(case.N, -1e30, F), np.zeros(case.N, F), np.zeros((case.N, case.C), F)
        for kv0 in range(0, case.N, 64):
            kt, vt = f[b, kv0:kv0 + 64].astype(F), h[b, kv0:kv0 + 64].astype(F)
            s = np.full((case.N, 64), -1e30, F)
            s[:, :len(kt)] = qq @ kt.T
            m_new = np.maximum(m, s.max(1))
            alpha = np.exp(m - m_new, dtype=F)
            p = np.exp(s - m_new[:, None], dtype=F)
            l = l * alpha + p.sum(1, dtype=F)
            o = o * alpha[:, None] + p[:, :len(kt)].astype(np.float16).astype(F) @ vt
            m = m_new
        out[b] = (o * (F(gamma) / l)[:, None] + xx).astype(np.float16)
    return out


# ---- element-wise kernels -----------------------------------------------------------------------------------------------------------------------------
SHAPES = ((1, 1), (2, 3), (5, 7), (18, 18), (17, 31))
CHANNELS = (8, 24, 64, 264)          # 64 (and 8): affine_fast_kernel, C / 8 divides 256; 24 and 264: the generic affine_kernel
SENT = bits(np.array([SENTINEL]))[0]


def in_view(values, pitch, coff, fill=SENTINEL):
    """values [..., C] -> a [..., pitch] fp16 buffer image filled with `fill`, the values at channel offset coff"""
    buf = np.full(values.shape[:-1] + (pitch,), fill, np.float16)
    buf[..., coff:coff + values.shape[-1]] = values
    return buf


def outside_is_sentinel(full, coff, C):
    """every element of the destination buffer outside channels coff .. coff + C kept the sentinel it was filled with"""
    out = np.delete(bits(full), np.s_[coff:coff + C], axis=-1)
    return bool((out == SENT).all())


def run_ew(ctx, kind, src, Ho, Wo, scale=None, shift=None, relu=False, batch=None):
    """one MAXPOOL / BLUR_RESIZE / AFFINE / COPY_CH op (kind: "maxpool", "blur", "affine", "copy"): src [B][Hi][Wi][C] fp16 as a view at channel offset 8 of
    a C + 16 pitch buffer -> a view at offset 16 of a C + 24 pitch buffer; both buffers hold the sentinel elsewhere.
    Returns (result [B][Ho][Wo][C], the whole destination buffer [B][Ho][Wo][C + 24])."""
    from tests.gpu_util import run_plan
    from vsdeoldify_amd import _native as nat
    from vsdeoldify_amd.plan import PlanBuilder, View, WeightPack
    B, Hi, Wi, C = src.shape
    pack, b = WeightPack(), PlanBuilder()
    xv = View(b.buf(Hi * Wi * (C + 16)), 8, C + 16, Hi, Wi, C, C)
    yv = View(b.buf(Ho * Wo * (C + 24)), 16, C + 24, Ho, Wo, C, C)
    if kind == "maxpool":
        b.maxpool("op", xv, yv)
    elif kind == "blur":
        b.blur_resize("op", xv, yv)
    elif kind == "affine":
        b.affine("op", xv, yv, pack.add(scale.astype(np.float32)), pack.add(shift.astype(np.float32)), relu)
    else:
        b._op("op", type=nat.OP_COPY_CH, src=xv.buf, src_coff=xv.coff, src_cpitch=xv.cpitch, dst=yv.buf, dst_coff=yv.coff, dst_cpitch=yv.cpitch,
              Hi=Hi, Wi=Wi, Ci=C, Ho=Ho, Wo=Wo, Co=C)
    dst = np.full((B, Ho, Wo, C + 24), SENTINEL, np.float16)
    full = run_plan(ctx, pack, b, {xv.buf: in_view(src, C + 16, 8), yv.buf: dst}, {yv.buf: (dst.shape, np.float16)}, batch or B, max_batch=B)[yv.buf]
    return full[..., 16:16 + C], full


def maxpool_f64(x):
    """MaxPool2d(3, stride 2, pad 1) over the valid taps: x [B][H][W][C] -> float64 [B][Ho][Wo][C]"""
    x = np.asarray(x, np.float64)
    B, H, W, C = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    out = np.empty((B, Ho, Wo, C))
    for ho in range(Ho):
        for wo in range(Wo):
            out[:, ho, wo] = x[:, max(2 * ho - 1, 0):min(2 * ho + 2, H), max(2 * wo - 1, 0):min(2 * wo + 2, W)].max(axis=(1, 2))
    return out


def nearest_index(n_in, n_out):
    """torch 'nearest': min(floor(dst * fp32(in / out)), in - 1), the product in float32"""
    scale = np.float32(n_in) / np.float32(n_out)
    return np.minimum(np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64), n_in - 1)


def blur_resize_f64(x, Ho, Wo):
    """ReplicationPad2d((1, 0, 1, 0)) + AvgPool2d(2, stride 1), then nearest resize to Ho x Wo: x [B][H][W][C] -> float64"""
    x = np.asarray(x, np.float64)
    H, W = x.shape[1:3]
    sy, sx = nearest_index(H, Ho), nearest_index(W, Wo)
    y0, x0 = np.maximum(sy - 1, 0), np.maximum(sx - 1, 0)
    return (x[:, y0][:, :, x0] + x[:, y0][:, :, sx] + x[:, sy][:, :, x0] + x[:, sy][:, :, sx]) / 4.0


def blur_inputs(shape, seed):
    """fp16 integer multiples of 2^-8 with |v| <= 16: the fp32 sum of four and the x 0.25 are exact, the kernel's one rounding is the fp16 store"""
    return (np.random.default_rng(seed).integers(-4096, 4097, shape) / 256.0).astype(np.float16)


def affine_exact(x, scale, shift, relu):
    """float64 x * scale + shift from the fp16 inputs and the float32 constants -> (exact [relu applied], the rule's magnitude |x scale| + |shift|)"""
    prod = x.astype(np.float64) * scale.astype(np.float64)
    v = prod + shift.astype(np.float64)
    return (np.maximum(v, 0.0) if relu else v), np.abs(prod) + np.abs(shift.astype(np.float64))


def affine_excess(got, exact, mag):
    """|got - exact| / (ulp16(exact) / 2 + 2^-22 (|x scale| + |shift|)): half an fp16 ulp is the final rounding, the second term covers the fp32 product and
    sum (2^-24 relative each, on terms no larger than mag), fused or not, with a factor 2 to spare.  <= 1 passes."""
    return np.abs(np.asarray(got).astype(np.float64) - exact) / (ulp16(exact) / 2 + 2.0 ** -22 * mag)


def finite_patterns(shape, seed):
    """fp16 with random finite non-zero bit patterns of either sign (never the sentinel's): a copy is bit-exact or wrong"""
    r = np.random.default_rng(seed)
    p = (r.integers(1, 0x7C00, shape) | (r.integers(0, 2, shape) << 15)).astype(np.uint16)
    p[p == SENT] = 0x3C00
    return p.view(np.float16)


# ---- prep_rgb8 ----
MEAN = np.array([0.485, 0.456, 0.406], np.float32)
STD = np.array([0.229, 0.224, 0.225], np.float32)
PREP_S = 66                            # 66 x 66 = 4356 pixels: 256 greys, the 16^3 lattice, 4 more


def gray_l(rgb):
    """Pillow's rgb2l: (19595 R + 38470 G + 7471 B + 0x8000) >> 16"""
    c = rgb.astype(np.int64)
    return (19595 * c[..., 0] + 38470 * c[..., 1] + 7471 * c[..., 2] + 0x8000) >> 16


def prep_exact(L):
    """float64 (L / 255 - mean) / std with the float32 constants the kernel holds: L [...] -> [..., 3]"""
    return (np.asarray(L, np.float64)[..., None] / 255.0 - MEAN.astype(np.float64)) / STD.astype(np.float64)


def prep_excess(got, exact):
    """|got - exact| / (ulp16(exact) / 2 + 2^-20): the absolute term is two fp32 divisions and a subtraction of values <= 1 (3 x 2^-24), divided by
    std >= 0.224 (x 4.5: 2^-21.2 at most), with a factor 2"""
    return np.abs(np.asarray(got).astype(np.float64) - exact) / (ulp16(exact) / 2 + 2.0 ** -20)


def prep_images():
    """u8 [2][66][66][3]: frame 0 = the 256 greys, then the 16 x 16 x 16 RGB lattice 0, 17, .. 255 (its corners are the cube's), then 4 random pixels;
    frame 1 = random"""
    r = np.random.default_rng(41)
    lv = np.arange(16, dtype=np.uint8) * 17
    lattice = np.stack(np.meshgrid(lv, lv, lv, indexing="ij"), -1).reshape(-1, 3)
    greys = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, 1)
    f0 = np.concatenate([greys, lattice, r.integers(0, 256, (4, 3), dtype=np.uint8)])
    assert len(f0) == PREP_S * PREP_S and {(0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 255)} <= set(map(tuple, lattice))
    return np.stack([f0.reshape(PREP_S, PREP_S, 3), r.integers(0, 256, (PREP_S, PREP_S, 3), dtype=np.uint8)])


def run_prep(ctx, rgb, form):
    """HAVC_OP_PREP_RGB8 on rgb u8 [B][S][S][3]; y0 = a view at offset 8 of a 24-pitch buffer.  form: "single" = no second destination;
    "plain" = second destination at channel 280 of a 320-pitch buffer (560 bytes: not 64-byte aligned, so prep_rgb8_kernel runs although 24 pad
    channels are offered); "fill" = at channel 288 (576 bytes) with y1_fill = 24: prep_rgb8_fill_kernel.
    Returns (y0 buffer [B][S*S][24], y1 buffer [B][S*S][320] or None, the slot's channel offset)."""
    from tests.gpu_util import run_plan
    from vsdeoldify_amd.plan import PlanBuilder, View, WeightPack
    B, S = rgb.shape[:2]
    b = PlanBuilder()
    src = b.buf(S * S * 3, 1)
    y0 = View(b.buf(S * S * 24), 8, 24, S, S, 3, 8)
    slot = {"single": None, "plain": 280, "fill": 288}[form]
    ups = {src: rgb, y0.buf: np.full((B, S * S, 24), SENTINEL, np.float16)}
    downs = {y0.buf: ((B, S * S, 24), np.float16)}
    y1 = None
    if slot is not None:
        y1 = View(b.buf(S * S * 320), slot, 320, S, S, 3, 8)
        ups[y1.buf] = np.full((B, S * S, 320), SENTINEL, np.float16)
        downs[y1.buf] = ((B, S * S, 320), np.float16)
    b.prep_rgb8("prep", src, S, y0, y1, y1_fill=24)
    out = run_plan(ctx, WeightPack(), b, ups, downs, B)
    return out[y0.buf], (out[y1.buf] if y1 else None), slot
