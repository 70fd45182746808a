"""numpy restatement of havc_tweak_clip / havc_rgb_to_yuv420 / havc_yuv420_to_rgb / havc_adjust_rgb_clip (csrc/tweak.hip) and of the reference's Python around
them: THE DEFINITION of the stand-ins for this project (include/havc_mi355.h has it in prose).

UNPINNED -- neither VapourSynth nor zimg can be executed where the fixtures are made.  What stands in for them, every assumption about zimg spelled out:
  * resize.Bicubic(format=YUV420P8, matrix_s="709", range_s="full") -> `rgb_to_yuv420`: BT.709 full range on samples / 255, then the chroma planes 2 : 1 in
    both directions through a separable Mitchell bicubic (b = c = 1/3, zimg's default for Bicubic) stretched by 2 (8 taps), VERTICAL pass first, vertical
    siting centred (centre 2j + 0.5), horizontal siting left (centre 2j: MPEG-2 chroma location, VapourSynth's default), taps outside the plane on the
    mirrored sample (-1 -> 0, n -> n - 1), weights normalised to sum 1, round half to even, no dither on the way down.
  * resize.Bicubic(format=RGB24, matrix_in_s="709", range_s="full", dither_type="error_diffusion") -> `yuv420_to_rgb_float` + `dither_fs`: chroma 1 : 2 with
    the same kernel unstretched (4 taps), vertical first, the inverse matrix, then Floyd - Steinberg error diffusion per plane, rows top to bottom and
    left to right, with the weights 7 / 16 (left), 3 / 16 (top right), 5 / 16 (top), 1 / 16 (top left) on the errors already made.
  * std.Levels(gamma=g) -> the table int(pow(v / 255, 1 / g) * 255 + 0.5) in float64 (`gamma_table`).
  * std.Expr on 8-bit clips -> float32 arithmetic in the expression's own order, one rounding per operation, never fused; stored as clip(rint(.)).
  * std.Lut -> table lookup; std.Merge / std.PlaneStats / "x g *": vsdeoldify_amd.equalize's stand-ins.
All arithmetic is float32 unless stated, a * b + c is a rounded product, then a rounded sum.

PINNED by tests/golden/tweak.npz (made by executing the reference, tools/gen_golden_tweak.py) in tests/test_tweak_host.py: what vsdeoldify_amd/tweak.py
derives -- the gamma handed to std.Levels, the resize arguments, both expression strings, the luma table, the affine expressions, the per-plane gammas, the
normalisation gains and rgb_denoise's calls.  This file takes those from vsdeoldify_amd.tweak, so the pin covers it too."""
import math

import numpy as np

from tests import equalize_util as EU
from vsdeoldify_amd import equalize as EQ
from vsdeoldify_amd import tweak as TW

F32 = np.float32

# ---- constants ------------------------------------------------------------------------------------------------------------------------------------------------
KR, KB = 0.2126, 0.0722                                        # BT.709
KG = 1.0 - KR - KB
CB_DIV, CR_DIV = 2.0 * (1.0 - KB), 2.0 * (1.0 - KR)            # Cb = (b - Y) / CB_DIV
R_CR, B_CB = 2.0 * (1.0 - KR), 2.0 * (1.0 - KB)                # R = Y + R_CR Cr
G_CR, G_CB = 2.0 * (1.0 - KR) * KR / KG, 2.0 * (1.0 - KB) * KB / KG
MITCHELL_B = MITCHELL_C = 1.0 / 3.0
DOWN_TAPS, DOWN_FIRST = 8, -3                                  # taps 2j - 3 .. 2j + 4 of the 2 : 1 pass
UP_TAPS = 4
FS_LEFT, FS_TOPRIGHT, FS_TOP, FS_TOPLEFT = 7.0 / 16.0, 3.0 / 16.0, 5.0 / 16.0, 1.0 / 16.0


def mitchell(x):
    """float64, products and sums in this order (csrc/tweak_ops.h writes the same)"""
    b, c, x = MITCHELL_B, MITCHELL_C, abs(x)
    x2 = x * x
    x3 = x2 * x
    if x < 1.0:
        p0, p1, p2 = (12.0 - 9.0 * b) - 6.0 * c, (-18.0 + 12.0 * b) + 6.0 * c, 6.0 - 2.0 * b
        return ((p0 * x3 + p1 * x2) + p2) / 6.0
    if x < 2.0:
        q0, q1, q2, q3 = -b - 6.0 * c, 6.0 * b + 30.0 * c, -12.0 * b - 48.0 * c, 8.0 * b + 24.0 * c
        return (((q0 * x3 + q1 * x2) + q2 * x) + q3) / 6.0
    return 0.0


def _normalised(w):
    s = 0.0
    for v in w:                                                # in tap order: numpy's sum pairs its terms differently
        s += v
    return np.array([v / s for v in w], np.float64).astype(F32)


def down_weights(centred):
    """the 8 weights of one output sample of the 2 : 1 pass: tap k sits at 2j - 3 + k, the centre at 2j + 0.5 (centred) or 2j (left)"""
    c = 0.5 if centred else 0.0
    return _normalised([mitchell((DOWN_FIRST + k - c) / 2.0) for k in range(DOWN_TAPS)])


def up_weights(centred, odd):
    """the 4 weights of output sample i = 2m + odd of the 1 : 2 pass and the first tap's offset from m.  Centre (i + 0.5) / 2 - 0.5 (centred) or i / 2 (left);
    taps floor(centre) - 1 .. floor(centre) + 2"""
    centre = (odd + 0.5) / 2.0 - 0.5 if centred else odd / 2.0
    first = math.floor(centre) - 1
    return _normalised([mitchell(first + k - centre) for k in range(UP_TAPS)]), first


def mirror(p, n):
    """-1 -> 0, -2 -> 1, n -> n - 1, n + 1 -> n - 2, repeated while outside (planes narrower than the kernel)"""
    while p < 0 or p >= n:
        p = -1 - p if p < 0 else 2 * n - 1 - p
    return p


def _taps(plane, axis, index):
    return np.take(plane, index, axis=axis)


def _down(plane, axis, centred):
    n = plane.shape[axis]
    w = down_weights(centred)
    acc = None
    for k in range(DOWN_TAPS):
        idx = [mirror(2 * j + DOWN_FIRST + k, n) for j in range(n // 2)]
        term = w[k] * _taps(plane, axis, idx)
        acc = term if acc is None else acc + term
    assert acc.dtype == F32
    return acc


def _up(plane, axis, centred):
    n = plane.shape[axis]
    out = np.empty([2 * s if a == axis else s for a, s in enumerate(plane.shape)], F32)
    for odd in (0, 1):
        w, first = up_weights(centred, odd)
        acc = None
        for k in range(UP_TAPS):
            idx = [mirror(m + first + k, n) for m in range(n)]
            term = w[k] * _taps(plane, axis, idx)
            acc = term if acc is None else acc + term
        sel = [slice(None)] * plane.ndim
        sel[axis] = slice(odd, None, 2)
        out[tuple(sel)] = acc
    return out


def _quant(v):
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


# ---- the two halves ----------------------------------------------------------------------------------------------------------------------------------------
def rgb_to_yuv420(rgb):
    """uint8 [..., h, w, 3] -> (y [..., h, w], u, v [..., h / 2, w / 2]) uint8"""
    rgb = np.asarray(rgb)
    h, w = rgb.shape[-3], rgb.shape[-2]
    if h % 2 or w % 2:
        raise ValueError("rgb_to_yuv420: width and height must be even")
    s = rgb.astype(F32) / F32(255)
    r, g, b = s[..., 0], s[..., 1], s[..., 2]
    y = (F32(KR) * r + F32(KG) * g) + F32(KB) * b
    cb = (b - y) / F32(CB_DIV)
    cr = (r - y) / F32(CR_DIV)
    ax_v, ax_h = y.ndim - 2, y.ndim - 1
    cb = _down(_down(cb, ax_v, True), ax_h, False)
    cr = _down(_down(cr, ax_v, True), ax_h, False)
    return _quant(y * F32(255)), _quant(cb * F32(255) + F32(128)), _quant(cr * F32(255) + F32(128))


def yuv420_to_rgb_float(y, u, v):
    """uint8 planes -> (R, G, B) float32 planes in [0, 255] scale (before the dither)"""
    yf = np.asarray(y).astype(F32) / F32(255)
    ax_v, ax_h = yf.ndim - 2, yf.ndim - 1
    cb = (np.asarray(u).astype(F32) - F32(128)) / F32(255)
    cr = (np.asarray(v).astype(F32) - F32(128)) / F32(255)
    cb = _up(_up(cb, ax_v, True), ax_h, False)
    cr = _up(_up(cr, ax_v, True), ax_h, False)
    r = yf + F32(R_CR) * cr
    b = yf + F32(B_CB) * cb
    g = (yf - F32(G_CR) * cr) - F32(G_CB) * cb
    return r * F32(255), g * F32(255), b * F32(255)


def dither_fs(x):
    """float32 [..., h, w] -> uint8: every leading index is a problem of its own (frames, channels)"""
    x = np.asarray(x, F32)
    h, w = x.shape[-2:]
    flat = x.reshape(-1, h, w)
    err = np.zeros((flat.shape[0], h + 1, w + 2), F32)           # row 0 and columns 0, w + 1: the zeros outside the plane
    out = np.empty(flat.shape, np.uint8)
    a, b, c, d = F32(FS_LEFT), F32(FS_TOPRIGHT), F32(FS_TOP), F32(FS_TOPLEFT)
    lo, hi = F32(0), F32(255)
    for i in range(h):
        for j in range(w):
            e = ((err[:, i + 1, j] * a + err[:, i, j + 2] * b) + err[:, i, j + 1] * c) + err[:, i, j] * d
            v = np.minimum(np.maximum(flat[:, i, j] + e, lo), hi)
            q = np.rint(v)
            err[:, i + 1, j + 1] = v - q
            out[:, i, j] = q
    return out.reshape(x.shape)


def yuv420_to_rgb(y, u, v):
    """-> uint8 [..., h, w, 3]"""
    return np.stack([dither_fs(p) for p in yuv420_to_rgb_float(y, u, v)], -1)


# ---- vs_tweak (vsslib/vsfilters.py:753-850) -----------------------------------------------------------------------------------------------------------------
def gamma_table(gamma):
    return TW.gamma_table(gamma)


def hue_sat(u, v, c, s):
    """the two expressions of :809-812 on uint8 planes; c, s: the float64 products hue_cos * sat, hue_sin * sat the reference formats into the strings"""
    c, s = F32(c), F32(s)
    x, y = u.astype(F32) - F32(128), v.astype(F32) - F32(128)
    un = (x * c + y * s) + F32(128)
    vn = (y * c - x * s) + F32(128)
    lim = lambda p: _quant(np.minimum(np.maximum(p, F32(0)), F32(255)))
    return lim(un), lim(vn)


def tweak_float(clip, hue=0, sat=1, bright=0, cont=1, gamma=1):
    """vs_tweak on uint8 [..., h, w, 3], line by line, up to the samples the error diffusion gets: float32 [3, ..., h, w] (None: the neutral call)"""
    plan = TW.tweak_plan(hue, sat, bright, cont, gamma)
    if plan is None:
        return None
    if plan["gamma"] is not None:
        clip = gamma_table(plan["gamma"])[clip]
    y, u, v = rgb_to_yuv420(clip)
    if plan["hue_sat"] is not None:
        u, v = hue_sat(u, v, *plan["hue_sat"])
    if plan["luma_lut"] is not None:
        y = np.asarray(plan["luma_lut"], np.uint8)[y]
    return np.stack(yuv420_to_rgb_float(y, u, v))


def tweak(clip, **kw):
    x = tweak_float(clip, **kw)
    return clip if x is None else np.moveaxis(dither_fs(x), 0, -1)


def tweak_many(clip, sets):
    """tweak for several parameter sets with ONE walk of the error diffusion (its Python loop costs the same for any number of planes)"""
    out = dither_fs(np.stack([tweak_float(clip, **kw) for kw in sets]))
    return [np.moveaxis(o, 0, -1) for o in out]


# ---- HAVC_adjust_rgb (vsdeoldify/__init__.py:1342-1374) -----------------------------------------------------------------------------------------------------
def rgb_normalize(clip):
    """vs_rgb_normalize (vsfilters.py:1013-1038) on uint8 [n, h, w, 3]: the gains are NOT rounded (they reach the expression through repr)"""
    out = []
    for f in clip:
        n = f.shape[0] * f.shape[1]
        avg = [EQ.plane_average(f[:, :, c].sum(dtype=np.int64), n) for c in range(3)]
        gains = TW.normalize_gains(*avg)
        out.append(np.stack([EQ.expr_mul(f[:, :, c], gains[c]) for c in range(3)], -1))
    return np.stack(out)


def affine(v, gain, bias):
    """std.Expr "x r * rb +" on uint8 samples"""
    p = np.asarray(v).astype(F32) * F32(gain) + F32(bias)
    return _quant(p)


def adjust_rgb(clip, strength=0.0, factor=(1.0, 1.0, 1.0), bias=(0, 0, 0), gamma=(1.0, 1.0, 1.0), color_range=None):
    """HAVC_adjust_rgb on uint8 [n, h, w, 3], stage by stage"""
    plan = TW.adjust_plan(factor, bias, gamma, color_range)
    if strength == 1:
        clip = rgb_normalize(clip)
    elif 0 < strength < 1:
        clip = EQ.merge15(clip, rgb_normalize(clip), strength)
    planes = []
    for c in range(3):
        p = affine(clip[..., c], plan["gain"][c], plan["bias"][c])
        if plan["gamma"][c] is not None:
            p = gamma_table(plan["gamma"][c])[p]
        planes.append(p)
    return np.stack(planes, -1)


# ---- HAVC_rgb_denoise (vsdeoldify/__init__.py:924-944 -> havc_utils.py:752-773) ------------------------------------------------------------------------------
def rgb_denoise(clip, denoise_levels=(0.4, 0.3), rgb_factors=(0.95, 1.05, 1.01)):
    clip = EQ.tv_in_table()[clip]
    clip = EU.rgb_balance(clip, denoise_levels[0], [rgb_factors[0], rgb_factors[1], rgb_factors[2]])
    clip = EU.rgb_equalizer(clip, method=0, strength=denoise_levels[1], luma_blend=False, range_tv=True)
    return EQ.tv_out_table()[clip]


# ---- clips ----------------------------------------------------------------------------------------------------------------------------------------------------
def make_clip(h, w, n, seed=0):
    """n frames of seeded noise with a different tint each; the LAST frame is a smooth gradient"""
    r = np.random.default_rng(100000 * h + 10 * w + n + seed)
    clip = r.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    ramp = np.stack([xx * 255.0 / max(w - 1, 1), yy * 255.0 / max(h - 1, 1), (xx + yy) * 255.0 / max(w + h - 2, 1)], -1)
    clip[n - 1] = np.rint(ramp).astype(np.uint8)
    return clip
