"""numpy restatement of havc_planes_to_rgb24 / havc_rgb24_to_planes (csrc/vformat.hip): THE DEFINITION of the two conversions convert_format_RGB24 /
restore_format (vsdeoldify/havc_utils.py:57-237) ask zimg for, on a clip's own planes.  Built on tests/tweak_util.py by import: the Mitchell resampler
(`_up`, `_down`), the mirroring and the Floyd - Steinberg weights are that file's, and so is the float32 discipline (a * b + c is a rounded product, then a
rounded sum).

UNPINNED -- zimg cannot be executed where the fixtures are made.  On top of tweak_util's assumptions this file WRITES DOWN, as this project's stand-in:
  * the matrices: KR, KB = 0.2126, 0.0722 (709), 0.299, 0.114 (470bg, 170m), 0.2627, 0.0593 (2020ncl); every derived constant in float64, then float32.
  * to codes at depth b (`rgb_to_planes`): limited Y 219 2^(b-8) + 16 2^(b-8), C 224 2^(b-8) + 2^(b-1); full Y (2^b - 1) + 0, C (2^b - 1) + 2^(b-1); then
    round half to even and clip to [0, 2^b - 1] (dither 0), or the error diffusion clamped to that interval (dither 1): Y over w x h, U and V each over
    their own plane in raster order.
  * from codes (`planes_to_rgb`): more than 8 bit goes to 8 bit first, in a step of its own as the reference asks (:129-130), no dither: limited v 2^-(b-8);
    full luma v (255 / (2^b - 1)), full chroma ((v - 2^(b-1)) (255 / (2^b - 1))) + 128; clip(rint(.), 0, 255).  Then Y = (y - 16) / 219, C = (c - 128) / 224
    (limited) or Y = (y - 0) / 255, C = (c - 128) / 255 (full), the chroma 1 : 2 where it is subsampled (vertical pass first), the inverse matrix times 255.
  * GRAY -> RGB24 (`gray_to_rgb`): R = G = B = clip(rint(((y8 - 16) / 219) 255)), no dither (:144-150).
At 709 / full / 8 bit / 4:2:0 the bytes are those of tweak_util.yuv420_to_rgb and tweak_util.rgb_to_yuv420 (tests/test_vformat_host.py).

PINNED by tests/golden/vformat.json (tools/gen_golden_vformat.py executes the reference): WHICH conversions run, in which order and with which arguments --
vsdeoldify_amd/vformat.py's plans, which `convert` / `restore` below take from that module."""
import numpy as np

from tests import tweak_util as TU

F32 = np.float32
MATRICES = {"709": (0.2126, 0.0722), "470bg": (0.299, 0.114), "170m": (0.299, 0.114), "2020ncl": (0.2627, 0.0593)}


def _matrix(matrix):
    kr, kb = MATRICES[matrix]
    kg = 1.0 - kr - kb
    return dict(kr=kr, kg=kg, kb=kb, cb_div=2.0 * (1.0 - kb), cr_div=2.0 * (1.0 - kr), r_cr=2.0 * (1.0 - kr), b_cb=2.0 * (1.0 - kb),
                g_cr=2.0 * (1.0 - kr) * kr / kg, g_cb=2.0 * (1.0 - kb) * kb / kg)


def _quant(v, hi):
    return np.clip(np.rint(v), 0, hi).astype(np.uint8 if hi <= 255 else np.uint16)


def depth_to_8(plane, bits, full, chroma):
    """the depth step of its own: a plane of `bits` > 8 as 8-bit codes, in the clip's own range, no dither"""
    plane = np.asarray(plane)
    if bits == 8:
        return plane.astype(np.uint8)
    v = plane.astype(F32)
    if not full:
        p = v * F32(1.0 / (1 << (bits - 8)))
    elif not chroma:
        p = v * F32(255.0 / ((1 << bits) - 1))
    else:
        p = (v - F32(1 << (bits - 1))) * F32(255.0 / ((1 << bits) - 1)) + F32(128)
    return _quant(p, 255)


def dither_fs(x, hi):
    """tweak_util.dither_fs with the clamp at [0, hi]: float32 [..., h, w] -> uint8 (hi <= 255) or uint16, every leading index a problem of its own"""
    x = np.asarray(x, F32)
    h, w = x.shape[-2:]
    flat = x.reshape(-1, h, w)
    err = np.zeros((flat.shape[0], h + 1, w + 2), F32)
    out = np.empty(flat.shape, np.uint8 if hi <= 255 else np.uint16)
    a, b, c, d = F32(TU.FS_LEFT), F32(TU.FS_TOPRIGHT), F32(TU.FS_TOP), F32(TU.FS_TOPLEFT)
    lo, top = F32(0), F32(hi)
    for i in range(h):
        for j in range(w):
            e = ((err[:, i + 1, j] * a + err[:, i, j + 2] * b) + err[:, i, j + 1] * c) + err[:, i, j] * d
            v = np.minimum(np.maximum(flat[:, i, j] + e, lo), top)
            q = np.rint(v)
            err[:, i + 1, j + 1] = v - q
            out[:, i, j] = q
    return out.reshape(x.shape)


def planes_to_rgb_float(y, u, v, sub_w, sub_h, bits=8, matrix="709", full_range=False, depth_full_range=False):
    """planes [..., h, w] / [..., h >> sub_h, w >> sub_w] -> (R, G, B) float32 in [0, 255] scale, before the rounding or the dither"""
    m = _matrix(matrix)
    y8, u8, v8 = depth_to_8(y, bits, depth_full_range, False), depth_to_8(u, bits, depth_full_range, True), depth_to_8(v, bits, depth_full_range, True)
    y_off, y_scale, c_scale = (0, 255, 255) if full_range else (16, 219, 224)
    yf = (y8.astype(F32) - F32(y_off)) / F32(y_scale)
    ax_v, ax_h = yf.ndim - 2, yf.ndim - 1
    cc = []
    for p in (u8, v8):
        c = (p.astype(F32) - F32(128)) / F32(c_scale)
        if sub_h:
            c = TU._up(c, ax_v, True)
        if sub_w:
            c = TU._up(c, ax_h, False)
        cc.append(c)
    cb, cr = cc
    r = yf + F32(m["r_cr"]) * cr
    b = yf + F32(m["b_cb"]) * cb
    g = (yf - F32(m["g_cr"]) * cr) - F32(m["g_cb"]) * cb
    return r * F32(255), g * F32(255), b * F32(255)


def planes_to_rgb(y, u, v, sub_w, sub_h, bits=8, matrix="709", full_range=False, depth_full_range=False, dither=True):
    """-> uint8 [..., h, w, 3]"""
    x = planes_to_rgb_float(y, u, v, sub_w, sub_h, bits, matrix, full_range, depth_full_range)
    x = np.stack(x)                                                 # one walk of the error diffusion for the three channels (its Python loop is the cost)
    return np.moveaxis(dither_fs(x, 255) if dither else _quant(x, 255), 0, -1)


def gray_to_rgb(y, bits=8, depth_full_range=False):
    y8 = depth_to_8(y, bits, depth_full_range, False)
    q = _quant(((y8.astype(F32) - F32(16)) / F32(219)) * F32(255), 255)
    return np.stack([q, q, q], -1)


def rgb_to_planes(rgb, sub_w, sub_h, bits=8, matrix="709", full_range=False, dither=True):
    """uint8 [..., h, w, 3] -> (y, u, v) codes of `bits` (uint8 for 8, uint16 above)"""
    rgb = np.asarray(rgb)
    m = _matrix(matrix)
    s = rgb.astype(F32) / F32(255)
    r, g, b = s[..., 0], s[..., 1], s[..., 2]
    y = (F32(m["kr"]) * r + F32(m["kg"]) * g) + F32(m["kb"]) * b
    cb = (b - y) / F32(m["cb_div"])
    cr = (r - y) / F32(m["cr_div"])
    ax_v, ax_h = y.ndim - 2, y.ndim - 1
    if sub_h:
        cb, cr = TU._down(cb, ax_v, True), TU._down(cr, ax_v, True)
    if sub_w:
        cb, cr = TU._down(cb, ax_h, False), TU._down(cr, ax_h, False)
    top, step = (1 << bits) - 1, 1 << (bits - 8)
    ys, yo, cs = (float(top), 0.0, float(top)) if full_range else (219.0 * step, 16.0 * step, 224.0 * step)
    co = float(1 << (bits - 1))
    yp, cp = y * F32(ys) + F32(yo), np.stack([cb * F32(cs) + F32(co), cr * F32(cs) + F32(co)])
    if not dither:
        return _quant(yp, top), _quant(cp[0], top), _quant(cp[1], top)
    c = dither_fs(cp, top)                                          # U and V: two problems, one walk
    return dither_fs(yp, top), c[0], c[1]


# ---- the reference's two functions as compositions of the above, following vsdeoldify_amd/vformat.py's plans (pinned by tests/golden/vformat.json) ----------
def convert(planes, fmt, matrix=None, color_range=None):
    """convert_format_RGB24 on host planes -> uint8 [n, h, w, 3]"""
    from vsdeoldify_amd import vformat as VF
    steps = VF.convert_steps(fmt, matrix, color_range)
    f = VF.FORMATS[fmt]
    if f["family"] == "GRAY":
        return gray_to_rgb(planes[0], f["bits"], steps["depth_full_range"])
    return planes_to_rgb(*planes, f["sub_w"], f["sub_h"], f["bits"], steps["matrix"], steps["full_range"], steps["depth_full_range"], steps["dither"])


def restore(rgb, fmt, matrix=None, color_range=None):
    """restore_format of an RGB24 clip to what `convert` of (fmt, matrix, color_range) remembered -> (format name, planes)"""
    from vsdeoldify_amd import vformat as VF
    steps = VF.restore_steps(fmt, matrix, color_range)
    f = VF.FORMATS[steps["format"]]
    return steps["format"], rgb_to_planes(rgb, f["sub_w"], f["sub_h"], f["bits"], steps["matrix"], steps["full_range"], steps["dither"])


def make_planes(fmt_bits, sub_w, sub_h, n, h, w, seed=0, gray=False, extremes=False):
    """seeded random codes of `fmt_bits`; extremes: only 0 and the maximum code (out of a limited range: every clamp is hit)"""
    r = np.random.default_rng(1000 * h + 10 * w + n + 7 * fmt_bits + seed)
    top, dt = (1 << fmt_bits) - 1, np.uint8 if fmt_bits == 8 else np.uint16
    shapes = [(n, h, w)] if gray else [(n, h, w), (n, h >> sub_h, w >> sub_w), (n, h >> sub_h, w >> sub_w)]
    if extremes:
        return tuple((r.integers(0, 2, s) * top).astype(dt) for s in shapes)
    return tuple(r.integers(0, top + 1, s).astype(dt) for s in shapes)
