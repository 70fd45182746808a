"""Shared by tests/test_retinex_host.py and tests/test_gpu_retinex.py (and tools/retinex_bench.py): the numpy restatement of the MSRCP plugin's pixel work --
THE DEFINITION of HAVC_retinex's stand-in (vsdeoldify_amd/retinex.py says why there is nothing to pin it to) -- with the reference's Python around it, the
test clips, and the cases of tests/golden/retinex.npz.

Per frame, RGB24, every step in the order written, `dtype` float64 (the definition) or float32 (only to measure what float32 would cost):
  I = ((R - sF) + (G - sF) + (B - sF)) * (1.0 / (3 * sR));  per sigma a Young - van Vliet recursive Gaussian, rows then columns, each line forward then
  backward from its own first value;  P = product over the sigmas of (g <= 0 ? 1 : I / g + 1);  O = log(P) / n_sigmas;  4096 bins between the frame's
  extremes, lo / hi where the running count from either end first exceeds int(npix * 0.001 + 0.5);  O' = clamp((O - lo) * (1.0 / (hi - lo)), 0, 1), or I
  when mx <= mn or hi <= lo;  gain = O' / I (1 where I <= 0), at most sR / (max(R, G, B) - sF);  out = clamp(floor((c - sF) * gain * (dR / sR) + dF + 0.5)).
The recursion is vectorised across lines with a Python loop along the line.
"""
import functools
import json
import os

import numpy as np

from oracle import cvcolor
from vsdeoldify_amd import retinex as RX

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BINS = 4096
SIZES = [(7, 5), (64, 64), (65, 130), (33, 257), (96, 200), (3, 1100)]      # h x w: below any tile, one tile, tile + 1 / two tiles + 2, odd, ordinary, long row
SIGMA_SETS = [(25, 80, 250), (0.5, 2.0, 3.0)]                              # the default; both branches of q and the sigma < 1 end


@functools.lru_cache(maxsize=1)
def golden():
    with np.load(os.path.join(GOLDEN, "retinex.npz")) as z:
        d = {k: z[k] for k in z.files}
    return d, [json.loads(str(d[f"case_{i}_params"])) for i in range(int(d["n_cases"]))]


def sum_y(frame):
    return int(cvcolor.cvtColor(np.ascontiguousarray(frame), cvcolor.COLOR_RGB2YUV)[:, :, 0].astype(np.int64).sum())


# ---- the definition ----------------------------------------------------------------------------------------------------------------------------------------
def sweep(x, coef, dtype=np.float64):
    """one pass over the LAST axis of x: forward, then backward in place"""
    B, B1, B2, B3 = (dtype(c) for c in coef)
    y = np.empty_like(x)
    n = x.shape[-1]
    p1 = p2 = p3 = x[..., 0]
    for i in range(n):
        v = ((B * x[..., i] + B1 * p1) + B2 * p2) + B3 * p3
        y[..., i] = v
        p3, p2, p1 = p2, p1, v
    p1 = p2 = p3 = y[..., n - 1].copy()
    for i in range(n - 1, -1, -1):
        v = ((B * y[..., i] + B1 * p1) + B2 * p2) + B3 * p3
        y[..., i] = v
        p3, p2, p1 = p2, p1, v
    return y


def gaussian(plane, sigma, dtype=np.float64):
    """[..., h, w] -> the same: rows, then columns of the result"""
    coef = RX.coefficients(sigma)
    rows = sweep(np.ascontiguousarray(plane, dtype=dtype), coef, dtype)
    return np.ascontiguousarray(np.swapaxes(sweep(np.ascontiguousarray(np.swapaxes(rows, -1, -2)), coef, dtype), -1, -2))


def ranges(fulls, fulld):
    return ((0, 255) if fulls else (16, 219)) + ((0, 255) if fulld else (16, 219))


def intensity(clip, fulls, dtype=np.float64):
    sF, sR = (0, 255) if fulls else (16, 219)
    c = clip.astype(np.int64) - sF
    return (c[..., 0] + c[..., 1] + c[..., 2]).astype(dtype) * dtype(1.0 / (3 * sR))


def planes(clip, sigmas, fulls, dtype=np.float64):
    """clip [n, h, w, 3] -> (I [n, h, w], G [n, n_sigmas, h, w], P [n, h, w])"""
    inten = intensity(clip, fulls, dtype)
    g = np.stack([gaussian(inten, s, dtype) for s in sigmas], 1)
    p = np.ones_like(inten)
    for k in range(len(sigmas)):
        gk = g[:, k]
        with np.errstate(divide="ignore", invalid="ignore"):
            p = p * np.where(gk <= 0, dtype(1), inten / gk + dtype(1))
    return inten, g, p


def msrcp_frame(frame, inten, p, n_sigmas, fulls, fulld, dtype=np.float64, log_shift=None):
    """one frame from its intensity and MSR product.  log_shift: an int array of -1 / 0 / +1 that moves the logarithm by that many ulps (measurement (b))"""
    sF, sR, dF, dR = ranges(fulls, fulld)
    lg = np.log(p)
    if log_shift is not None:
        lg = np.where(log_shift > 0, np.nextafter(lg, np.inf), np.where(log_shift < 0, np.nextafter(lg, -np.inf), lg))
    o = lg / dtype(n_sigmas)
    mn, mx = o.min(), o.max()
    stretched = inten
    if mx > mn:
        bins = ((o - mn) * (dtype(BINS - 1) / (mx - mn))).astype(np.int64)
        count = np.bincount(bins.ravel(), minlength=BINS)
        thr = int(o.size * 0.001 + 0.5)
        k_lo = int(np.argmax(np.cumsum(count) > thr))
        k_hi = BINS - 1 - int(np.argmax(np.cumsum(count[::-1]) > thr))
        lo = dtype(k_lo) / dtype(BINS - 1) * (mx - mn) + mn
        hi = dtype(k_hi) / dtype(BINS - 1) * (mx - mn) + mn
        if hi > lo:
            stretched = np.clip((o - lo) * (dtype(1.0) / (hi - lo)), 0, 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        gain = np.where(inten <= 0, dtype(1), stretched / inten)
    c = frame.astype(np.int64) - sF
    m = c.max(-1)
    with np.errstate(divide="ignore"):
        gain = np.where(m > 0, np.minimum(gain, dtype(sR) / m.astype(dtype)), gain)
    v = np.floor(c.astype(dtype) * gain[..., None] * (dtype(dR) / dtype(sR)) + dtype(dF) + dtype(0.5))
    return np.clip(v, 0, 255).astype(np.uint8)


def msrcp(clip, sigmas=(25, 80, 250), fulls=True, fulld=True, dtype=np.float64, log_seed=None):
    """the plugin's stand-in on a clip [n, h, w, 3] -> uint8 [n, h, w, 3].  log_seed: perturb the logarithm by one ulp up / down / not at all at random"""
    inten, _, p = planes(clip, sigmas, fulls, dtype)
    r = np.random.default_rng(log_seed) if log_seed is not None else None
    return np.stack([msrcp_frame(clip[f], inten[f], p[f], len(sigmas), fulls, fulld, dtype,
                                 None if r is None else r.integers(-1, 2, inten[f].shape)) for f in range(len(clip))])


# ---- the reference's Python around the plugin (pinned by tests/golden/retinex.npz through test_retinex_host.py) -----------------------------------------
def pil_blend(a, b, w):
    """Image.blend(a, b, w) on uint8 arrays: (UINT8)(a + w * (b - a)) in float32"""
    a32, b32 = a.astype(np.float32), b.astype(np.float32)
    return (a32 + np.float32(w) * (b32 - a32)).astype(np.int32).astype(np.uint8)


def around(frame, frame_rtx, luma_dark, luma_bright, range_tv, blend):
    """filter_retinex (vsslib/vsretinex.py:64-84) on one frame and the plugin's frame"""
    _, gate, w = RX.frame_rule(sum_y(frame), frame.shape[0] * frame.shape[1], luma_dark, luma_bright, range_tv, blend)
    if not gate:
        return frame.copy()
    return frame_rtx if w is None else pil_blend(frame, frame_rtx, w)


def retinex_ref(clip, luma_dark=0.20, luma_bright=0.80, sigmas=(25, 80, 250), range_tv_in=True, range_tv_out=True, blend=False, rtx=None):
    """HAVC_retinex on the CPU.  rtx: the stand-in's output when the caller has it already (it does not depend on the gate or the blend)"""
    if rtx is None:
        rtx = msrcp(clip, sigmas, range_tv_in, range_tv_out)
    return np.stack([around(clip[f], rtx[f], luma_dark, luma_bright, range_tv_in, blend) for f in range(len(clip))])


# ---- the test clips ----------------------------------------------------------------------------------------------------------------------------------------
# A constant plane comes out of the float64 recursion constant only to rounding (about 1e-16 relative), unless ((B x + B1 x) + B2 x) + B3 x rounds back to x
# for every sigma: then it is exactly stationary, g = I, P = 2 ** n_sigmas everywhere and the frame takes the mx <= mn path.  Any other constant frame has
# last-place noise in O, mx > mn, and that noise is stretched to the full range (the definition's behaviour on a frame without content).  16 is the one
# level that is stationary for the default sigmas under both source ranges (test_retinex_host.py searches all 255).
CONSTANT_LEVEL = 16
@functools.lru_cache(maxsize=None)
def make_clip(h, w, seed=0):
    """6 frames: gated dark (f_luma < 0.20), gated bright (> 0.80), in the blend zone (0.20 <= f_luma < 0.40), ordinary (>= 0.40), constant (mx <= mn: it
    comes back unchanged -- see CONSTANT_LEVEL: the default bounds gate it out, so the tests of that path open the gate with luma_dark = 0), and a textured frame with runs of pure black pixels (I <= 0) and of pixels with one saturated channel (the sR / m cap).  The levels
    hold for range_tv on and off (`frame_kinds` says what each frame is; the tests assert it).  No sample of a frame that passes the gate lies below 16
    except the pure black runs, which sit next to bright pixels: I / g + 1 stays positive under fulls = False as well (asserted with the planes)."""
    r = np.random.default_rng(7000 * h + w + seed)
    yy, xx = np.mgrid[0:h, 0:w]

    def textured(level, spread):
        base = level + spread * (xx / max(w - 1, 1) - 0.5) + spread * 0.5 * (yy / max(h - 1, 1) - 0.5)
        f = base[:, :, None] + r.integers(-spread // 3, spread // 3 + 1, (h, w, 3))
        f = np.clip(f, 16, 255).astype(np.uint8)
        f[: max(h // 3, 1), : max(w // 4, 1)] = int(level)
        return f
    clip = np.empty((6, h, w, 3), np.uint8)
    clip[0] = textured(30, 18)
    clip[1] = textured(236, 24)
    clip[2] = textured(84, 60)
    clip[3] = textured(140, 90)
    clip[4] = CONSTANT_LEVEL
    f = textured(150, 80)
    # short runs: black, then one saturated channel.  Never on the first sample of a row or a column: the recursion starts from that sample, which then
    # weighs so much at sigma = 250 that under fulls = False (black = -48 / 657) the Gaussian there gets too small for I / g + 1 to stay positive
    for k in range(1, h, 4):
        x0 = 1 + (k * 5) % max(w - 5, 1)
        f[k, x0:x0 + 2] = 0
        f[k, x0 + 2:x0 + 4] = (255, 90, 60)
    clip[5] = f
    clip.setflags(write=False)
    return clip


def frame_kinds(clip, range_tv, luma_dark=0.20, luma_bright=0.80):
    """per frame (f_luma, gate, blend weight with blend=True)"""
    return [RX.frame_rule(sum_y(fr), fr.shape[0] * fr.shape[1], luma_dark, luma_bright, range_tv, True) for fr in clip]


@functools.lru_cache(maxsize=None)
def reference(h, w, sigmas, fulls):
    """(I, G, P) of make_clip(h, w): computed once, shared, read-only"""
    out = planes(make_clip(h, w), sigmas, fulls)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference_bytes(h, w, sigmas, fulls, fulld):
    inten, _, p = reference(h, w, sigmas, fulls)
    clip = make_clip(h, w)
    out = np.stack([msrcp_frame(clip[f], inten[f], p[f], len(sigmas), fulls, fulld) for f in range(len(clip))])
    out.setflags(write=False)
    return out


def count_diff(got, want):
    """(bytes that differ, largest difference)"""
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    return int((d != 0).sum()), int(d.max()) if d.size else 0
