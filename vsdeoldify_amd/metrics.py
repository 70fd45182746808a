"""The project's yardstick on the GPU: per-pixel CIEDE2000 between two RGB24 clips.

The contract of this project is a colour difference -- CIEDE2000 below 1.0 per pixel against the reference's fp32 arithmetic -- and `clip_delta_e` measures it
for a whole clip without leaving HBM: one HIP pass in float64 (havc_delta_e_clip, csrc/metrics.hip) that restates oracle/imaging.py delta_e00_images, the
parity metric of BASELINE.json.  Per frame it brings back one small record (sum, max, a 1025-bin histogram in steps of 1/64, and the exact integer sums of
squared byte differences); the per-pixel map is written on request only.

What equals the oracle bit for bit: the sRGB -> linear table (`srgb_linear_table` is the oracle's own numpy expression, uploaded once per context), the
constants and the branches.  What does not: cbrt, hypot, atan2, sin, cos, exp of the device library, and fused multiply-adds; the difference stays below
1e-9 per pixel (tests/test_gpu_metrics.py), nine orders below the contract.  CIEDE2000 itself jumps where two hues are exactly 180 degrees apart; there a
last-bit difference decides the side.

The histogram makes `below(t)` exact for every t that is a multiple of 1/64 up to 16 -- 1.0 among them -- and percentiles exact to a bin.  sum, max and the
histogram do not depend on the order the GPU runs its blocks in: two runs give the same bytes.
"""
import ctypes as C
import math

import numpy as np

BINS = 1025                   # _native.DE_BINS: bin i counts floor(dE * 64) == i, the last one everything at or above 16.0
BIN_SCALE = 64
CONTRACT = 1.0                # the project's limit: CIEDE2000 below 1.0 at every pixel


def _err(msg):
    from .havc import HAVCError
    return HAVCError(msg)


def srgb_linear_table():
    """the sRGB -> linear value of the 256 byte values, float64: oracle/imaging.py srgb_to_lab's expression on np.arange(256)"""
    c = np.arange(256).astype(np.float64) / 255.0
    return np.ascontiguousarray(np.where(c > 0.04045, ((c + 0.055) / 1.055) ** 2.4, c / 12.92))


def _below(hist, t):
    t = float(t)
    if not 0 <= t <= (BINS - 1) / BIN_SCALE:
        raise ValueError(f"below({t}): the histogram resolves 0 .. {(BINS - 1) / BIN_SCALE}")
    total = int(hist.sum())
    return int(hist[:int(math.floor(t * BIN_SCALE))].sum()) / total if total else 0.0


def _percentile(hist, q):
    q = float(q)
    if not 0 <= q <= 100:
        raise ValueError(f"percentile({q}): q is a percentage, 0 .. 100")
    cum = np.cumsum(hist.astype(np.uint64)).tolist()                # Python integers: 100 * count against q * total
    total = cum[-1]
    if total == 0:
        return 0.0
    i = next(i for i, c in enumerate(cum) if c * 100 >= q * total)
    return math.inf if i == BINS - 1 else (i + 1) / BIN_SCALE


def _psnr(sse, n_values):
    sse = np.asarray(sse, np.float64)
    with np.errstate(divide="ignore"):
        return np.where(sse == 0, np.inf, 10.0 * np.log10(255.0 ** 2 * n_values / np.where(sse == 0, 1.0, sse)))


class DeltaEReport:
    """what clip_delta_e returns.  recs: the per-frame records (_native.DE_REC_DTYPE), n_pixels: pixels per frame, map: None, an ndarray or a DevicePlane
    of float64 [n, h, w] ([h, w] for a single frame).

    per frame (arrays of n):  mean, max, psnr (dB over the three channels, inf for equal frames), hist [n, 1025]
    whole clip:               clip_mean, clip_max, clip_psnr, clip_hist (the summed integer histograms), meets_contract (clip_max < 1.0)
    below(t), percentile(q):  of the clip, or of frame `frame`"""

    def __init__(self, recs, n_pixels, map=None):
        self.recs, self.n_pixels, self.map = recs, int(n_pixels), map

    @property
    def n_frames(self):
        return len(self.recs)

    @property
    def mean(self):
        return self.recs["sum"] / float(self.n_pixels)

    @property
    def max(self):
        return self.recs["max"].copy()

    @property
    def hist(self):
        return self.recs["hist"]

    @property
    def psnr(self):
        return _psnr(self.recs["sse"].sum(axis=1, dtype=np.uint64), 3 * self.n_pixels)

    @property
    def clip_hist(self):
        return self.recs["hist"].sum(axis=0, dtype=np.uint64)

    @property
    def clip_mean(self):
        return math.fsum(self.recs["sum"].tolist()) / (float(self.n_pixels) * self.n_frames)

    @property
    def clip_max(self):
        return float(self.recs["max"].max())

    @property
    def clip_psnr(self):
        return float(_psnr(self.recs["sse"].sum(dtype=np.uint64), 3 * self.n_pixels * self.n_frames))

    @property
    def meets_contract(self):
        return self.clip_max < CONTRACT

    def _hist(self, frame):
        return self.clip_hist if frame is None else self.recs["hist"][frame]

    def below(self, t, frame=None):
        """the share of pixels with dE < t: exact when t is a multiple of 1/64 (0 .. 16); any other t counts the bins that lie entirely below it"""
        return _below(self._hist(frame), t)

    def percentile(self, q, frame=None):
        """the upper edge of the bin in which the cumulative count reaches q per cent of the pixels (inf: it is reached only at or above 16.0)"""
        return _percentile(self._hist(frame), q)

    def table(self):
        """the figures as text: one line per frame, then the clip"""
        rows = ["frame        mean       max   below 1.0       p99    PSNR dB"]
        line = "{:>5} {:>11.6f} {:>9.4f} {:>11.6f} {:>9.4f} {:>10.2f}".format
        mean, mx, ps = self.mean, self.max, self.psnr
        for f in range(self.n_frames):
            rows.append(line(f, mean[f], mx[f], self.below(CONTRACT, f), self.percentile(99, f), ps[f]))
        rows.append(line("clip", self.clip_mean, self.clip_max, self.below(CONTRACT), self.percentile(99), self.clip_psnr))
        rows.append(f"contract (max < {CONTRACT}): {'met' if self.meets_contract else 'NOT met'}")
        return "\n".join(rows)


def check_clips(a, b):
    """the refusals, before anything touches the GPU -> (shape, n_frames)"""
    from .device import is_device
    for name, x in (("a", a), ("b", b)):
        if not (is_device(x) or isinstance(x, np.ndarray)):
            raise _err(f"clip_delta_e: this is not a clip: {name}")
    for x in (a, b):
        if len(x.shape) not in (3, 4) or x.shape[-1] != 3 or (not is_device(x) and x.dtype != np.uint8):
            raise _err("clip_delta_e: only RGB24 clips (uint8 [n, h, w, 3]) are supported")
    if tuple(a.shape) != tuple(b.shape):
        raise _err(f"clip_delta_e: a {tuple(a.shape)} and b {tuple(b.shape)} differ in shape")
    shape = tuple(int(s) for s in a.shape)
    if len(shape) == 4 and shape[0] == 0:
        raise _err("clip_delta_e: a clip of zero frames")
    if shape[-3] < 1 or shape[-2] < 1:
        raise _err("clip_delta_e: a frame of zero pixels")
    return shape, (shape[0] if len(shape) == 4 else 1)


def _table_once(ctx):
    """the oracle's table, uploaded once per context"""
    from . import _native as nat
    if not ctx.__dict__.get("_de_table"):
        nat.check(ctx.lib.havc_delta_e_set_table(ctx.h, nat.as_ptr(srgb_linear_table())), ctx.h)
        ctx.__dict__["_de_table"] = True


def delta_e_np(ctx, a, b, return_map=False):
    """havc_delta_e_clip on checked operands of one context -> DeltaEReport.  Two DeviceImages: the map is a DevicePlane and the call blocks only for the
    records; with an ndarray among the operands the map is an ndarray."""
    from . import _native as nat
    from .device import is_device, operand_ptr
    from .vformat import DevicePlane
    shape, n = check_clips(a, b)
    a, b = (x if is_device(x) else np.ascontiguousarray(x) for x in (a, b))
    _table_once(ctx)
    recs = np.zeros(n, nat.DE_REC_DTYPE)
    dmap = None
    if return_map:
        dmap = DevicePlane(ctx, shape[:-1], np.float64) if is_device(a) and is_device(b) else np.empty(shape[:-1], np.float64)
    mp = None if dmap is None else (dmap.ptr if isinstance(dmap, DevicePlane) else nat.as_ptr(dmap))
    nat.check(ctx.lib.havc_delta_e_clip(ctx.h, operand_ptr(a), operand_ptr(b), shape[-2], shape[-3], n, nat.as_ptr(recs), mp), ctx.h)
    return DeltaEReport(recs, shape[-3] * shape[-2], dmap)


def clip_delta_e(a, b, *, device_index=0, return_map=False):
    """CIEDE2000 between two RGB24 clips of equal shape, uint8 [n, h, w, 3] or a single frame [h, w, 3], each an ndarray or a DeviceImage -> DeltaEReport.
    Nothing but the per-frame records leaves the GPU, unless return_map asks for the float64 map of an ndarray operand."""
    from .device import is_device
    check_clips(a, b)
    devs = [x for x in (a, b) if is_device(x)]
    if len(devs) == 2 and devs[0].ctx is not devs[1].ctx:
        raise _err("clip_delta_e: a and b live on different contexts")
    if devs:
        ctx = devs[0].ctx
    else:
        from .render import get_context
        ctx = get_context(device_index)
    return delta_e_np(ctx, a, b, return_map)
