"""What the tests of clip_delta_e (csrc/metrics.hip, vsdeoldify_amd/metrics.py) share: the oracle and its intermediates, the inputs, the restatement of the
kernel's fixed-order sum, and the stand-alone host build of csrc/metrics_ops.h.

The oracle is oracle/imaging.py delta_e00_images, float64 numpy.  LIMIT is the per-pixel bound against it: the expected difference is a few ulp of the math
library and of FMA contraction on values up to 360, about 1e-12; 1e-9 sits three orders above that, seven below the histogram's bin width and nine below the
contract.  It is a margin, not a measurement (profiles/delta_e.txt has the measured maximum).

CIEDE2000 jumps where the two hues are exactly 180 degrees apart: pixels whose oracle |abs(h1' - h2') - 180| < HUE_EPS degrees are left out of the per-pixel
comparison, and at most HUE_CAP of the pixels may be.  The structured inputs here are chosen so that none is (checked on the CPU, asserted as 0)."""
import os
import subprocess

import numpy as np

from oracle import imaging

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 1e-9
HUE_EPS = 1e-6
HUE_CAP = 1e-5
BINS = 1025
BLOCK_THREADS, THREAD_PIXELS = 256, 4                      # csrc/metrics.hip: a block is 256 threads of 4 pixels


def oracle_map(a, b):
    """float64 dE of every pixel, frame by frame (the oracle's arrays of a whole clip at once would be large)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.ndim == 3:
        return imaging.delta_e00_images(a, b)
    return np.stack([imaging.delta_e00_images(x, y) for x, y in zip(a, b)])


def oracle_intermediates(a, b):
    """the values the oracle's np.where conditions look at, from its own srgb_to_lab and the first statements of its ciede2000 (oracle/imaging.py:59-75)"""
    lab1, lab2 = imaging.srgb_to_lab(a), imaging.srgb_to_lab(b)
    a1, b1, a2, b2 = lab1[..., 1], lab1[..., 2], lab2[..., 1], lab2[..., 2]
    C1, C2 = np.hypot(a1, b1), np.hypot(a2, b2)
    Cb = (C1 + C2) / 2
    G = 0.5 * (1 - np.sqrt(Cb ** 7 / (Cb ** 7 + 25.0 ** 7)))
    a1p, a2p = (1 + G) * a1, (1 + G) * a2
    C1p, C2p = np.hypot(a1p, b1), np.hypot(a2p, b2)
    h1p = np.degrees(np.arctan2(b1, a1p)) % 360
    h2p = np.degrees(np.arctan2(b2, a2p)) % 360
    return dict(cc=C1p * C2p, dh=h2p - h1p, habs=np.abs(h1p - h2p), hs=h1p + h2p)


def branch_counts(a, b):
    """pixels in every branch of the oracle's np.where's: the sRGB and Lab pieces (per sample), the three of dh and the three of hbp with the achromatic one"""
    out = {}
    for name, x in (("a", a), ("b", b)):
        c = np.asarray(x).astype(np.float64) / 255.0
        lin = np.where(c > 0.04045, ((c + 0.055) / 1.055) ** 2.4, c / 12.92)
        M = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]])
        xyz = lin @ M.T / np.array([0.95047, 1.0, 1.08883])
        out[f"srgb_pow_{name}"], out[f"srgb_lin_{name}"] = int((c > 0.04045).sum()), int((c <= 0.04045).sum())
        out[f"lab_cbrt_{name}"], out[f"lab_lin_{name}"] = int((xyz > 0.008856).sum()), int((xyz <= 0.008856).sum())
    v = oracle_intermediates(a, b)
    chroma = v["cc"] != 0
    out["achromatic"] = int((~chroma).sum())
    out["dh_gt_180"] = int((chroma & (v["dh"] > 180)).sum())
    out["dh_lt_m180"] = int((chroma & ~(v["dh"] > 180) & (v["dh"] < -180)).sum())
    out["dh_plain"] = int((chroma & ~(v["dh"] > 180) & ~(v["dh"] < -180)).sum())
    out["hbp_half"] = int((chroma & (v["habs"] <= 180)).sum())
    out["hbp_plus"] = int((chroma & ~(v["habs"] <= 180) & (v["hs"] < 360)).sum())
    out["hbp_minus"] = int((chroma & ~(v["habs"] <= 180) & ~(v["hs"] < 360)).sum())
    return out


def hue_excluded(a, b):
    """bool per pixel: the documented discontinuity (module docstring)"""
    v = oracle_intermediates(a, b)
    return (v["cc"] != 0) & (np.abs(v["habs"] - 180) < HUE_EPS)


def compare_maps(got, a, b, want=None):
    """-> (largest |got - oracle| over the compared pixels, share of pixels left out); asserts the cap"""
    want = oracle_map(a, b) if want is None else want
    skip = hue_excluded(a, b)
    share = float(skip.mean())
    assert share <= HUE_CAP, share
    err = np.abs(np.asarray(got) - want)
    assert not np.isnan(err[~skip]).any()
    return (float(err[~skip].max()) if (~skip).any() else 0.0), share


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------------------------
def palette():
    """the 5-bit-per-channel grid (32768 colours, 0 and 255 among the levels), the 256 greys, black and white: uint8 [33026, 3]"""
    lv = (np.arange(32) * 255 // 31).astype(np.uint8)
    grid = np.stack(np.meshgrid(lv, lv, lv, indexing="ij"), -1).reshape(-1, 3)
    grey = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, 1)
    return np.concatenate([grid, grey, np.array([[0, 0, 0], [255, 255, 255]], np.uint8)])


BANDS = dict(same=(0, 128), near=(128, 384), black=(384, 512), swap=(512, 768), far=(768, 1024))          # rows of the structured frame


def structured_pair(side=1024):
    """(a, b) uint8 [side, side, 3].  a walks the palette over and over; b, by bands of rows: a itself | a +- 1..3 per channel | black | a with R and B
    swapped (hue differences on both sides of +-180, hue sums on both sides of 360) | another palette colour (large differences, the overflow bin)"""
    pal = palette()
    n = side * side
    idx = np.arange(n) % len(pal)
    a = pal[idx].reshape(side, side, 3)
    b = a.copy()
    r = np.random.default_rng(2000)
    rows = {k: (lo * side // 1024, hi * side // 1024) for k, (lo, hi) in BANDS.items()}
    lo, hi = rows["near"]
    step = r.integers(1, 4, (hi - lo, side, 3)) * r.choice([-1, 1], (hi - lo, side, 3))
    b[lo:hi] = np.clip(a[lo:hi].astype(np.int64) + step, 0, 255).astype(np.uint8)
    lo, hi = rows["black"]
    b[lo:hi] = 0
    lo, hi = rows["swap"]
    b[lo:hi] = a[lo:hi, :, ::-1]
    lo, hi = rows["far"]
    b[lo:hi] = pal[(idx * 7919 + 12345) % len(pal)].reshape(side, side, 3)[lo:hi]
    return np.ascontiguousarray(a), np.ascontiguousarray(b), rows


def random_pair(shape, seed):
    """two uint8 clips of `shape`: b is a within +-6 on most pixels, anything on some, a itself on some"""
    r = np.random.default_rng(seed)
    a = r.integers(0, 256, shape, dtype=np.uint8)
    near = np.clip(a.astype(np.int64) + r.integers(-6, 7, shape), 0, 255).astype(np.uint8)
    far = r.integers(0, 256, shape, dtype=np.uint8)
    pick = r.integers(0, 8, shape[:-1])[..., None]
    b = np.where(pick == 0, far, np.where(pick == 1, a, near))
    return a, np.ascontiguousarray(b)


# ---- the kernel's record, restated from its own map ------------------------------------------------------------------------------------------------------------
def fixed_order_sum(frame_map):
    """the sum of one frame as csrc/metrics.hip adds it: blocks of 1024 pixels; thread t of a block adds its four pixels in order, starting from 0.0 (a pixel
    beyond the frame adds nothing); the 256 thread sums fold as v[t] += v[t + s] for s = 128, 64 .. 1; the block sums are added in block order from 0.0"""
    v = np.asarray(frame_map, np.float64).reshape(-1)
    per = BLOCK_THREADS * THREAD_PIXELS
    nb = (len(v) + per - 1) // per
    p = np.zeros(nb * per, np.float64)
    p[:len(v)] = v
    p = p.reshape(nb, BLOCK_THREADS, THREAD_PIXELS)
    t = np.zeros((nb, BLOCK_THREADS), np.float64)
    for k in range(THREAD_PIXELS):
        t = t + p[:, :, k]
    s = BLOCK_THREADS // 2
    while s:
        t[:, :s] = t[:, :s] + t[:, s:2 * s]
        s //= 2
    total = np.float64(0.0)
    for x in t[:, 0]:
        total = total + x
    return float(total)


def records_from_map(dmap, a, b):
    """what the records must be, exactly, given the kernel's own map [n, h, w] and the clips: dict(hist [n, 1025], max [n], sse [n, 3], sum [n])"""
    dmap = np.asarray(dmap)
    n = dmap.shape[0]
    bins = np.minimum(np.floor(dmap * 64), BINS - 1).astype(np.int64).reshape(n, -1)
    d = a.astype(np.int64) - b.astype(np.int64)
    return dict(hist=np.stack([np.bincount(x, minlength=BINS) for x in bins]), max=dmap.reshape(n, -1).max(axis=1),
                sse=(d * d).reshape(n, -1, 3).sum(axis=1), sum=np.array([fixed_order_sum(m) for m in dmap]))


def check_records(rep, dmap, a, b):
    """the records of a DeltaEReport against the kernel's own map (all exact but the last line)"""
    a, b, dmap = np.asarray(a), np.asarray(b), np.asarray(dmap)
    if a.ndim == 3:
        a, b, dmap = a[None], b[None], dmap[None]
    want = records_from_map(dmap, a, b)
    recs = rep.recs
    assert np.array_equal(recs["hist"], want["hist"])
    assert recs["hist"].sum(axis=1).tolist() == [dmap[0].size] * len(recs)
    assert np.array_equal(recs["max"], want["max"])
    assert np.array_equal(recs["sse"].astype(np.int64), want["sse"])
    assert recs["sum"].tobytes() == want["sum"].tobytes(), (recs["sum"], want["sum"])
    ref = dmap.reshape(len(recs), -1).sum(axis=1)
    assert np.all(np.abs(recs["sum"] - ref) <= 1e-9 * np.abs(ref))
    assert not recs["reserved"].any()


# ---- the host build of csrc/metrics_ops.h ------------------------------------------------------------------------------------------------------------------------
HOST_MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include "metrics_ops.h"
// argv: table (256 float64), pairs (n x 6 bytes: r g b of a, r g b of b), out (n float64 dE, n int32 bins); "-" as the table: the library's own formula
int main(int argc, char** argv) {
    if (argc != 5) return 2;
    const long n = atol(argv[4]);
    double lin[256];
    FILE* f;
    if (argv[1][0] == '-') { for (int v = 0; v < 256; ++v) lin[v] = de_srgb_linear(v); }
    else { f = fopen(argv[1], "rb"); if (!f || fread(lin, 8, 256, f) != 256) return 3; fclose(f); }
    uint8_t* px = (uint8_t*)malloc((size_t)n * 6);
    double* de = (double*)malloc((size_t)n * 8);
    int* bin = (int*)malloc((size_t)n * 4);
    f = fopen(argv[2], "rb"); if (!f || (long)fread(px, 6, (size_t)n, f) != n) return 4; fclose(f);
    for (long i = 0; i < n; ++i) { de[i] = de_pixel(lin, px + 6 * i, px + 6 * i + 3); bin[i] = de_bin(de[i]); }
    f = fopen(argv[3], "wb"); if (!f || (long)fwrite(de, 8, (size_t)n, f) != n || (long)fwrite(bin, 4, (size_t)n, f) != n) return 5; fclose(f);
    free(px); free(de); free(bin);
    return 0;
}
"""


def build_host(tmp, flags=("-O2",)):
    """compile csrc/metrics_ops.h with a main of its own (g++, no GPU toolchain) -> path of the program"""
    src, exe = os.path.join(tmp, "de_host.cpp"), os.path.join(tmp, "de_host")
    with open(src, "w") as f:
        f.write(HOST_MAIN)
    subprocess.check_call(["g++", "-std=c++17", *flags, "-I", os.path.join(ROOT, "vsdeoldify_amd", "csrc"), src, "-o", exe, "-lm"])
    return exe


def run_host(exe, tmp, a, b, table=None):
    """the host build on two uint8 arrays [..., 3] -> (dE float64 [...], bins int32 [...])"""
    a, b = np.asarray(a, np.uint8), np.asarray(b, np.uint8)
    n = a.size // 3
    tp, pp, op = (os.path.join(tmp, x) for x in ("table.bin", "pairs.bin", "out.bin"))
    if table is not None:
        np.asarray(table, np.float64).tofile(tp)
    np.concatenate([a.reshape(-1, 3), b.reshape(-1, 3)], 1).tofile(pp)
    subprocess.check_call([exe, tp if table is not None else "-", pp, op, str(n)])
    raw = open(op, "rb").read()
    return np.frombuffer(raw[:8 * n], np.float64).reshape(a.shape[:-1]), np.frombuffer(raw[8 * n:], np.int32).reshape(a.shape[:-1])
