"""numpy restatement of havc_scene_stats (csrc/scdetect.hip) and the clips the scene-detection tests share.  The normalisation is written as the
reference writes it (vsutils.frame_normalize, vsutils.py:304-318): numpy's own float64 expression on the uint8 plane."""
import functools
import json
import os

import numpy as np

from vsdeoldify_amd import scdetect as SD

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scdetect.npz")


@functools.lru_cache(maxsize=None)
def fixture():
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files}


def params(g, key):
    return json.loads(str(g[key]))


def gray(clip, coeffs):
    cr, cg, cb, bias = coeffs
    c = clip.astype(np.int64)
    y = (cr * c[..., 0] + cg * c[..., 1] + cb * c[..., 2] + bias) >> 16
    assert y.min() >= 0 and y.max() <= 255
    return y.astype(np.uint8)


def frame_normalize(frame_y, tht_black, tht_white):
    """vsutils.frame_normalize on one gray plane; a flat plane inside the thresholds (NaN there) -> zeros"""
    frame_luma = np.mean(frame_y) / 255.0
    if frame_luma <= tht_black or frame_luma >= tht_white:
        return frame_y
    if np.max(frame_y) == np.min(frame_y):
        return np.zeros_like(frame_y)
    out = np.multiply(255, (frame_y - np.min(frame_y)) / (np.max(frame_y) - np.min(frame_y)))
    return out.clip(0, 255).astype('uint8')


def scene_stats_np(clip, offset=1, normalize=False, coeffs=SD.LUMA_LIMITED, tht_black=SD.DEF_THT_BLACK_MIN, tht_white=SD.DEF_THT_WHITE_MIN):
    """-> dict of int64 arrays sum_y, sad, sum_raw, min_y, max_y (one entry per frame)"""
    y = gray(clip, coeffs)
    n = y.shape[0]
    planes = [frame_normalize(f, tht_black, tht_white) for f in y] if normalize else list(y)
    out = {k: np.zeros(n, np.int64) for k in ("sum_y", "sad", "sum_raw", "min_y", "max_y")}
    for i in range(n):
        p = max(i - offset, 0)
        out["sum_y"][i] = planes[i].astype(np.int64).sum()
        out["sad"][i] = np.abs(planes[i].astype(np.int64) - planes[p].astype(np.int64)).sum()
        out["sum_raw"][i] = y[i].astype(np.int64).sum()
        out["min_y"][i], out["max_y"][i] = y[i].min(), y[i].max()
    return out


def noise_clip(seed, n, h, w):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def normalize_clip(seed, h, w):
    """5 frames for normalize=True: below the black threshold, above the white one, flat inside, two ordinary ones (LUMA_LIMITED / LUMA_FULL alike)"""
    r = np.random.default_rng(seed)
    c = np.empty((5, h, w, 3), np.uint8)
    c[0] = r.integers(0, 24, (h, w, 3))
    c[1] = r.integers(225, 256, (h, w, 3))
    c[2] = 120
    c[3] = r.integers(40, 200, (h, w, 3))
    c[4] = np.clip(c[3].astype(np.int64) + r.integers(-30, 31, (h, w, 3)), 60, 170)
    return c


def detect_clip(seed=7, n=24, h=96, w=160):
    """24 frames: scenes with seeded noise of their own around different levels -- cuts at 5, 11 and 19 --, a black stretch (frames 8..10) and a slow fade
    (frames 13..18).  Differences sit far from the thresholds: a cut moves the mean gray by tens of levels, noise inside a scene by a few."""
    r = np.random.default_rng(seed)
    level = np.empty(n)
    level[0:5], level[5:8], level[8:11], level[11:13], level[19:] = 70, 150, 4, 110, 60
    level[13:19] = 110 + 4 * np.arange(1, 7)
    scene_of = np.searchsorted([5, 8, 11, 19], np.arange(n), side="right")
    textures = [r.integers(-25, 26, (h, w, 3)) for _ in range(5)]
    clip = np.empty((n, h, w, 3), np.uint8)
    for i in range(n):
        clip[i] = np.clip(level[i] + textures[scene_of[i]] + r.integers(-2, 3, (h, w, 3)), 0, 255)
    return clip
