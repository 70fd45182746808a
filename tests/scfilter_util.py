"""numpy restatements for the scene filter (csrc/scfilter.hip, vsdeoldify_amd/scdetect.py) and the clips its tests share.

skimage.metrics.structural_similarity(a, b, full=False) on uint8 planes with its defaults -- win_size 7, uniform window, data_range 255 (from the dtype),
K1 0.01, K2 0.03, sample covariance -- is a closed formula over 7 x 7 window sums, and for uint8 planes those sums are exact integers:
    `ssim_np`     from the integer window sums, the variances formed as (49 Sxx - Sx^2) / (49 * 48): the form the kernel is tested against
    `ssim_scipy`  skimage's own sequence (published source of skimage/metrics/_structural_similarity.py): scipy.ndimage.uniform_filter on float64 planes,
                  cov_norm * (E[x^2] - E[x]^2), crop by (win_size - 1) // 2, mean in float64
cv2's gray and histogram: `gray` ((4899 R + 9617 G + 1868 B + 8192) >> 14, oracle/cvcolor.py) and np.bincount."""
import functools
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scfilter.npz")
WIN, NP_WIN = 7, 49
C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2


@functools.lru_cache(maxsize=None)
def fixture():
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files}


def params(g, key):
    return json.loads(str(g[key]))


def gray(rgb):
    """cv2.cvtColor(rgb, COLOR_RGB2GRAY) == cv2.cvtColor(rgb, COLOR_RGB2YUV)[..., 0] for uint8 input"""
    c = np.asarray(rgb).astype(np.int64)
    y = (4899 * c[..., 0] + 9617 * c[..., 1] + 1868 * c[..., 2] + 8192) >> 14
    assert y.min() >= 0 and y.max() <= 255
    return y.astype(np.uint8)


def hist(plane):
    """cv2.calcHist([plane], [0], None, [256], [0, 256]) as integers"""
    return np.bincount(np.asarray(plane, np.uint8).ravel(), minlength=256).astype(np.int64)


def window_sums(a):
    """sums over every 7 x 7 window inside the plane, int64 [h - 6, w - 6]"""
    s = np.zeros((a.shape[0] + 1, a.shape[1] + 1), np.int64)
    s[1:, 1:] = np.cumsum(np.cumsum(a.astype(np.int64), 0), 1)
    return s[WIN:, WIN:] - s[:-WIN, WIN:] - s[WIN:, :-WIN] + s[:-WIN, :-WIN]


def ssim_map_np(a, b):
    a, b = np.asarray(a, np.uint8).astype(np.int64), np.asarray(b, np.uint8).astype(np.int64)
    assert a.shape == b.shape and min(a.shape) >= WIN
    sx, sy, sxx, syy, sxy = window_sums(a), window_sums(b), window_sums(a * a), window_sums(b * b), window_sums(a * b)
    ux, uy = sx / 49.0, sy / 49.0
    vx = (NP_WIN * sxx - sx * sx) / float(NP_WIN * (NP_WIN - 1))
    vy = (NP_WIN * syy - sy * sy) / float(NP_WIN * (NP_WIN - 1))
    vxy = (NP_WIN * sxy - sx * sy) / float(NP_WIN * (NP_WIN - 1))
    return ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))


def ssim_np(a, b):
    """structural_similarity(a, b, full=False) of two uint8 planes -> float64"""
    return np.float64(ssim_map_np(a, b).mean(dtype=np.float64))


def ssim_scipy(a, b):
    from scipy.ndimage import uniform_filter
    x, y = np.asarray(a, np.uint8).astype(np.float64), np.asarray(b, np.uint8).astype(np.float64)
    cov_norm = NP_WIN / (NP_WIN - 1)
    ux, uy = uniform_filter(x, size=WIN), uniform_filter(y, size=WIN)
    uxx, uyy, uxy = uniform_filter(x * x, size=WIN), uniform_filter(y * y, size=WIN), uniform_filter(x * y, size=WIN)
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    s = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
    pad = (WIN - 1) // 2
    return np.float64(s[pad:s.shape[0] - pad, pad:s.shape[1] - pad].mean(dtype=np.float64))


# ---- kernel test clips: frames of one size whose pairs cover the contents the kernels can go wrong on ----
TILE = 32                                                   # SCF_SSIM_TILE (csrc/kernels.h): window positions per block and direction
SHAPES = [(7, 7), (8, 13), (9, 70), (37, 65), (TILE + 6 - 1, TILE + 6 - 1), (TILE + 6, TILE + 6), (TILE + 6 + 1, TILE + 6 + 1), (TILE + 6 - 1, TILE + 6 + 1),
          (2 * TILE + 6 + 1, TILE + 6 - 1)]


def kernel_clip(h, w, seed=0):
    """-> (clip u8 [9, h, w, 3], pairs): random / random, identical, +-20 perturbed, two constants (zero variance: only C2 is left in the denominator), a
    constant against noise, a step edge on the border of the first tile (column / row TILE + 3 is where the windows of the second tile begin to see it)
    against its shifted self, and two frames far apart"""
    r = np.random.default_rng(seed + 1000 * h + w)
    c = np.empty((9, h, w, 3), np.uint8)
    c[0] = r.integers(0, 256, (h, w, 3))
    c[1] = r.integers(0, 256, (h, w, 3))
    c[2] = np.clip(c[0].astype(np.int64) + r.integers(-20, 21, (h, w, 3)), 0, 255)
    c[3], c[4] = 37, 201
    edge = min(TILE + 3, w // 2)
    c[5] = 30
    c[5][:, edge:] = 220
    c[6] = 30
    c[6][:, min(edge + 1, w - 1):] = 220
    edge = min(TILE + 3, h // 2)
    c[7] = (10, 200, 90)
    c[7][edge:] = (250, 40, 180)
    c[8] = r.integers(100, 140, (h, w, 3))
    pairs = [(0, 1), (0, 0), (2, 0), (3, 4), (4, 4), (3, 1), (5, 6), (7, 5), (8, 0), (7, 7)]
    return c, pairs


def detect_filtered_np(clip, threshold=0.10, frequency=0, sc_tht_filter=0.0, min_length=1, tht_white=0.70, tht_black=0.10, frame_norm=False, tht_offset=1):
    """scdetect.scene_detect_filtered without the GPU, for a clip that needs no resize: the statistics from tests/scdetect_util.py, the scores from ssim_np /
    hist -> (SceneInfo, debug); debug["raw"][t_n] = the unrounded (ssim, 1 - hellinger distance) of every score the walk took, debug["asked"] the pairs"""
    from tests import scdetect_util as SU
    from vsdeoldify_amd import scdetect as SD
    n, h, w, _ = clip.shape
    assert SD.resize_min_hw(w, h) == (w, h) and SD.filter_active(sc_tht_filter, min_length)
    t_offset, m_length = min(max(tht_offset, 1), 25), min(max(min_length, 1), 25)
    custom = sc_tht_filter > 0.0 or threshold < 0.10 or t_offset > 1
    st = SU.scene_stats_np(clip, t_offset if custom else 1, frame_norm)
    if custom:
        prev, nxt, luma, ratio = SD.custom_detector(st["sum_y"], st["sad"], h * w, threshold, frequency, 1, tht_white, tht_black)
    else:
        p, q = SD.plugin_flags(st["sad"], h * w, threshold)
        prev, nxt, luma = SD.filter_black_white(p, q, st["sum_y"], h * w, frequency, tht_white, tht_black)
        ratio = np.zeros(n)
    g = gray(clip)
    debug = {"raw": {}, "asked": [], "stage1": np.flatnonzero(prev).tolist()}

    def scores(t_n, last):
        s, d = ssim_np(g[t_n], g[last]), SD.hellinger_distance(hist(g[last]), hist(g[t_n]))
        debug["raw"][t_n] = (float(s), 1.0 - d)
        debug["asked"].append((t_n, last))
        return s, d

    prev, nxt = SD.scene_filter(prev, nxt, luma, ratio, scores, sc_tht_filter, m_length, tht_white, tht_black, frequency, debug=debug)
    return SD.SceneInfo(prev, nxt, luma, ratio, threshold, frequency), debug


def filter_clip(n=24, h=48, w=64, seed=11):
    """the end-to-end clip, 24 frames of 64 x 48: scenes of seeded texture (the frames of a scene are the scene's texture shifted sideways by a pixel or two,
    plus a little noise), flat fields, a dark stretch.  Scene starts: 0, 4 (new texture), 7 (the texture of scene 0 again, brighter), 10 (flat gray), 12 (flat,
    lighter), 14 (dark), 17 (new texture), 20 (the texture of 17, shifted by half a frame), 22 (new texture)."""
    r = np.random.default_rng(seed)
    tex = [np.kron(r.integers(-60, 61, (h // 4, w // 4 + 4, 1)), np.ones((4, 4, 1), np.int64)).repeat(3, 2) + r.integers(-8, 9, (1, 1, 3)) for _ in range(4)]
    starts = [0, 4, 7, 10, 12, 14, 17, 20, 22]
    scene = np.searchsorted(starts, np.arange(n), side="right") - 1
    spec = [(0, 95, 0), (1, 120, 0), (0, 135, 0), (None, 128, 0), (None, 150, 0), (2, 22, 0), (2, 110, 0), (2, 110, 8), (3, 90, 0)]      # texture, level, shift
    clip = np.empty((n, h, w, 3), np.uint8)
    for i in range(n):
        t, level, shift = spec[scene[i]]
        k = i - starts[scene[i]]
        if t is None:
            f = np.full((h, w, 3), float(level)) + r.integers(-1, 2, (h, w, 3))
        else:
            amp = 0.25 if level < 40 else 1.0
            f = level + amp * tex[t][:, shift + k:shift + k + w] + r.integers(-2, 3, (h, w, 3))
        clip[i] = np.clip(f, 0, 255)
    return clip
