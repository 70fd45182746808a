"""Shared by tests/test_tiles_host.py and tests/test_gpu_tiles.py: tests/golden/tiles.npz (the reference's vs_slice_into_2x2_overlapping_tiles /
vs_slice_into_2_horizontal_tiles, executed by tools/gen_golden_tiles.py) and a numpy restatement of HAVC_clip_slice / HAVC_clip_reconstruct
(vsdeoldify/__init__.py:2886-2945, vsslib/vstiles4.py) that follows the reference step by step -- pad, crop; pad both operands to the blended size, build
the position mask, merge, crop -- on clips [n, h, w, 3].  std.MaskedMerge is VapourSynth native code: its stand-in is (a * (255 - m) + b * m + 127) // 255."""
import json
import os

import numpy as np

from tests.conftest import GOLDEN


def fixture():
    """-> (npz, cases); a case = dict(input, slices, overlap_x, overlap_y, numbers = [base_tile_w, base_tile_h, overlap_x, overlap_y] of the reference)"""
    g = np.load(os.path.join(GOLDEN, "tiles.npz"))
    return g, [json.loads(str(c)) for c in g["cases"]]


def fixture_tiles(g, k, n_tiles):
    """the reference's tiles of case k as clips [n, th, tw, 3] (the file holds them planar)"""
    return [np.ascontiguousarray(np.moveaxis(g[f"tile_{k}_{t}"], 1, -1)) for t in range(n_tiles)]


def clip(seed, n, h, w):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def slice_np(clip, slices=2, overlap_x=32, overlap_y=32):
    """-> (tiles, base_tile_w, base_tile_h, overlap_x, overlap_y), vstiles4.py:72-105 / :132-156"""
    n, h, w, _ = clip.shape
    base_w = (w + 1) // 2
    overlap_x = (overlap_x // 2) * 2
    if slices == 4:
        base_h, overlap_y = (h + 1) // 2, (overlap_y // 2) * 2
    else:
        base_h, overlap_y = h, 0
    # std.AddBorders(right, bottom): black.  An odd size with overlap 0 is the one case where the right / bottom crop ends a pixel beyond that border:
    # VapourSynth refuses it (no fixture case), the library treats that pixel as border as well.
    full_h = 2 * base_h if slices == 4 else h
    padded = np.zeros((n, max(h + overlap_y, full_h), max(w + overlap_x, 2 * base_w), 3), np.uint8)
    padded[:, :h, :w] = clip

    def crop(left, top):                                                                         # std.CropAbs
        t = padded[:, top:top + base_h + overlap_y, left:left + base_w + overlap_x]
        assert t.shape[1:3] == (base_h + overlap_y, base_w + overlap_x)
        return np.ascontiguousarray(t)
    tiles = [crop(0, 0), crop(base_w - overlap_x, 0)]
    if slices == 4:
        tiles += [crop(0, base_h - overlap_y), crop(base_w - overlap_x, base_h - overlap_y)]
    return tiles, base_w, base_h, overlap_x, overlap_y


def blend_mask(size, overlap, base, weight):
    """_make_horizontal_blend_mask_akarin / _make_vertical_blend_mask_akarin (vstiles4.py:281-312) as a vector of `size` mask values"""
    mask_val = int(round(weight * 255))
    x = np.arange(size)
    start, end = base - overlap, base + overlap
    if mask_val == 0:                                                                            # "X start1 < 0 X end1 > 255 X start - 255 * overlap / ? ?"
        ramp = np.minimum(255, np.floor((x - start) * 255 / overlap + 0.5))
        m = np.where(x < start + 1, 0, np.where(x > end - 1, 255, ramp))
    else:                                                                                        # "X end >= 255 X start < 0 mask_val ? ?"
        m = np.where(x >= end, 255, np.where(x < start, 0, mask_val))
    return m.astype(np.int64)


def masked_merge(a, b, m):
    """the stand-in of std.MaskedMerge: m broadcasts against [n, h, w, 3]"""
    return ((a.astype(np.int64) * (255 - m) + b.astype(np.int64) * m + 127) // 255).astype(np.uint8)


def _blend(first, second, overlap, base, weight, axis):
    """_blend_horizontal (axis 2) / _blend_vertical (axis 1), vstiles4.py:315-349"""
    if overlap <= 0:
        return np.concatenate([first, second], axis)
    size = base * 2

    def padded(t, after):                                                                        # std.AddBorders up to `size` along the axis
        pad = [(0, 0)] * 4
        pad[axis] = (0, size - t.shape[axis]) if after else (size - t.shape[axis], 0)
        return np.pad(t, pad)
    m = blend_mask(size, overlap, base, weight)
    m = m[None, None, :, None] if axis == 2 else m[None, :, None, None]
    return masked_merge(padded(first, True), padded(second, False), m)


def luma_of(color, orig):
    """the library's stand-in of vsresize.resize_to_chroma: chroma_post_process per frame (oracle.pipeline, pinned to the reference by test_oracle_golden)"""
    from oracle import pipeline
    return np.stack([pipeline.chroma_post_process(c, o) for c, o in zip(color, orig)])


def reconstruct_np(tiles, clip_orig, base_w, base_h, overlap_x, overlap_y, blend_weight=0.5, chroma_resize=False):
    """vstiles4.py:161-278 on clips [n, h, w, 3]; clip_orig None: no crop"""
    full = _blend(tiles[0], tiles[1], overlap_x, base_w, blend_weight, 2)
    if len(tiles) == 4:
        bottom = _blend(tiles[2], tiles[3], overlap_x, base_w, blend_weight, 2)
        full = _blend(full, bottom, overlap_y, base_h, blend_weight, 1)
    if clip_orig is not None:
        full = np.ascontiguousarray(full[:, :clip_orig.shape[1], :clip_orig.shape[2]])           # std.CropAbs(width, height)
    return luma_of(full, clip_orig) if chroma_resize else full
