"""Shared by tests/test_stabilizer_host.py and tests/test_gpu_stabilizer.py: tests/golden/stabilizer.npz (the reference's HAVC_stabilizer filters, executed
by tools/gen_golden_stabilizer.py) and the chain of the ORACLE's three frame bodies, with HAVC_stabilizer's argument list and unpacking
(vsdeoldify/__init__.py:2806-2860).  Colormap names are translated through the fixture's table, never through the code under test."""
import json
import os

import numpy as np

from oracle import tweaks
from tests.conftest import GOLDEN

MEDIUM = dict(dark=True, dark_p=[0.2, 0.8], smooth=True, smooth_p=[0.3, 0.7, 0.9, 0.0, "none"], colormap="red->brown")     # preset "medium"


def fixture():
    g = np.load(os.path.join(GOLDEN, "stabilizer.npz"))
    cases = [json.loads(str(c)) for c in g["cases"]]
    table = dict(zip((str(n) for n in g["colormap_in"]), (str(o) for o in g["colormap_out"])))
    return g, cases, table


def parsed(table, dark=False, dark_p=(0.2, 0.8), smooth=False, smooth_p=(0.3, 0.7, 0.9, 0.0, "none"), colormap="none"):
    """HAVC_stabilizer's arguments -> (dark, smooth, colormap) as the frame bodies / stabilize_np take them (None = off)"""
    d = (dark_p[0], dark_p[1], (dark_p[2] if len(dark_p) > 2 else "none").lower()) if dark else None
    s = (smooth_p[0], smooth_p[1], smooth_p[2], -smooth_p[3], (smooth_p[4] if len(smooth_p) > 4 else "none").lower()) if smooth else None
    c = table[colormap.lower()] if colormap.lower() not in ("none", "") else None
    return d, s, c


def chain(mod, frame, dark, smooth, colormap, **kw):
    """dark_tweak_frame -> chroma_bright_tweak_frame -> colormap_frame of `mod` (oracle.tweaks, or vsdeoldify_amd.stabilizer: the existing entry points)"""
    x = np.asarray(frame)
    if dark is not None:
        x = mod.dark_tweak_frame(x, *dark, **kw)
    if smooth is not None:
        x = mod.chroma_bright_tweak_frame(x, *smooth, **kw)
    if colormap is not None:
        x = mod.colormap_frame(x, colormap, **kw)
    return np.asarray(x)


def oracle_chain(clip, dark, smooth, colormap):
    clip = np.asarray(clip)
    if clip.ndim == 3:
        return chain(tweaks, clip, dark, smooth, colormap)
    return np.stack([chain(tweaks, f, dark, smooth, colormap) for f in clip])


def colourful(seed, n, h, w):
    """seeded clip with every hue and a dark-to-bright ramp: each luma mask of the filters has pixels on both sides"""
    r = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    out = []
    for i in range(n):
        col = np.stack([128 + 110 * np.sin(xx / (7.0 + i) + yy / 23.0), 128 + 110 * np.cos(yy / (5.0 + i) - xx / 31.0),
                        128 + 110 * np.sin((xx + yy) / 9.0 + 1.0 + i)], -1)
        level = (0.04 + 0.96 * xx / max(w - 1, 1))[..., None] ** 1.5
        out.append(np.clip(col * level + 6 * r.standard_normal((h, w, 3)), 0, 255).astype(np.uint8))
    return np.stack(out)
