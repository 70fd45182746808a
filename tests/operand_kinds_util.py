"""The C entry points with a result of the OTHER kind than the input, and with several operands of mixed kinds in one scratch slot.  The Python wrappers
allocate a result where the input is, so these combinations are reachable only at the ctypes level: a wrapper runs once on host operands behind a recorder
that keeps the native call (the parameter struct included), and the call is replayed through ctx.lib with some operands moved to havc_dev_alloc memory.

`calls(ctx)` yields (label, outputs, launches) for every combination; tests/test_gpu_boundary.py compares them, and they are plain data so that a script can
list them for two builds of the library."""
import ctypes as C

import numpy as np

from vsdeoldify_amd import _native as nat


class _Recorder:
    """stands in for ctx.lib while a wrapper runs: forwards everything, keeps the arguments of the last call of `name`"""

    def __init__(self, lib, name):
        self._lib, self._name, self.args = lib, name, None

    def __getattr__(self, key):
        fn = getattr(self._lib, key)
        if key != self._name:
            return fn

        def call(*args):
            self.args = args
            return fn(*args)
        return call


def record(ctx, name, wrapper):
    """-> the arguments of the ctx.lib.<name> call that `wrapper()` makes"""
    lib = ctx.lib
    ctx.lib = rec = _Recorder(lib, name)
    try:
        wrapper()
    finally:
        ctx.lib = lib
    assert rec.args is not None, name
    return list(rec.args)


def replay(ctx, name, args, ins, outs, kinds):
    """One native call.  ins: {where: ndarray}, outs: {where: (shape, dtype)}; `where` is an argument index, or (argument index, k) for entry k of an array
    of pointers.  kinds: {where: "h" | "d"}.  -> ([result arrays in the order of outs], launches of the call)"""
    args, dev, host_out, tables = list(args), {}, {}, {}

    def put(where, ptr):
        if isinstance(where, tuple):
            if where[0] not in tables:
                tables[where[0]] = args[where[0]] = (C.c_void_p * len(args[where[0]]))(*args[where[0]])      # a copy: the recorded table stays as it was
            tables[where[0]][where[1]] = ptr.value
        else:
            args[where] = ptr
    try:
        for where, a in ins.items():
            a = np.ascontiguousarray(a)
            if kinds[where] == "d":
                dev[where] = ctx.dev_alloc(a.nbytes)
                ctx.dev_upload(dev[where], a)
                put(where, dev[where])
            else:
                put(where, nat.as_ptr(a))
        for where, (shape, dtype) in outs.items():
            host_out[where] = np.zeros(shape, dtype)
            if kinds[where] == "d":
                dev[where] = ctx.dev_alloc(host_out[where].nbytes)
                put(where, dev[where])
            else:
                put(where, nat.as_ptr(host_out[where]))
        before = ctx.stats().launches
        nat.check(getattr(ctx.lib, name)(*args), ctx.h)
        launches = ctx.stats().launches - before
        for where in outs:
            if kinds[where] == "d":
                ctx.dev_download(host_out[where], dev[where])                  # (synchronises: a call with device results has only enqueued)
        return [host_out[w] for w in outs], launches
    finally:
        for p in dev.values():
            ctx.dev_free(p)


def make_clip(seed=0):
    """3 frames of 16 x 24 (h x w): even, at least the equaliser's 8 x 8 grid and SSIM's 7 x 7 window -- the smallest every entry accepts"""
    return np.random.default_rng(seed).integers(0, 256, (3, 16, 24, 3), dtype=np.uint8)


def calls(ctx):
    from vsdeoldify_amd import chroma_stab, equalize, havc, mcomb, retinex, scdetect_edge, tweak
    clip, other = make_clip(0), make_clip(1)
    n, h, w, _ = clip.shape
    like = (clip.shape, np.uint8)
    # ---- one input (two for recover), one result: all host, host -> device, device -> host ----
    single = [
        ("havc_equalize_clip", lambda: equalize.rgb_equalizer_np(ctx, clip, method=2), {1: clip}, {2: like}),
        ("havc_adjust_rgb_clip", lambda: tweak.adjust_rgb_np(ctx, clip, 0.5, tweak.adjust_plan((1.1, 0.9, 1.0), (2, 0, -3), (1.2, 1.0, 0.8))), {1: clip}, {2: like}),
        ("havc_tweak_clip", lambda: tweak.tweak_np(ctx, clip, tweak.tweak_plan(hue=20, sat=1.3, bright=4, cont=1.1, gamma=1.2)), {1: clip}, {2: like}),
        ("havc_reduce_flicker_clip", lambda: chroma_stab.reduce_flicker_np(ctx, clip), {1: clip}, {2: like}),
        ("havc_recover_color_clip", lambda: mcomb.recover_color_clip(ctx, clip, other), {1: clip, 2: other}, {3: like}),
        ("havc_retinex_clip", lambda: retinex.retinex_np(ctx, clip, sigma=(1, 2)), {1: clip}, {2: like}),
        ("havc_spline64_resize_n", lambda: havc.spline64(ctx, clip, 12, 8), {1: clip}, {4: ((n, 8, 12, 3), np.uint8)}),
    ]
    for name, wrapper, ins, outs in single:
        args = record(ctx, name, wrapper)
        (out_at,) = outs
        for i_kind, o_kind in (("h", "h"), ("h", "d"), ("d", "h")):
            kinds = {**{k: i_kind for k in ins}, out_at: o_kind}
            yield (name, f"{i_kind}->{o_kind}") + replay(ctx, name, args, ins, outs, kinds)
    # ---- packs: the planes of the two YUV halves, the tiles ----
    y, u, v = tweak.rgb_to_yuv420_np(ctx, clip)
    args = record(ctx, "havc_rgb_to_yuv420", lambda: tweak.rgb_to_yuv420_np(ctx, clip))
    outs = {2: (y.shape, np.uint8), 3: (u.shape, np.uint8), 4: (v.shape, np.uint8)}
    for label, k in (("hhh", "hhh"), ("hdh", "hdh"), ("ddd", "ddd")):
        yield ("havc_rgb_to_yuv420", label) + replay(ctx, "havc_rgb_to_yuv420", args, {1: clip}, outs, {1: "h", 2: k[0], 3: k[1], 4: k[2]})
    args = record(ctx, "havc_yuv420_to_rgb", lambda: tweak.yuv420_to_rgb_np(ctx, y, u, v))
    for label, k in (("hhh", "hhh"), ("dhd", "dhd"), ("ddd", "ddd")):
        yield ("havc_yuv420_to_rgb", label) + replay(ctx, "havc_yuv420_to_rgb", args, {1: y, 2: u, 3: v}, {4: like}, {1: k[0], 2: k[1], 3: k[2], 4: "h"})
    ct = havc.HAVC_clip_slice(clip, 4, 4, 4)
    args = record(ctx, "havc_tile_slice", lambda: havc.HAVC_clip_slice(clip, 4, 4, 4))
    outs = {(2, t): (ct.tiles[t].shape, np.uint8) for t in range(4)}
    for label in ("hhhh", "hdhd", "dhdh"):
        yield ("havc_tile_slice", label) + replay(ctx, "havc_tile_slice", args, {1: clip}, outs, {1: "h", **{(2, t): label[t] for t in range(4)}})
    args = record(ctx, "havc_tile_reconstruct", lambda: havc.HAVC_clip_reconstruct(ct, 0.3, True))
    ins = {**{(1, t): ct.tiles[t] for t in range(4)}, 2: clip}
    for label in ("hhhh", "hdhd", "dhdh"):                                    # clip_orig on the host throughout, the result on the host: two slots staged
        yield ("havc_tile_reconstruct", label) + replay(ctx, "havc_tile_reconstruct", args, ins, {3: like}, {**{(1, t): label[t] for t in range(4)}, 2: "h", 3: "h"})
    # ---- two host results of one call: the records and the mask tap ----
    rec_dtype = nat.EDGE_REC_DTYPE
    args = record(ctx, "havc_scene_edge_stats", lambda: scdetect_edge.edge_stats(ctx, clip, mask_tap=True))
    outs = {3: ((n,), rec_dtype), 4: ((n, h, w), np.uint8)}
    for label, src in (("tap", "h"), ("tap, device clip", "d")):
        yield ("havc_scene_edge_stats", label) + replay(ctx, "havc_scene_edge_stats", args, {1: clip}, outs, {1: src, 3: "h", 4: "h"})
    args[4] = None
    yield ("havc_scene_edge_stats", "no tap") + replay(ctx, "havc_scene_edge_stats", args, {1: clip}, {3: ((n,), rec_dtype)}, {1: "h", 3: "h"})
