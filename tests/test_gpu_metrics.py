"""-m gpu: clip_delta_e (csrc/metrics.hip) against the float64 oracle oracle/imaging.py delta_e00_images, pixel by pixel at tests/metrics_util.py LIMIT
(1e-9; the reasons are written there), and its per-frame records against the kernel's own map, exactly."""
import ctypes as C

import numpy as np
import pytest

from tests import metrics_util as mu
from vsdeoldify_amd import _native as nat
from vsdeoldify_amd import metrics
from vsdeoldify_amd.device import DeviceImage
from vsdeoldify_amd.vformat import DevicePlane

pytestmark = pytest.mark.gpu


def _run(ctx, a, b, **kw):
    rep = metrics.delta_e_np(ctx, a, b, return_map=True, **kw)
    dmap = rep.map.numpy() if isinstance(rep.map, DevicePlane) else rep.map
    return rep, dmap


# frame sizes (w x h): one pixel, less than a thread's four, one thread's row, odd sizes, a row that is no multiple of four pixels, one block and a bit,
# several blocks with a ragged last one; frame counts 1, 3 and 5 spread over them
SHAPES = [(1, 1, 1), (3, 3, 1), (1, 4, 4), (5, 37, 23), (3, 130, 3), (1, 64, 64), (3, 255, 257)]


@pytest.mark.parametrize("n,w,h", SHAPES)
def test_shapes_against_the_oracle(ctx, n, w, h):
    a, b = mu.random_pair((n, h, w, 3), 100 + w)
    rep, dmap = _run(ctx, a, b)
    assert dmap.shape == (n, h, w) and dmap.dtype == np.float64
    err, share = mu.compare_maps(dmap, a, b)
    print(f"{n} x {w} x {h}: max |GPU - oracle| {err:.3e}, excluded share {share}")
    assert err <= mu.LIMIT
    assert not dmap[np.all(a == b, -1)].any()
    mu.check_records(rep, dmap, a, b)
    want = mu.oracle_map(a, b)
    assert np.all(np.abs(rep.mean - want.reshape(n, -1).mean(axis=1)) <= mu.LIMIT)


def test_single_frame_is_accepted(ctx):
    a, b = mu.random_pair((23, 37, 3), 7)
    rep = metrics.clip_delta_e(a, b, return_map=True)
    assert rep.map.shape == (23, 37) and rep.n_frames == 1
    clip = metrics.clip_delta_e(a[None], b[None], return_map=True)
    assert clip.recs.tobytes() == rep.recs.tobytes() and clip.map.tobytes() == rep.map.tobytes()


@pytest.fixture(scope="module")
def structured(ctx):
    a, b, rows = mu.structured_pair()
    want = mu.oracle_map(a, b)
    rep, dmap = _run(ctx, a, b)
    for x in (a, b, want, dmap):
        x.setflags(write=False)
    return a, b, rows, want, rep, dmap


def test_structured_pairs_reach_every_branch(structured):
    a, b, rows, want, rep, dmap = structured
    counts = mu.branch_counts(a, b)
    assert all(v > 0 for v in counts.values()), counts
    assert counts["achromatic"] >= (rows["black"][1] - rows["black"][0]) * a.shape[1]
    assert int(mu.hue_excluded(a, b).sum()) == 0


def test_structured_pairs_per_pixel(structured):
    a, b, rows, want, rep, dmap = structured
    err, share = mu.compare_maps(dmap, a, b, want)
    print(f"structured 1024 x 1024: max |GPU - oracle| {err:.3e}, excluded share {share}")
    assert share == 0
    assert err <= mu.LIMIT
    for band, (lo, hi) in rows.items():
        print(f"  band {band}: max |GPU - oracle| {np.abs(dmap[lo:hi] - want[lo:hi]).max():.3e}, largest dE {dmap[lo:hi].max():.4f}")


def test_identical_pixels_are_exactly_zero(ctx, structured):
    a, b, rows, want, rep, dmap = structured
    lo, hi = rows["same"]
    assert not dmap[lo:hi].any()
    assert not dmap[np.all(a == b, -1)].any()
    same = metrics.delta_e_np(ctx, a[lo:hi], a[lo:hi].copy(), return_map=True)
    assert same.recs["max"][0] == 0.0 and same.recs["sum"][0] == 0.0 and int(same.recs["hist"][0, 0]) == (hi - lo) * a.shape[1]
    assert not same.recs["sse"].any() and not same.map.any() and same.meets_contract and same.below(1 / 64) == 1.0
    assert same.psnr[0] == np.inf


def test_structured_records_against_the_kernels_own_map(structured):
    a, b, rows, want, rep, dmap = structured
    mu.check_records(rep, dmap, a, b)
    assert int(rep.recs["hist"][0, 1024]) == int((dmap >= 16.0).sum()) > 0
    assert abs(rep.clip_mean - want.mean()) <= mu.LIMIT and abs(rep.clip_max - want.max()) <= mu.LIMIT
    assert rep.below(1.0) == float((dmap < 1.0).mean()) and not rep.meets_contract


def test_two_runs_give_the_same_bytes(ctx, structured):
    a, b, rows, want, rep, dmap = structured
    again, dmap2 = _run(ctx, a, b)
    assert again.recs.tobytes() == rep.recs.tobytes() and dmap2.tobytes() == dmap.tobytes()


def test_operand_kinds_give_the_same_bytes(ctx, monkeypatch):
    a, b = mu.random_pair((3, 130, 67, 3), 11)
    da, db = DeviceImage.from_numpy(ctx, a), DeviceImage.from_numpy(ctx, b)
    base, bmap = _run(ctx, a, b)
    assert isinstance(base.map, np.ndarray)
    for x, y, kind in ((da, db, DevicePlane), (a, db, np.ndarray), (da, b, np.ndarray)):
        rep, dmap = _run(ctx, x, y)
        assert isinstance(rep.map, kind)
        assert rep.recs.tobytes() == base.recs.tobytes() and dmap.tobytes() == bmap.tobytes()
    assert metrics.clip_delta_e(da, db).recs.tobytes() == base.recs.tobytes()            # the public entry finds the context of its operands
    # without return_map there is no map: no buffer from the pool, no scratch that grows, the records alone come back
    made = []
    init = DevicePlane.__init__
    monkeypatch.setattr(DevicePlane, "__init__", lambda self, *k, **kw: (made.append(k), init(self, *k, **kw))[1])
    before = ctx.stats().bytes_resident
    for x, y in ((da, db), (a, b)):
        rep = metrics.delta_e_np(ctx, x, y)
        assert rep.map is None and rep.recs.tobytes() == base.recs.tobytes()
    assert not made and ctx.stats().bytes_resident == before


def test_sentinels_around_records_and_map_stay(ctx):
    """device records and a device map inside larger buffers of 0xA5: the bytes in front of and behind them are as they were"""
    n, h, w, pad = 2, 23, 37, 4096
    a, b = mu.random_pair((n, h, w, 3), 21)
    da, db = DeviceImage.from_numpy(ctx, a), DeviceImage.from_numpy(ctx, b)
    rb, mb = n * nat.DE_REC_DTYPE.itemsize, n * h * w * 8
    fill = {}
    for name, size in (("rec", rb), ("map", mb)):
        host = np.full(size + 2 * pad, 0xA5, np.uint8)
        d = ctx.dev_alloc(host.nbytes)
        ctx.dev_upload(d, host)
        fill[name] = (d, host)
    try:
        metrics._table_once(ctx)
        nat.check(ctx.lib.havc_delta_e_clip(ctx.h, da.ptr, db.ptr, w, h, n, C.c_void_p(fill["rec"][0].value + pad), C.c_void_p(fill["map"][0].value + pad)), ctx.h)
        got = {}
        for name, (d, host) in fill.items():
            out = np.empty_like(host)
            ctx.dev_download(out, d)
            assert (out[:pad] == 0xA5).all() and (out[-pad:] == 0xA5).all(), name
            got[name] = out[pad:-pad]
    finally:
        for d, _ in fill.values():
            ctx.dev_free(d)
    want, wmap = _run(ctx, a, b)
    assert got["rec"].tobytes() == want.recs.tobytes() and got["map"].tobytes() == wmap.tobytes()
    # host records and a host map inside larger arrays
    hrec, hmap = np.full(rb + 2 * pad, 0xA5, np.uint8), np.full(mb + 2 * pad, 0xA5, np.uint8)
    nat.check(ctx.lib.havc_delta_e_clip(ctx.h, nat.as_ptr(a), nat.as_ptr(b), w, h, n, C.c_void_p(hrec.ctypes.data + pad), C.c_void_p(hmap.ctypes.data + pad)), ctx.h)
    for x, ref in ((hrec, want.recs), (hmap, wmap)):
        assert (x[:pad] == 0xA5).all() and (x[-pad:] == 0xA5).all() and x[pad:-pad].tobytes() == ref.tobytes()


def test_partials_beyond_a_small_slot_run_in_two_chunks(ctx, monkeypatch):
    """three frames of 255 x 257 are 64 partial sums each; a context whose slot holds 128 of them takes two frames at a time: two chunks, four launches,
    the same bytes as the one chunk of the session's context"""
    a, b = mu.random_pair((3, 257, 255, 3), 31)
    base, bmap = _run(ctx, a, b)
    monkeypatch.setenv("HAVC_DE_SCRATCH_BYTES", str(128 * 8))
    small = nat.Context(0)
    try:
        # a context that was never given a table builds it with the C library's pow: the same formula, a pixel moves by far less than LIMIT
        recs, dmap = np.zeros(3, nat.DE_REC_DTYPE), np.empty((3, 257, 255))
        nat.check(small.lib.havc_delta_e_clip(small.h, nat.as_ptr(a), nat.as_ptr(b), 255, 257, 3, nat.as_ptr(recs), nat.as_ptr(dmap)), small.h)
        assert np.abs(dmap - bmap).max() <= mu.LIMIT and np.array_equal(recs["sse"], base.recs["sse"])
        for x, y in ((a, b), (DeviceImage.from_numpy(small, a), DeviceImage.from_numpy(small, b))):
            small.synchronize()
            l0 = small.stats().launches
            rep, dmap = _run(small, x, y)
            assert small.stats().launches - l0 == 4
            assert rep.recs.tobytes() == base.recs.tobytes() and dmap.tobytes() == bmap.tobytes()
            del rep
        l0 = ctx.stats().launches
        metrics.delta_e_np(ctx, a, b)
        assert ctx.stats().launches - l0 == 2
        del x, y
    finally:
        small.close()


def test_end_to_end_fast_against_precise(ctx):
    """a seeded DeOldify video model colours an 80 x 80 clip in fast and in precise arithmetic; clip_delta_e of the two outputs equals the oracle's figures
    for the same two outputs.  No threshold is put on the difference itself."""
    from PIL import Image
    from vsdeoldify_amd import render
    from vsdeoldify_amd.synth import synth_state_dict
    sds = {"video": synth_state_dict("wide", 1)}
    r = np.random.default_rng(3)
    frames = []
    for i in range(2):
        yy, xx = np.mgrid[0:80, 0:80]
        luma = np.clip(110 + 60 * np.sin(xx / (5.0 + i)) * np.cos(yy / 7.0) + 12 * r.standard_normal((80, 80)), 0, 255).astype(np.uint8)
        frames.append(np.stack([luma] * 3, -1))
    outs = {}
    for mode in ("fast", "precise"):
        mir = render.ModelImageRender("", "video", render_factor=5, state_dicts=sds, precision=mode)
        outs[mode] = np.stack([np.asarray(mir.get_transformed_image(Image.fromarray(f))) for f in frames])
        assert outs[mode].shape == (2, 80, 80, 3)
    rep = metrics.clip_delta_e(outs["fast"], outs["precise"], return_map=True)
    want = mu.oracle_map(outs["fast"], outs["precise"])
    err, share = mu.compare_maps(rep.map, outs["fast"], outs["precise"], want)
    print(f"fast against precise, 2 x 80 x 80: mean {rep.clip_mean:.4f}, max {rep.clip_max:.4f}, below 1.0 {rep.below(1.0):.5f}; "
          f"max |GPU - oracle| {err:.3e}, excluded share {share}")
    assert err <= mu.LIMIT
    mu.check_records(rep, rep.map, outs["fast"], outs["precise"])
    skip = mu.hue_excluded(outs["fast"], outs["precise"])
    if not skip.any():
        assert np.all(np.abs(rep.mean - want.reshape(2, -1).mean(axis=1)) <= mu.LIMIT) and abs(rep.clip_max - want.max()) <= mu.LIMIT
        assert rep.below(1.0) == float((want < 1.0).mean()) or np.abs(want - 1.0).min() <= mu.LIMIT
        assert rep.meets_contract == bool(want.max() < 1.0) or abs(want.max() - 1.0) <= mu.LIMIT
