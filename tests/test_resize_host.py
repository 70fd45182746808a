"""CPU (-m "not gpu"): the host side of the Spline64 resize -- the float64 reference of tests/resize_util.py against the fp32 twin (oracle/resample.py),
the tap counts and the choice of the horizontal kernel (havc_resize_plan), and the LDS span invariant of resize_h_rows_kernel (csrc/colorfilters.hip)."""
import numpy as np
import pytest

from oracle import resample
from tests import resize_util as RU
from vsdeoldify_amd import _native as nat


@pytest.fixture(scope="module")
def lib():
    return nat.load()


def small_clip(seed, n, sh, sw):
    r = np.random.default_rng(seed)
    clip = r.integers(0, 256, (n, sh, sw, 3), dtype=np.uint8)
    clip[0] = r.integers(0, 2, clip[0].shape, dtype=np.uint8) * 255          # hard 0 / 255 edges: overshoot beyond both ends of the byte range
    return clip


# (n, sh, sw) -> (dw, dh): beyond 48 taps, same size, up-sampling with a ragged second tile, 32 and 29 taps, a long source row
SMALL = [((3, 50, 600), (96, 31)), ((1, 61, 83), (83, 61)), ((2, 37, 96), (260, 50)), ((2, 45, 93), (24, 20)), ((2, 33, 42), (12, 40)),
         ((2, 9, 1306), (256, 12)), ((2, 30, 40), (130, 77))]          # (the last one up-samples both axes: its 0 / 255 frame saturates)


@pytest.mark.parametrize("case", range(len(SMALL)))
def test_ref64_agrees_with_the_fp32_twin(case):
    """rounded, the float64 reference is the oracle's uint8 result outside near-ties, and the twin's unrounded fp32 value lies within eps of it: the bound
    the GPU tests rely on holds for the restatement of the kernels' own order of operations"""
    (n, sh, sw), (dw, dh) = SMALL[case]
    clip = small_clip(case, n, sh, sw)
    ref = RU.ref64(clip, dw, dh)
    tie = RU.assert_near_tie_share(ref, f"small {SMALL[case]}")
    assert (ref.n_h, ref.n_v) == (resample.taps(sw, dw)[1].shape[1], resample.taps(sh, dh)[1].shape[1])
    twin = np.stack([resample.resize_rgb8_float(f, dw, dh) for f in clip])
    err = float(np.abs(twin.astype(np.float64) - ref.v).max())
    print(f"max |fp32 - fp64| {err:.3e}, eps {ref.eps:.3e}, ratio {ref.eps / max(err, 1e-30):.1f}")
    assert err <= ref.eps, (err, ref.eps)
    want = np.stack([resample.resize_rgb8(f, dw, dh) for f in clip])
    assert np.array_equal(RU.rounded(ref)[~tie], want[~tie])
    if dw > sw and dh > sh:                                    # (a strong down-sampling averages the 0 / 255 noise back into range)
        assert ref.v[0].max() > 255.5 and ref.v[0].min() < -0.5, "frame 0 must overshoot the byte range on both sides"
    if (sw, sh) == (dw, dh):
        assert np.array_equal(RU.rounded(ref), clip) and not tie.any()


def test_resize_plan_tap_counts_match_the_oracle(lib):
    for sw in list(range(1, 140)) + [255, 256, 257, 384, 511, 512, 560, 600, 1080, 1306, 1326, 1400, 1920, 3840, 4096]:
        for dw in (1, 2, 3, 12, 24, 96, 130, 256, 260, 384, 512, 560, 1080, 1920, 3840):
            assert RU.plan(lib, sw, dw, 1080)[0] == resample.taps(sw, dw)[1].shape[1], (sw, dw)


def test_resize_plan_rejects_bad_arguments(lib):
    import ctypes
    t, v = ctypes.c_int(), ctypes.c_int()
    for sw, dw, rows in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4)):
        assert lib.havc_resize_plan(sw, dw, rows, ctypes.byref(t), ctypes.byref(v)) == nat.HAVC_E_INVALID
    assert lib.havc_resize_plan(1920, 560, 1080, None, None) > 0          # both outputs are optional


def test_resize_plan_variants_of_the_benchmark_passes(lib):
    """what the comments of launch_resize_passes claim for 64 frames of 1080p: 29 / 32 / 48 on the way down, 9 on every way up; one frame keeps the
    one-block-per-row kernel"""
    for dw, taps, variant in ((560, 29, 29), (512, 31, 32), (384, 41, 48)):
        assert RU.plan(lib, 1920, dw, 64 * 1080)[:2] == (taps, variant), dw
        assert RU.plan(lib, dw, 1920, 64 * dw)[:2] == (9, 9), dw
        assert RU.plan(lib, 1080, dw, 64 * 1080)[0] == resample.taps(1080, dw)[1].shape[1]
    assert RU.plan(lib, 384, 1920, 64 * 216)[:2] == (9, 9)
    assert RU.plan(lib, 1920, 560, 1080)[1] == 0
    assert RU.plan(lib, 560, 1920, 560)[1] == 0


def test_resize_plan_thresholds(lib):
    """the three conditions, each at its edge: 2048 blocks, 48 taps, 4096 staged bytes"""
    assert RU.plan(lib, 40, 130, 32753)[1] == 9 and RU.plan(lib, 40, 130, 32752)[1] == 0          # one tile: 2048 chunks of 16 rows
    assert RU.plan(lib, 96, 260, 16369)[1] == 9 and RU.plan(lib, 96, 260, 16368)[1] == 0          # two tiles: 1024 chunks
    assert RU.plan(lib, 40, 130, 65535 * 16)[1] == 9 and RU.plan(lib, 40, 130, 65535 * 16 + 1)[1] == 0      # the grid's y limit
    big = 65535 * 16
    assert RU.plan(lib, 600, 96, big)[:2] == (51, 0)                                              # beyond 48 taps
    assert RU.plan(lib, 1326, 260, big) == (42, 48, 4048)
    sw = next(s for s in range(1326, 1500) if RU.plan(lib, s, 260, big)[2] > 4096)
    assert RU.plan(lib, sw, 260, big)[1] == 0 and RU.plan(lib, sw - 1, 260, big)[1] == 48 and RU.plan(lib, sw - 1, 260, big)[2] == 4096


def tile_spans(sw, dw, taps):
    """lo, hi of every 256-column tile as resize_h_rows_kernel computes them, from the start table of get_resize_table; sw: int64 [m], taps: int64 [m]"""
    scale = dw / sw.astype(np.float64)
    support = 4.0 / np.minimum(scale, 1.0)
    x0 = np.arange(0, dw, 256)
    xl = np.minimum(x0 + 255, dw - 1)

    def start(i):
        center = (i[None, :] + 0.5) / scale[:, None] - 0.5
        return np.floor(center - support[:, None]).astype(np.int64) + 1
    lo = np.clip(start(x0), 0, sw[:, None] - 1)
    hi = np.clip(start(xl) + taps[:, None] - 1, 0, sw[:, None] - 1)
    return lo, hi


def test_tile_spans_restate_the_oracle_start_table():
    for sw, dw in ((40, 130), (96, 260), (520, 260), (1326, 260), (1920, 560), (93, 24), (7, 600)):
        pos, w = resample.taps(sw, dw)
        n = w.shape[1]
        lo, hi = tile_spans(np.array([sw]), dw, np.array([n]))
        x0 = np.arange(0, dw, 256)
        xl = np.minimum(x0 + 255, dw - 1)
        assert np.array_equal(lo[0], pos[x0, 0]) and np.array_equal(hi[0], pos[xl, n - 1]), (sw, dw)
        assert (np.diff(pos[:, 0]) >= 0).all(), "start[] ascends with x: the span of a tile is start[first] .. start[last] + taps - 1"
        # ceil(2 * support) + 1 taps from floor(centre - support) + 1 on: the last one always lies beyond centre + support and weighs exactly 0, so the
        # last pixel of a tile's span is staged but never contributes (hi one shorter gives the same bytes; two shorter does not)
        assert (w[:, -1] == 0).all() and (w[:, -2] != 0).any()


def test_staged_span_never_exceeds_what_the_launcher_reserves(lib):
    """resize_h_rows_kernel prefetches a tile's source span into four dwords per thread (1024 dwords) and writes it to LDS under `if (i * 4 < out_off)`, where
    out_off is the launcher's estimate of the span.  Were the real span (from the start table) ever longer than the estimate, the guard would drop staged
    bytes without a fault.  For every dw of the sweep and every sw that selects the batched kernel: the real span of every tile fits both."""
    big = 65535 * 16                                           # rows: enough chunks for any tile count, so the variant depends on the span and the taps alone
    checked = 0
    for dw in sorted(set(range(4, 601, 7)) | {256, 257, 512, 1920}):
        sws, tapl, staged = [], [], []
        sw = 1
        while True:
            t, variant, lds = RU.plan(lib, sw, dw, big)
            if variant == 0:
                break
            assert t <= variant <= 48 and lds <= 4096, (sw, dw, t, variant, lds)
            sws.append(sw); tapl.append(t); staged.append(lds)
            sw += 1
        assert sw > dw, (dw, sw)                               # every up-sampling and same-size pass of this width is covered
        sws, tapl, staged = np.array(sws), np.array(tapl), np.array(staged)
        lo, hi = tile_spans(sws, dw, tapl)
        span_bytes = (hi - lo + 1) * 3
        assert (span_bytes > 0).all()
        nwords = (3 + span_bytes + 3) >> 2                     # worst misalignment of the span's first byte: a0 = 3
        worst = np.unravel_index(np.argmax(span_bytes + 3 - staged[:, None]), span_bytes.shape)
        assert (nwords <= 1024).all(), (dw, int(sws[np.argmax(nwords.max(1))]))
        assert (span_bytes + 3 <= staged[:, None]).all(), (dw, int(sws[worst[0]]), int(span_bytes[worst]), int(staged[worst[0]]))
        # the last pixel's two-dword read (v_alignbyte) stays inside the staged bytes as well
        assert ((((3 + span_bytes - 3) & ~3) + 8) <= staged[:, None]).all(), dw
        checked += len(sws)
    print(f"{checked} (sw, dw) pairs")
    assert checked > 50000
