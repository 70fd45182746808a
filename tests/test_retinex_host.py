"""CPU (-m "not gpu"): HAVC_retinex.  The reference's Python around the Retinex plugin (vsdeoldify_amd/retinex.py frame_rule / plugin_args, tests/retinex_util.py
around) against the reference EXECUTED by tools/gen_golden_retinex.py (tests/golden/retinex.npz); the library's host entry points (the kernels' C++ compiled
for the host) against the same records; properties of the numpy restatement of the plugin's pixel work (tests/retinex_util.py: the definition); the
signature, the header, the bindings and the refusals; and the two reference-only measurements the GPU test's tolerances rest on."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from tests import retinex_util as U
from vsdeoldify_amd import _native as nat
from vsdeoldify_amd import havc
from vsdeoldify_amd import retinex as RX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "havc_mi355.h")


def test_signature_equals_the_reference():
    def pos(fn):
        return [(k, v.default) for k, v in inspect.signature(fn).parameters.items() if v.kind is v.POSITIONAL_OR_KEYWORD]
    assert pos(havc.HAVC_retinex) == [("clip", inspect.Parameter.empty), ("luma_dark", 0.20), ("luma_bright", 0.80), ("sigmas", (25, 80, 250)),
                                      ("range_tv_in", True), ("range_tv_out", True), ("blend", False), ("chroma_resize", False)]    # __init__.py:1073-1075
    assert (RX.DEF_RETINEX_DARK, RX.DEF_RETINEX_BRIGHT) == (0.20, 0.80)                                                            # constants.py:26-27
    import vsdeoldify_amd
    assert vsdeoldify_amd.HAVC_retinex is havc.HAVC_retinex
    assert "HAVC_retinex" in havc.__doc__ and "UNPINNED" in RX.__doc__ and "PINNED" in RX.__doc__


@pytest.mark.parametrize("sigma", [0.5, 0.9, 2.0, 2.4999, 2.5, 3.0, 25, 80, 250, 10000])
def test_coefficients_equal_the_library_bit_for_bit(sigma):
    py, c = RX.coefficients(sigma), RX.native_coefficients(sigma)
    assert np.array_equal(np.array(py).view(np.uint64), np.array(c).view(np.uint64)), (sigma, py, c)
    assert abs(sum(py) - 1.0) <= 1e-15, (sigma, sum(py) - 1.0)
    with pytest.raises(ValueError):
        RX.native_coefficients(0.49)
    with pytest.raises(ValueError):
        RX.native_coefficients(float("nan"))


def test_a_constant_plane_stays_constant_at_sigma_250():
    g = U.gaussian(np.full((1, 40, 70), 0.4470588235294118), 250)
    assert np.abs(g - 0.4470588235294118).max() <= 1e-9, np.abs(g - 0.4470588235294118).max()


def test_the_fixture_covers_what_it_claims():
    d, cases = U.golden()
    assert len(cases) == 64 and "executing the reference" in str(d["provenance"])
    for i in range(len(cases)):
        assert d[f"case_{i}_in"].shape[0] <= 24 and d[f"case_{i}_in"].shape[1] <= 40
    gated = [c for c in cases if not c["gate"]]
    assert any(c["f_luma"] < c["luma_dark"] for c in gated) and any(c["f_luma"] > c["luma_bright"] for c in gated)
    assert any(c["f_luma"] == c["luma_dark"] and c["gate"] for c in cases) and any(c["f_luma"] == c["luma_bright"] and c["gate"] for c in cases)
    for tv in (True, False):
        sub = [c for c in cases if c["range_tv_in"] is tv]
        assert any(not c["gate"] for c in sub) and any(c["gate"] for c in sub)
        assert any(c["weight"] >= 0 for c in sub) and any(c["gate"] and c["blend"] and c["weight"] < 0 and c["f_luma"] >= 0.40 for c in sub)
    assert any(c["weight"] == 0.25 for c in cases) and any(0.25 < c["weight"] < 0.90 for c in cases)            # the min_w floor, and above it
    assert any(c["gate"] and not c["blend"] and c["f_luma"] < 0.40 for c in cases)                              # blend off below 0.40: the plugin's frame


def test_frame_rule_and_the_library_reproduce_every_record():
    _, cases = U.golden()
    for i, c in enumerate(cases):
        args = (c["sum_y"], c["n_pixels"], c["luma_dark"], c["luma_bright"], c["range_tv_in"], c["blend"])
        want = (c["f_luma"], c["gate"], None if c["weight"] < 0 else c["weight"])
        for what, got in (("frame_rule", RX.frame_rule(*args)), ("havc_retinex_frame_params", RX.frame_params(*args))):
            assert got[0] == want[0] and got[1] is want[1], (i, what, got, want)
            if want[2] is None:
                assert got[2] is None, (i, what, got, want)
            else:                                                    # the weight reaches Pillow as a C float
                assert got[2] is not None and np.float32(got[2]) == np.float32(want[2]), (i, what, got, want)


def test_around_reproduces_every_output_frame():
    d, cases = U.golden()
    for i, c in enumerate(cases):
        got = U.around(d[f"case_{i}_in"], d[f"case_{i}_rtx"], c["luma_dark"], c["luma_bright"], c["range_tv_in"], c["blend"])
        assert np.array_equal(got, d[f"case_{i}_out"]), (i, c)
        if not c["gate"]:
            assert np.array_equal(d[f"case_{i}_out"], d[f"case_{i}_in"])                                       # whatever range_tv_out is


def test_havc_retinex_forwards_what_the_reference_forwards(monkeypatch):
    _, cases = U.golden()
    seen = []

    def record(ctx, clip, *a, **k):
        seen.append((a, k))
        return clip
    real = inspect.signature(RX.retinex_np)
    monkeypatch.setattr(havc, "get_context", lambda i: None)
    monkeypatch.setattr(RX, "retinex_np", record)
    frame = np.zeros((8, 8, 3), np.uint8)
    for c in cases:
        del seen[:]
        havc.HAVC_retinex(frame, c["luma_dark"], c["luma_bright"], c["sigmas"], c["range_tv_in"], c["range_tv_out"], c["blend"])
        (a, k), = seen
        assert a == ()
        plugin = {n: k[n] for n in ("sigma", "lower_thr", "upper_thr", "fulls", "fulld", "chroma_protect")}
        assert real.bind(None, None, **k) and list(real.parameters)[2:8] == list(plugin)                                     # they are retinex_np's plugin arguments
        assert {"sigmas" if n == "sigma" else n: v for n, v in plugin.items()} == \
            {"sigmas" if n == "sigma" else n: v for n, v in c["plugin"].items()}, (c, k)
        assert (k["luma_dark"], k["luma_bright"], k["range_tv"], k["blend"]) == (c["luma_dark"], c["luma_bright"], c["range_tv_in"], c["blend"])


def test_the_clip_is_what_it_was_built_for():
    for h, w in U.SIZES:
        clip = U.make_clip(h, w)
        for tv in (True, False):
            kinds = U.frame_kinds(clip, tv)
            assert kinds[0][0] < 0.20 and not kinds[0][1] and kinds[1][0] > 0.80 and not kinds[1][1], (h, w, tv, kinds)
            assert 0.20 <= kinds[2][0] < 0.40 and kinds[2][1] and kinds[2][2] is not None, (h, w, tv, kinds)
            for k in (3, 5):
                assert kinds[k][0] >= 0.40 and kinds[k][1] and kinds[k][2] is None, (h, w, tv, kinds)
            assert not kinds[4][1] and U.frame_kinds(clip, tv, luma_dark=0.0)[4][1]                            # the constant frame: through the gate at luma_dark = 0
            inten, _, p = U.reference(h, w, (25, 80, 250), tv)
            assert (p > 0).all(), (h, w, tv)                                                                   # the logarithm is defined everywhere
            assert (inten[5] <= 0).any() and (clip[5].max(-1) == 255).any() and np.ptp(clip[4]) == 0
            assert np.ptp(p[4]) == 0 and p[4, 0, 0] == (1.0 if inten[4, 0, 0] == 0 else 8.0)                   # exactly stationary: the mx <= mn path


def test_the_constant_level_is_the_only_stationary_one():
    def stationary(x, sigma):
        B, B1, B2, B3 = RX.coefficients(sigma)
        return ((B * x + B1 * x) + B2 * x) + B3 * x == x
    ok = [v for v in range(1, 256) if all(stationary(x, s) for x in (3 * v * (1.0 / 765), (3 * v - 48) * (1.0 / 657)) for s in (25, 80, 250))]
    assert ok == [U.CONSTANT_LEVEL]


def test_gated_and_constant_frames_come_back_unchanged_and_the_ordinary_one_changed():
    h, w = 33, 257
    clip = U.make_clip(h, w)
    for tv in (True, False):
        rtx = U.reference_bytes(h, w, (25, 80, 250), tv, tv)
        out = U.retinex_ref(clip, range_tv_in=tv, range_tv_out=tv, rtx=rtx)
        for k in (0, 1, 4):
            assert np.array_equal(out[k], clip[k]), (tv, k)
        assert not np.array_equal(out[3], clip[3]) and not np.array_equal(out[2], clip[2])
        open_gate = U.retinex_ref(clip, luma_dark=0.0, range_tv_in=tv, range_tv_out=tv, rtx=rtx)
        assert np.array_equal(open_gate[4], clip[4]) and not np.array_equal(open_gate[0], clip[0])             # through the gate and still unchanged: mx <= mn
    out = U.retinex_ref(clip, range_tv_in=True, range_tv_out=False, rtx=U.reference_bytes(h, w, (25, 80, 250), True, False))
    assert np.array_equal(out[0], clip[0]) and np.array_equal(out[1], clip[1])                                 # gated out: the input, whatever range_tv_out is


def test_an_unclamped_pixel_keeps_its_channel_ratio():
    h, w = 33, 257
    clip = U.make_clip(h, w)
    out = U.reference_bytes(h, w, (25, 80, 250), True, True)[3].astype(np.float64)
    src = clip[3].astype(np.float64)
    inside = (out.max(-1) < 255) & (src.min(-1) > 0)
    assert inside.sum() > h * w // 2
    gain = out[inside] / src[inside]                                                                           # each within 0.5 / c of the pixel's gain
    slack = (0.5 / src[inside]).sum(-1, keepdims=True) + 1e-12
    assert (np.abs(gain - gain.mean(-1, keepdims=True)) <= slack).all()


def test_header_struct_and_bindings():
    src = open(HEADER).read()
    m = re.search(r"typedef struct havc_retinex_params \{(.*?)\} havc_retinex_params;", src, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = [re.sub(r"\[\d+\]", "", n).strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == [f[0] for f in nat.RetinexParams._fields_]
    P = nat.RetinexParams
    assert ctypes.sizeof(P) == 120 and P.sigma.offset == 16 and P.luma_dark.offset == 80 and P.fulls.offset == 96 and P.chunk_frames.offset == 112
    assert "int havc_retinex_clip(havc_ctx* ctx, const uint8_t* src, uint8_t* dst, const havc_retinex_params* params, double* tap);" in src
    assert "int havc_retinex_frame_params(int64_t sum_y, int64_t n_pixels, int range_tv, double luma_dark, double luma_bright, int blend, double* out);" in src
    assert "int havc_retinex_coefficients(double sigma, double* out4);" in src
    assert "UNPINNED" in src[src.index("HAVC_retinex"):src.index("typedef struct havc_retinex_params")]
    assert "identical from run to run" in src[src.index("} havc_retinex_params;"):src.index("int havc_retinex_clip(")]
    sym = {s[0]: s for s in nat.SYMBOLS}
    assert len(sym["havc_retinex_clip"][2]) == 5 and len(sym["havc_retinex_frame_params"][2]) == 7 and len(sym["havc_retinex_coefficients"][2]) == 2
    lib = nat.load()
    out = (ctypes.c_double * 3)()
    assert lib.havc_retinex_frame_params(-1, 10, 1, 0.2, 0.8, 0, out) == nat.HAVC_E_INVALID
    assert lib.havc_retinex_frame_params(10, 0, 1, 0.2, 0.8, 0, out) == nat.HAVC_E_INVALID
    assert lib.havc_retinex_frame_params(10, 10, 1, 0.2, 0.8, 0, None) == nat.HAVC_E_INVALID


def test_refusals_come_before_any_gpu_work(monkeypatch):
    def no_gpu(*a, **k):
        raise AssertionError("GPU work was started")
    monkeypatch.setattr(havc, "get_context", no_gpu)
    monkeypatch.setattr(RX, "retinex_np", no_gpu)
    c = np.zeros((2, 16, 16, 3), np.uint8)
    E = havc.HAVCError
    with pytest.raises(NotImplementedError, match="chroma_resize"):
        havc.HAVC_retinex(c, chroma_resize=True)
    for bad in (None, [[1, 2, 3]]):
        with pytest.raises(E, match="not a clip"):
            havc.HAVC_retinex(bad)
    for bad in (np.zeros((2, 16, 16, 4), np.uint8), np.zeros((16, 16), np.uint8), c.astype(np.float32), np.zeros((0, 16, 16, 3), np.uint8)):
        with pytest.raises(E, match="RGB24"):
            havc.HAVC_retinex(bad)
    for bad, text in (((), "0 sigmas"), ([1.0] * 9, "9 sigmas"), ((25, 0.4), "sigma = 0.4"), ((25, 10001), "sigma = 10001"), ((float("nan"),), "sigma = nan"),
                      (25, "sequence")):
        with pytest.raises(E, match=text):
            havc.HAVC_retinex(c, sigmas=bad)
    # the pinned refusals next door stay
    with pytest.raises(NotImplementedError, match="Retinex"):
        havc.HAVC_bw_tune(c, bw_method=5)


def test_retinex_np_refusals_need_no_context():
    c = np.zeros((2, 16, 16, 3), np.uint8)
    with pytest.raises(havc.HAVCError, match="sigmas"):
        RX.retinex_np(None, c, sigma=())
    with pytest.raises(havc.HAVCError, match="RGB24"):
        RX.retinex_np(None, c[..., :2])
    with pytest.raises(havc.HAVCError, match="fixed"):
        RX.retinex_np(None, c, lower_thr=0.01)


# ---- the two measurements the GPU tolerances rest on (recorded in profiles/retinex.txt) ---------------------------------------------------------------
def test_measurement_a_float32_planes_move_far_more_than_one_byte_in_a_hundred():
    """(a) the float32 run of the restatement against the float64 run on the 33 x 257 clip, the frames that pass the gate and the constant one.  Measured: 67 052 of
    101 772 bytes differ (65.9 %); the largest difference, 239, is the constant frame, which float32 does not keep stationary."""
    h, w = 33, 257
    clip = U.make_clip(h, w)[2:]
    want = U.reference_bytes(h, w, (25, 80, 250), True, True)[2:]
    got = U.msrcp(clip, (25, 80, 250), True, True, dtype=np.float32)
    n, mx = U.count_diff(got, want)
    print(f"measurement (a): float32 vs float64 at {h} x {w}: {n} of {want.size} bytes differ ({100.0 * n / want.size:.1f} %), largest difference {mx}")
    assert n > want.size // 100


def test_measurement_b_a_last_place_error_of_the_logarithm_moves_almost_nothing():
    """(b) the float64 run with its logarithm moved one ulp up or down at random (three seeds) against the unperturbed run, over the GPU test's sizes: at most
    1 LSB and fewer than 1 byte in 100 000.  Measured: 7 of 2 352 348 bytes, largest difference 1."""
    total = differ = worst = 0
    for h, w in U.SIZES:
        clip = U.make_clip(h, w)
        want = U.reference_bytes(h, w, (25, 80, 250), True, True)
        inten, _, p = U.reference(h, w, (25, 80, 250), True)
        for seed in (1, 2, 3):
            r = np.random.default_rng(seed)
            # the constant frame is left alone: every pixel has the same P, so any logarithm gives every pixel the same O, whatever its last place is
            got = np.stack([U.msrcp_frame(clip[f], inten[f], p[f], 3, True, True, log_shift=r.integers(-1, 2, inten[f].shape) * (np.ptp(p[f]) > 0))
                            for f in range(len(clip))])
            n, mx = U.count_diff(got, want)
            total, differ, worst = total + want.size, differ + n, max(worst, mx)
    print(f"measurement (b): log +- 1 ulp: {differ} of {total} bytes differ, largest difference {worst}")
    assert worst <= 1 and differ * 100000 < total
