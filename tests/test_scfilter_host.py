"""CPU (-m "not gpu"): the scene filter (vsslib/vsscdect.py:352-495; vsdeoldify_amd/scdetect.py, csrc/scfilter.hip) and the reference-frame writers
(vsdeoldify/__init__.py:3272-3416; vsdeoldify_amd/havc.py) -- scene_filter against the executed reference's selector (tests/golden/scfilter.npz,
tools/gen_golden_scfilter.py), the numpy SSIM restatement against the scipy.ndimage form skimage evaluates, the kernels' arithmetic as the library
compiles it for the host, the Hellinger score, the writers' naming rules and bytes, and every refusal before a GPU context exists."""
import inspect
import os

import numpy as np
import pytest
from PIL import Image

from tests import scfilter_util as U
from tests.conftest import ROOT
from vsdeoldify_amd import _native as nat
from vsdeoldify_amd import havc
from vsdeoldify_amd import scdetect as SD

HEADER = os.path.join(ROOT, "include", "havc_mi355.h")


@pytest.fixture
def no_gpu(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a GPU context was asked for")
    monkeypatch.setattr(havc, "get_context", refuse)


def test_scene_filter_equals_the_executed_reference():
    g = U.fixture()
    assert "executing the reference" in str(g["provenance"])
    K, A, B = (int(v) for v in g["key"])
    n_cases = int(g["n_cases"])
    assert n_cases >= 7
    chunks, reasons_seen, skipped = set(), set(), 0
    for i in range(n_cases):
        p = U.params(g, f"case_{i}_params")
        asked = []

        def scores(t_n, last):
            asked.append((t_n, last))
            k = (A * t_n + B * last) % K
            return np.float64(g["ssim_table"][k]), float(g["hist_table"][k])

        in_prev, luma, ratio = g[f"case_{i}_in_prev"], g[f"case_{i}_luma"], g[f"case_{i}_ratio"]
        dbg = {}
        prev, nxt = SD.scene_filter(in_prev, np.zeros(len(in_prev), np.int8), luma, ratio, scores, p["ssim_tht"], p["min_length"], p["tht_white"],
                                    p["tht_black"], p["frequency"], chunk=p["chunk"], debug=dbg)
        assert np.array_equal(prev, g[f"case_{i}_prev"]) and np.array_equal(nxt, g[f"case_{i}_next"]), i
        assert asked == [tuple(int(v) for v in r) for r in g[f"case_{i}_pairs"]], i       # the same scores, of the same pairs, in the same order
        assert prev[0] == 1 and not (prev & ~np.maximum(in_prev, np.eye(1, len(prev), 0, dtype=np.int8)[0])).any()   # the filter only removes (frame 0 aside)
        chunks.add(p["chunk"])
        reasons_seen |= set(dbg["reasons"].values())
        skipped += sum(1 for r in dbg["reasons"].values() if r == -1)
        if p["ssim_tht"] == 1:
            assert not asked and set(dbg["scores"].values()) == {(1, 1)}                   # :432-433: no score is taken, both are set to 1
    assert SD.FILTER_CHUNK == 5000 in chunks and len(chunks) >= 3
    assert {-1, 0, 1, 2, 3, 5, 6, 7} <= reasons_seen and skipped > 0                      # every exit of the selector, with and without the interval's +4
    # a wrong chunk length changes the answer: the chunk-local n is not decoration
    p = U.params(g, "case_4_params")
    k = lambda t_n, last: (np.float64(g["ssim_table"][(A * t_n + B * last) % K]), float(g["hist_table"][(A * t_n + B * last) % K]))
    prev, _ = SD.scene_filter(g["case_4_in_prev"], np.zeros(48, np.int8), g["case_4_luma"], g["case_4_ratio"], k, p["ssim_tht"], p["min_length"],
                              p["tht_white"], p["tht_black"], p["frequency"], chunk=5000)
    assert not np.array_equal(prev, g["case_4_prev"])


def test_numpy_ssim_equals_the_uniform_filter_form():
    pytest.importorskip("scipy")
    worst = 0.0
    for h, w in U.SHAPES + [(48, 64), (120, 213)]:
        clip, pairs = U.kernel_clip(h, w)
        g = U.gray(clip)
        for a, b in pairs:
            s, t = U.ssim_np(g[a], g[b]), U.ssim_scipy(g[a], g[b])
            worst = max(worst, abs(float(s) - float(t)))
            assert abs(float(s) - float(t)) <= 1e-12, (h, w, a, b, s, t)
            if a == b:
                assert s == 1.0
    # two constant planes: zero variances leave only C2 -> the luminance term alone
    flat = U.ssim_np(np.full((9, 9), 37, np.uint8), np.full((9, 9), 201, np.uint8))
    assert abs(flat - (2 * 37 * 201 + U.C1) / (37 ** 2 + 201 ** 2 + U.C1)) < 1e-15
    print(f"numpy integer-sum SSIM against the uniform_filter form: max difference {worst:.3e}")


def test_host_compiled_kernel_arithmetic_equals_numpy():
    lib = nat.load()
    r = np.random.default_rng(3)
    rgb = np.concatenate([r.integers(0, 256, (500, 3)), [[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255]]]).astype(np.uint8)
    assert [lib.havc_scene_gray(int(a), int(b), int(c)) for a, b, c in rgb] == list(U.gray(rgb))
    # oracle/cvcolor.py: the Y of COLOR_RGB2YUV is the same expression -> one gray value serves the SSIM plane and the histogram
    from oracle import cvcolor
    assert np.array_equal(cvcolor.rgb2yuv_u8(rgb)[:, 0], U.gray(rgb)) and (cvcolor.R2Y, cvcolor.G2Y, cvcolor.B2Y, cvcolor.YUV_SHIFT) == (4899, 9617, 1868, 14)
    for h, w, (a, b) in ((9, 13, (0, 1)), (9, 13, (3, 4)), (8, 8, (2, 0)), (7, 7, (5, 6))):
        clip, _ = U.kernel_clip(h, w)
        g = U.gray(clip).astype(np.int64)
        sums = [U.window_sums(x) for x in (g[a], g[b], g[a] * g[a], g[b] * g[b], g[a] * g[b])]
        got = np.array([lib.havc_scene_ssim_value(*(int(s[i, j]) for s in sums)) for i in range(h - 6) for j in range(w - 6)]).reshape(h - 6, w - 6)
        assert np.abs(got - U.ssim_map_np(g[a], g[b])).max() < 1e-14
    assert lib.havc_scene_ssim_value(49 * 255, 49 * 255, 49 * 65025, 49 * 65025, 49 * 65025) == 1.0      # the largest sums there are


def test_hellinger_score():
    r = np.random.default_rng(9)
    h = r.integers(0, 500, 256)
    assert round(1 - SD.hellinger_distance(h, h), 4) == 1.0 and SD.hellinger_distance(h, h) < 1e-7     # identical: 1 (sqrt of a rounding residue at most)
    assert SD.hellinger_distance(h, 7 * h) < 1e-7                                                        # the L2 normalisation takes the frame size out
    a, b = np.zeros(256, np.int64), np.zeros(256, np.int64)
    a[:100], b[150:] = 5, 9
    assert SD.hellinger_distance(a, b) == 1.0 and round(1 - SD.hellinger_distance(a, b), 4) == 0.0       # disjoint: 0
    one, other = np.zeros(256, np.int64), np.zeros(256, np.int64)
    one[37], other[201] = 3072, 3072                                                                     # two flat frames
    assert SD.hellinger_distance(one, other) == 1.0 and SD.hellinger_distance(one, one) == 0.0
    # against the definition written out: normalised histograms p, q -> sqrt(1 - sum sqrt(p q) / sqrt(sum p sum q))
    k = r.integers(0, 500, 256)
    p, q = h / np.sqrt((h * h).sum()), k / np.sqrt((k * k).sum())
    assert abs(SD.hellinger_distance(h, k) - np.sqrt(1 - np.sqrt(p * q).sum() / np.sqrt(p.sum() * q.sum()))) < 1e-12
    assert SD.hellinger_distance(np.zeros(256), np.zeros(256)) == 1.0                                    # |s1 s2| <= FLT_EPSILON: the factor is 1


def _clip(n=7, h=10, w=12, seed=2):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def _pil_bytes(arr, path, ext, quality=95):
    img = Image.fromarray(arr, 'RGB')
    if ext == "jpg":
        img.save(path, subsampling=0, quality=quality)
    else:
        img.save(path)
    return open(path, "rb").read()


def test_export_naming_offset_sequence_and_override(tmp_path, no_gpu):
    clip = _clip()
    scenes = SD.SceneInfo(np.array([0, 0, 1, 0, 1, 1, 0], np.int8), np.zeros(7, np.int8), np.full(7, 0.5), np.zeros(7), 0.1, 0)
    d, dbg = str(tmp_path / "a" / "b"), {}
    assert havc.HAVC_export_reference_frames(clip, d, scenes=scenes, debug=dbg) is clip                   # the directory is made, parents included
    assert sorted(os.listdir(d)) == ["ref_000000.jpg", "ref_000002.jpg", "ref_000004.jpg", "ref_000005.jpg"]      # frame 0 although it is not flagged
    assert dbg["written"] == [os.path.join(d, f) for f in sorted(os.listdir(d))]
    for f, n in zip(sorted(os.listdir(d)), (0, 2, 4, 5)):
        assert open(os.path.join(d, f), "rb").read() == _pil_bytes(clip[n], str(tmp_path / "want.jpg"), "jpg")
    d2 = str(tmp_path / "png")
    havc.HAVC_export_reference_frames(clip, d2, ref_offset=100, ref_ext="PNG", scenes=scenes)
    assert sorted(os.listdir(d2)) == ["ref_000100.png", "ref_000102.png", "ref_000104.png", "ref_000105.png"]    # the extension in lower case, as the writer's
    assert open(os.path.join(d2, "ref_000104.png"), "rb").read() == _pil_bytes(clip[4], str(tmp_path / "want.png"), "png")
    assert np.array_equal(np.asarray(Image.open(os.path.join(d2, "ref_000104.png"))), clip[4])
    # quality reaches the encoder
    d3 = str(tmp_path / "q")
    havc.HAVC_export_reference_frames(clip, d3, ref_jpg_quality=40, scenes=scenes)
    assert open(os.path.join(d3, "ref_000002.jpg"), "rb").read() == _pil_bytes(clip[2], str(tmp_path / "want40.jpg"), "jpg", 40)
    # HAVC_extract_reference_frames on the early returns (no pixel is read, no context): every second frame; sequence numbering ignores ref_offset
    d4, dbg = str(tmp_path / "seq"), {}
    info = havc.HAVC_extract_reference_frames(clip, sc_threshold=0, sc_min_freq=2, sc_framedir=d4, sc_sequence=True, ref_offset=50, ref_ext="png", debug=dbg)
    assert list(info.scene_change_prev) == [1, 0, 1, 0, 1, 0, 1] and (info.sc_threshold, info.sc_frequency) == (0, 2)
    assert sorted(os.listdir(d4)) == [f"ref_{i:06d}.png" for i in range(4)] and len(dbg["written"]) == 4
    assert np.array_equal(np.asarray(Image.open(os.path.join(d4, "ref_000003.png"))), clip[6])
    d5 = str(tmp_path / "off")
    havc.HAVC_extract_reference_frames(clip, sc_min_freq=1, sc_framedir=d5, ref_offset=50, ref_ext="png", sc_tht_ssim=0.6, sc_min_int=10)     # frequency 1 returns before the filter
    assert sorted(os.listdir(d5)) == [f"ref_{i + 50:06d}.png" for i in range(7)]
    # ref_override=False leaves an existing file alone (and, with sequence, still counts it)
    marker = os.path.join(d4, "ref_000001.png")
    open(marker, "wb").write(b"kept")
    os.remove(os.path.join(d4, "ref_000002.png"))
    dbg = {}
    havc.HAVC_extract_reference_frames(clip, sc_threshold=0, sc_min_freq=2, sc_framedir=d4, sc_sequence=True, ref_ext="png", ref_override=False, debug=dbg)
    assert open(marker, "rb").read() == b"kept" and dbg["written"] == [os.path.join(d4, "ref_000002.png")]
    assert np.array_equal(np.asarray(Image.open(os.path.join(d4, "ref_000002.png"))), clip[4])
    havc.HAVC_extract_reference_frames(clip, sc_threshold=0, sc_min_freq=2, sc_framedir=d4, sc_sequence=True, ref_ext="png")
    assert np.array_equal(np.asarray(Image.open(marker)), clip[2])                                       # the default overrides
    # no scene change at all (threshold 0, frequency 0): frame 0 alone
    d6 = str(tmp_path / "none")
    assert not havc.HAVC_extract_reference_frames(clip, sc_threshold=0, sc_framedir=d6).scene_change_prev.any()
    assert os.listdir(d6) == ["ref_000000.jpg"]


def test_exported_directory_is_read_back_by_the_remaster(tmp_path, no_gpu):
    from vsdeoldify_amd import remaster_render as RR
    clip = _clip(n=12)
    d = str(tmp_path / "refs")
    havc.HAVC_extract_reference_frames(clip, sc_threshold=0, sc_min_freq=5, sc_framedir=d, ref_ext="png")
    files, numbers = RR.get_ref_list(d)
    assert numbers == [0, 5, 10] and [os.path.basename(f) for f in files] == ["ref_000000.png", "ref_000005.png", "ref_000010.png"]
    for f, n in zip(files, numbers):
        assert np.array_equal(np.asarray(Image.open(f).convert("RGB")), clip[n])


def test_export_list_frames_rules(tmp_path, no_gpu):
    clip = _clip(n=10)

    def names(d):
        return sorted(os.listdir(d)) if os.path.isdir(d) else None

    d = str(tmp_path / "none")
    assert havc.HAVC_export_list_frames(clip, d) is clip and havc.HAVC_export_list_frames(clip, d, ref_list=[]) is clip and names(d) is None
    d = str(tmp_path / "every")
    assert havc.HAVC_export_list_frames(clip, d, ref_list=[4], ref_ext="png") is clip                     # ONE number: every 4th frame
    assert names(d) == ["ref_000000.png", "ref_000004.png", "ref_000008.png"]
    d = str(tmp_path / "list")
    havc.HAVC_export_list_frames(clip, d, ref_list=[7, 2, 7, 3], ref_ext="png")                           # sorted, duplicates dropped
    assert names(d) == ["ref_000002.png", "ref_000003.png", "ref_000007.png"]
    assert np.array_equal(np.asarray(Image.open(os.path.join(d, "ref_000007.png"))), clip[7])
    d = str(tmp_path / "offset")
    havc.HAVC_export_list_frames(clip, d, ref_list=[0, 5], offset=2, ref_ext="png")                       # the frame AT number + offset, named so
    assert names(d) == ["ref_000002.png", "ref_000007.png"] and np.array_equal(np.asarray(Image.open(os.path.join(d, "ref_000007.png"))), clip[7])
    d = str(tmp_path / "offset_every")
    havc.HAVC_export_list_frames(clip, d, ref_list=[4], offset=1)
    assert names(d) == ["ref_000001.jpg", "ref_000005.jpg", "ref_000009.jpg"]
    assert open(os.path.join(d, "ref_000005.jpg"), "rb").read() == _pil_bytes(clip[5], str(tmp_path / "w.jpg"), "jpg")
    with pytest.raises(havc.HAVCError, match="range"):
        havc.HAVC_export_list_frames(clip, str(tmp_path / "bad"), ref_list=[1, 10])                       # fast_extract picks frames: 10 is outside
    with pytest.raises(havc.HAVCError, match="range"):
        havc.HAVC_export_list_frames(clip, str(tmp_path / "bad"), ref_list=[4], offset=2)                 # 8 + 2
    d = str(tmp_path / "walk")
    havc.HAVC_export_list_frames(clip, d, ref_list=[1, 10, 12], ref_ext="png", fast_extract=False)        # the whole clip is walked: 10 and 12 are never met
    assert names(d) == ["ref_000001.png"]
    open(os.path.join(d, "ref_000001.png"), "wb").write(b"kept")
    havc.HAVC_export_list_frames(clip, d, ref_list=[1, 2], ref_ext="png", ref_override=False)
    assert open(os.path.join(d, "ref_000001.png"), "rb").read() == b"kept" and names(d) == ["ref_000001.png", "ref_000002.png"]
    with pytest.raises(havc.HAVCError, match="step"):
        havc.HAVC_export_list_frames(clip, d, ref_list=[0])


def test_signatures_equal_the_reference():
    def args(fn):
        return [(k, v.default) for k, v in inspect.signature(fn).parameters.items() if v.kind is v.POSITIONAL_OR_KEYWORD][1:]

    def extras(fn):
        return sorted(k for k, v in inspect.signature(fn).parameters.items() if v.kind is v.KEYWORD_ONLY)
    assert args(havc.HAVC_extract_reference_frames) == [                                                 # vsdeoldify/__init__.py:3272-3278
        ("sc_threshold", 0.10), ("sc_tht_offset", 1), ("sc_tht_ssim", 0.0), ("sc_min_int", 1), ("sc_min_freq", 0), ("sc_framedir", "./"),
        ("sc_sequence", False), ("sc_normalize", False), ("ref_offset", 0), ("sc_tht_white", 0.70), ("sc_tht_black", 0.10), ("ref_ext", "jpg"),
        ("ref_jpg_quality", 95), ("ref_override", True), ("sc_algo", 0), ("sc_debug", False)]
    assert args(havc.HAVC_export_reference_frames) == [("sc_framedir", "./"), ("ref_offset", 0), ("ref_ext", "jpg"), ("ref_jpg_quality", 95),
                                                       ("ref_override", True)]                            # :3364-3366
    assert args(havc.HAVC_export_list_frames) == [("sc_framedir", "./"), ("ref_list", None), ("offset", 0), ("ref_ext", "jpg"), ("ref_jpg_quality", 95),
                                                  ("ref_override", True), ("fast_extract", True)]         # :3387-3389
    assert extras(havc.HAVC_extract_reference_frames) == ["debug", "device_index", "luma_range"]
    assert extras(havc.HAVC_export_reference_frames) == ["debug", "scenes"] and extras(havc.HAVC_export_list_frames) == ["debug"]
    import vsdeoldify_amd
    for name in ("HAVC_extract_reference_frames", "HAVC_export_reference_frames", "HAVC_export_list_frames"):
        assert getattr(vsdeoldify_amd, name) is getattr(havc, name)
    # the filter's constants (vsslib/constants.py:42-54)
    assert (SD.DEF_THT_BLACK_FREQ, SD.DEF_THT_BLACK_MIN, SD.DEF_THT_WHITE_MIN, SD.DEF_ADAPTIVE_RATIO_RF) == (0.14, 0.19, 0.70, 2.0)
    assert (SD.DEF_SSIM_SCORE_EQUAL, SD.DEF_HIST_SCORE_EQUAL, SD.DEF_HIST_SCORE_HIGH) == (0.69, 0.70, 0.95)


def test_refusals_come_before_any_gpu_work(tmp_path, no_gpu):
    clip = _clip()
    d = str(tmp_path / "never")
    for algo, plugin in ((1, "TCanny.*akarin"), (2, "SCXvid"), (3, "MVTools")):
        with pytest.raises(NotImplementedError, match=plugin):
            havc.HAVC_extract_reference_frames(clip, sc_framedir=d, sc_algo=algo)
    with pytest.raises(havc.HAVCError, match="sc_algo"):
        havc.HAVC_extract_reference_frames(clip, sc_framedir=d, sc_algo=4)
    for bad in (None, [[1, 2, 3]]):
        with pytest.raises(havc.HAVCError, match="not a clip"):
            havc.HAVC_extract_reference_frames(bad, sc_framedir=d)
        with pytest.raises(havc.HAVCError, match="not a clip"):
            havc.HAVC_export_reference_frames(bad, d)
        with pytest.raises(havc.HAVCError, match="not a clip"):
            havc.HAVC_export_list_frames(bad, d, ref_list=[1, 2])
    with pytest.raises(havc.HAVCError, match="luma_range"):
        havc.HAVC_extract_reference_frames(clip, sc_framedir=d, luma_range="pc")
    with pytest.raises(havc.HAVCError, match="extension"):
        havc.HAVC_extract_reference_frames(clip, sc_framedir=d, ref_ext="nope")
    with pytest.raises(havc.HAVCError, match="RGB24"):
        havc.HAVC_extract_reference_frames(np.zeros((3, 8, 8, 1), np.uint8), sc_framedir=d)
    with pytest.raises(havc.HAVCError, match="scenes="):
        havc.HAVC_export_reference_frames(clip, d)
    with pytest.raises(havc.HAVCError, match="scenes="):
        havc.HAVC_export_reference_frames(clip, d, scenes=SD.scene_flags(np.zeros(3, np.int64), np.zeros(3, np.int64), 4, 0, 1))
    # a frame below 7 x 7 with the SSIM filter on: skimage raises there
    for shape in ((3, 6, 9, 3), (3, 9, 6, 3)):
        with pytest.raises(havc.HAVCError, match="7 x 7"):
            havc.HAVC_extract_reference_frames(np.zeros(shape, np.uint8), sc_framedir=d, sc_tht_ssim=0.6)
        with pytest.raises(ValueError, match="7 x 7"):
            SD.scene_detect_filtered(None, np.zeros(shape, np.uint8), sc_tht_filter=0.6)
    assert not os.path.exists(d)                                                                         # nothing was created on the way
    with pytest.raises(ValueError, match="post-filter is off"):
        SD.scene_detect_filtered(None, clip)
    # the early returns of the filtered detector touch no pixel and need no context
    info = SD.scene_detect_filtered(None, clip, threshold=0, frequency=3, sc_tht_filter=0.6, min_length=10)
    assert list(info.scene_change_prev) == [1, 0, 0, 1, 0, 0, 1]
    assert SD.filter_active(0.6, 1) and SD.filter_active(0.0, 2) and SD.filter_active(1.0, 99) and not SD.filter_active(0.0, 1)
    assert not SD.filter_active(1.0, 1) and not SD.filter_active(0.0, 0) and not SD.filter_active(1.5, -4)
    # HAVC_SceneDetect keeps its refusal
    for kw in (dict(sc_tht_ssim=0.5), dict(sc_min_int=5)):
        with pytest.raises(NotImplementedError, match="structural_similarity"):
            havc.HAVC_SceneDetect(clip, **kw)


def test_c_abi_declares_the_filter_kernels():
    src = open(HEADER).read()
    assert "int havc_scene_hist(havc_ctx* ctx, const uint8_t* clip, int n_frames, int width, int height, const int* idx, int k, uint32_t* out);" in src
    assert "int havc_scene_ssim(havc_ctx* ctx, const uint8_t* clip, int n_frames, int width, int height, const int* pairs, int m, double* out);" in src
    sym = {s[0]: s for s in nat.SYMBOLS}
    assert len(sym["havc_scene_hist"][2]) == 8 and len(sym["havc_scene_ssim"][2]) == 8
    kern = open(os.path.join(ROOT, "vsdeoldify_amd", "csrc", "kernels.h")).read()
    assert f"constexpr int SCF_SSIM_TILE = {U.TILE};" in kern                                            # the tile the GPU test's shapes straddle
