"""CPU (-m "not gpu"): the host side of HAVC_restore_video -- its signature, checks, refusals and parameter defaulting (vsdeoldify/__init__.py:1959-2083),
the clip-mode reference window of DeepRemaster (remaster_render.ClipReferenceWindow) step by step against the reference's RemasterColorizer
(tests/golden/restore_video.npz, tools/gen_golden_restore.py), the float64 Spline36 reference of tests/restore_util.py, the plan query of the new resize
entry point, and the near-tie condition of every Spline36 case of tests/test_gpu_restore.py, from the reference alone."""
import inspect
import os

import numpy as np
import pytest

from tests import resize_util as RU
from tests import restore_util as U
from vsdeoldify_amd import _native as nat

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def lib():
    return nat.load()


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "restore_video.npz"))


# ---- HAVC_restore_video: signature, checks, refusals, defaults ----
def test_signature_and_defaults():
    from vsdeoldify_amd import HAVC_restore_video
    want = dict(clip=None, clip_ref=None, method=6, render_speed='medium', ex_model=0, ref_merge=0, ref_weight=None, ref_thresh=None, ref_freq=None,
                ref_norm=False, max_memory_frames=0, render_vivid=True, encode_mode=0, encode_first=True, torch_dir=None)
    params = inspect.signature(HAVC_restore_video).parameters.values()
    pos = [p for p in params if p.kind == p.POSITIONAL_OR_KEYWORD]
    assert [p.name for p in pos] == list(want) and {p.name: p.default for p in pos} == want
    assert [p.kind for p in params if p.kind != p.POSITIONAL_OR_KEYWORD] == [inspect.Parameter.VAR_KEYWORD]


def test_checks_and_refusals_by_message():
    from vsdeoldify_amd import HAVC_restore_video
    from vsdeoldify_amd.havc import HAVCError
    clip, ref = np.zeros((3, 32, 48, 3), np.uint8), np.zeros((3, 36, 54, 3), np.uint8)
    for kw, exc, text in ((dict(clip=None, clip_ref=ref), HAVCError, "HAVC_restore_video: this is not a clip"),
                          (dict(clip=clip, clip_ref=None), HAVCError, "HAVC_restore_video: this is not a clip"),
                          (dict(clip=clip, clip_ref=[1, 2]), HAVCError, "HAVC_restore_video: this is not a clip"),
                          (dict(clip=clip, clip_ref=ref, method=0), HAVCError, "HAVC: Video restore is supported only with methods: 5, 6"),
                          (dict(clip=clip, clip_ref=ref, method=2), HAVCError, "HAVC: Video restore is supported only with methods: 5, 6"),
                          (dict(clip=clip, clip_ref=ref, ex_model=3), HAVCError, "HybridAVC: unknown exemplar model id: 3"),
                          (dict(clip=clip, clip_ref=ref, ex_model=7), HAVCError, "HybridAVC: unknown exemplar model id: 7"),
                          (dict(clip=clip, clip_ref=ref[:2]), HAVCError, "clip_ref has 2 frames, clip has 3"),
                          (dict(clip=clip, clip_ref=ref[:2], ex_model=2, render_vivid=False), HAVCError, "clip_ref has 2 frames, clip has 3"),
                          (dict(clip=clip, clip_ref=ref, ex_model=1), NotImplementedError, "ex_model 1 (Deep-Exemplar) is not built"),
                          (dict(clip=clip, clip_ref=ref, ex_model=2), NotImplementedError, "render_vivid is vs_tweak (a zimg YUV420 round trip): not in this harness"),
                          (dict(clip=clip, clip_ref=ref, ex_model=2, render_vivid=True), NotImplementedError, "render_vivid is vs_tweak"),
                          (dict(clip=clip, clip_ref=ref, encode_mode=2), NotImplementedError, "encode_mode = 2 is not built"),
                          (dict(clip=clip, clip_ref=ref, ex_model=2, render_vivid=False, encode_mode=2), NotImplementedError, "encode_mode = 2 is not built"),
                          (dict(clip=clip, clip_ref=ref, render_speed="warp"), HAVCError, "unknown render_speed ->warp"),
                          (dict(clip=clip, clip_ref=ref, ex_model=2, render_vivid=False, render_speed="warp"), HAVCError, "unknown render_speed ->warp"),
                          (dict(clip=np.zeros((3, 32, 48), np.uint8), clip_ref=ref), HAVCError, "only RGB24 clips"),
                          (dict(clip=clip, clip_ref=ref, colormap="none"), TypeError, "unexpected keyword arguments ['colormap']")):
        with pytest.raises(exc) as e:
            HAVC_restore_video(**kw)
        assert text in str(e.value), (list(kw), str(e.value))


def test_the_refusals_this_route_points_at_stay():
    from vsdeoldify_amd import HAVC_DeepRemaster, HAVC_deepex
    clip = np.zeros((2, 32, 32, 3), np.uint8)
    with pytest.raises(NotImplementedError, match="HAVC_restore_video"):
        HAVC_deepex(clip, clip, method=5, sc_framedir="x")
    with pytest.raises(NotImplementedError, match="mode = 1"):
        HAVC_DeepRemaster(clip, ref_dir=GOLDEN, mode=1)


@pytest.mark.parametrize("args, want", [
    # (method, ex_model, ref_merge, ref_weight, ref_thresh, ref_freq) -> (ref_thresh, ref_freq, ref_weight, merge)
    ((6, 0, 0, None, None, None), (0.10, 0, 1.0, False)),
    ((6, 2, 0, None, None, None), (0.10, 10, 1.0, False)),
    ((6, 2, 0, None, 0, 0), (0.10, 10, 1.0, False)),
    ((6, 0, 3, 0.8, 0.2, 25), (0.2, 25, 1.0, False)),          # method 6 never merges, whatever ref_merge says
    ((5, 0, 0, 0.8, None, None), (0.10, 0, 1.0, False)),       # ref_merge 0: the weight is 1.0
    ((5, 0, 1, None, None, None), (0.10, 0, 0.3, True)),
    ((5, 0, 2, None, None, None), (0.10, 0, 0.4, True)),
    ((5, 0, 3, None, None, None), (0.10, 0, 0.5, True)),
    ((5, 0, 4, 0, None, None), (0.10, 0, 0.6, True)),          # a weight of 0 counts as unset
    ((5, 2, 5, None, 0.15, None), (0.15, 10, 0.7, True)),
    ((5, 2, 3, 0.25, None, 40), (0.10, 40, 0.25, True)),
])
def test_parameter_defaulting_table(args, want):
    from vsdeoldify_amd.havc import restore_video_params
    assert restore_video_params(*args) == want


# ---- the clip-mode reference window against the reference's RemasterColorizer, call by call ----
@pytest.mark.parametrize("name", ["short", "extends", "sparse"])
def test_window_trace_step_by_step(fx, name):
    from vsdeoldify_amd.remaster_render import ClipReferenceWindow
    flags, size, trace = fx[f"trace_{name}_flags"], int(fx[f"trace_{name}_size"]), fx[f"trace_{name}"]
    w = ClipReferenceWindow(flags, size)
    assert [len(w.nums), w.size, w.clip_last_frame] == fx[f"trace_{name}_found"].tolist()
    N = len(flags)
    assert len(trace) == (N + 1) // 2
    slots_seen = set()
    for k, n0 in enumerate(range(0, N, 2)):
        moved = w.advance(min(n0 + 1, N - 1))
        if moved is not None:
            slots_seen.add(moved[0])
            assert w.nums[moved[1]] == trace[k][w.size - 1]                   # the still that enters is the newest of the window
        assert w.numbers() + [len(w.nums), w.clip_last_frame] == trace[k].tolist(), (name, k)
    assert sorted(w.slots) == list(range(len(w.nums) - w.size, len(w.nums))) and w.nums == np.flatnonzero(flags).tolist()
    assert len(slots_seen) == min(w.size, len(w.nums) - w.size), "an advance overwrites the oldest slot: the slots take turns"
    if name == "short":
        assert w.clip_last_frame == N - 1 == int(fx["trace_short_found"][2])         # at most 500 frames: one scan, never extended
    if name == "sparse":
        assert int(fx["trace_sparse_found"][2]) == N - 1 and len(np.flatnonzero(flags[:500])) == 1      # two extensions inside get_clip_ref_list
    if name == "extends":
        # ref_buffer_adjust extends on the first call (1 >= 499 - 500) and again once frame_n reaches 999 - 500
        assert int(fx["trace_extends_found"][2]) == 499 and trace[0][-1] == 999 and int(np.argmax(trace[:, -1] == N - 1)) == 249


def test_fewer_than_four_references_raise_with_the_reference_message(fx):
    from vsdeoldify_amd.havc import HAVCError
    from vsdeoldify_amd.remaster_render import ClipReferenceWindow
    msg = str(fx["trace_three_error"])
    assert msg == "RemasterColorizer(): number of reference frames must be at least 2, found  3"
    with pytest.raises(HAVCError) as e:
        ClipReferenceWindow(fx["trace_three_flags"], int(fx["trace_three_size"]))
    assert str(e.value) == msg


def test_window_of_the_clip_fixture(fx):
    from vsdeoldify_amd.remaster_render import ClipReferenceWindow, target_size
    w = ClipReferenceWindow(fx["flags"], int(fx["params"][1]))
    assert len(w.nums) == int(fx["found"]) == 7
    trace = []
    for n0 in range(0, len(fx["flags"]), 2):
        w.advance(min(n0 + 1, len(fx["flags"]) - 1))
        trace.append(w.numbers())
    assert trace == fx["trace"].tolist()
    assert target_size(fx["clip_ref"].shape[2], fx["clip_ref"].shape[1], int(fx["params"][0])) == tuple(fx["target_wh"])


def test_fixture_holds_data_only_and_stays_small(fx):
    assert not any(fx[k].dtype == object for k in fx.files)
    assert os.path.getsize(os.path.join(GOLDEN, "restore_video.npz")) <= os.path.getsize(os.path.join(GOLDEN, "remaster_render.npz"))
    assert "executing the reference" in str(fx["provenance"])


# ---- Spline36: the float64 reference and the plan query ----
def test_spline36_kernel_interpolates_and_has_support_three():
    k = np.arange(-4, 5)
    assert np.array_equal(U.spline36(k), (k == 0).astype(np.float64))             # 1 at 0, 0 at every other integer: exactly
    assert np.all(U.spline36(np.array([3.0, 3.5, -3.0, 10.0])) == 0.0)
    x = np.linspace(-3, 3, 6001)
    assert np.array_equal(U.spline36(x), U.spline36(-x)) and -0.13 < U.spline36(x).min() < -0.11
    assert abs(U.spline36(0.5) - (((13 / 11 * 0.5 - 453 / 209) * 0.5 - 3 / 209) * 0.5 + 1)) < 1e-15 and abs(U.spline36(0.5) - 0.598684) < 1e-6


@pytest.mark.parametrize("src, dst", [(40, 130), (96, 260), (83, 83), (520, 260), (42, 12), (93, 24), (600, 96), (7, 1), (1, 5)])
def test_spline36_taps_partition_of_unity(src, dst):
    pos, w = U.taps36(src, dst)
    assert w.shape == (dst, U.n_taps(src, dst)) and pos.min() >= 0 and pos.max() <= src - 1
    assert np.abs(w.sum(1) - 1.0).max() < 1e-14
    # un-normalised, the shifted kernels sum to 1 at every phase when the kernel is not stretched (the Spline36 pieces are a partition of unity)
    ph = np.linspace(0, 1, 101)[:, None]
    assert np.abs(U.spline36(ph + np.arange(-3, 3)[None, :]).sum(1) - 1.0).max() < 1e-12
    if src == dst:
        assert np.array_equal(w, (pos == np.arange(dst)[:, None]).astype(np.float64) * (np.arange(w.shape[1])[None, :] == 2))


def test_ref36_reproduces_constants_and_the_identity():
    r = np.random.default_rng(0)
    clip = r.integers(0, 256, (2, 19, 23, 3), dtype=np.uint8)
    same = U.ref36(clip, 23, 19)
    assert np.array_equal(RU.rounded(same), clip) and np.abs(same.v - clip).max() == 0 and not RU.near_ties(same).any()
    flat = np.full((1, 9, 11, 3), 77, np.uint8)
    for dw, dh in ((30, 20), (4, 3), (11, 40)):
        assert np.abs(U.ref36(flat, dw, dh).v - 77.0).max() < 1e-10


def test_plan_filter_matches_the_tables_and_the_spline64_query(lib):
    import ctypes
    for sw in list(range(1, 100)) + [255, 520, 600, 1326, 1347, 1400, 1920]:
        for dw in (1, 3, 12, 24, 96, 130, 260, 560, 1920):
            for rows in (1080, 64 * 1080):
                assert U.plan(lib, sw, dw, rows, U.SPLINE64) == RU.plan(lib, sw, dw, rows)
            assert U.plan(lib, sw, dw, 1080, U.SPLINE36)[0] == U.n_taps(sw, dw), (sw, dw)
    t, v = ctypes.c_int(), ctypes.c_int()
    for filt in (-1, 2, 9):
        assert lib.havc_resize_plan_filter(96, 260, 500, filt, ctypes.byref(t), ctypes.byref(v)) == nat.HAVC_E_INVALID
    assert lib.havc_resize_plan_filter(0, 260, 500, 1, None, None) == nat.HAVC_E_INVALID
    assert lib.havc_resize_plan_filter(1920, 560, 1080, 1, None, None) > 0


@pytest.mark.parametrize("name", list(U.CASES))
def test_spline36_gpu_cases_plan_and_near_tie_share(lib, name):
    """what tests/test_gpu_restore.py relies on for each of its cases, checked without a GPU: the kernel variant and tap count the case is named for, and
    the near-tie share of the float64 reference alone below resize_util's cap"""
    c = U.CASES[name]
    taps, variant, span = U.plan(lib, c.sw, c.dw, c.n * c.sh, U.SPLINE36)
    assert (taps, variant) == (c.taps, c.variant), (name, taps, variant, span)
    if variant:
        assert span <= 4096
    clip, _ = U.case_operands(name)
    ref = U.ref36(clip, c.dw, c.dh)
    assert (ref.n_h, ref.n_v) == (c.taps, U.n_taps(c.sh, c.dh))
    RU.assert_near_tie_share(ref, f"spline36 case {name}", per_pixel=c.luma)
