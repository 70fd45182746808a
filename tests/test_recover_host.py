"""CPU (-m "not gpu"): HAVC_recover_clip_color / ChromaRetentionMerge on clips.  The CPU reference of tests/recover_util.py against the reference EXECUTED by
tools/gen_golden_recover.py (tests/golden/recover.npz), byte for byte; the resize-size rule as a table against the sizes the fixture recorded; the signatures,
the refusals before any GPU context exists, the struct layout; and that the CPU reference can fail: switching one rule breaks fixture cases."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from tests import recover_util as U
from tests.conftest import ROOT
from vsdeoldify_amd import _native as nat
from vsdeoldify_amd import havc, mcomb

HEADER = os.path.join(ROOT, "include", "havc_mi355.h")


def _ref(params, clip, color, **kw):
    p = dict(params)
    return U.recover_clip_color_ref(clip, color, p["sat"], p["tht"], p["clipb_weight"], p["alpha"], p["mask_weight"], p["chroma_resize"],
                                    p.get("return_mask", False), p.get("binary_mask", False), 0, 0, **kw)


def test_cpu_reference_equals_the_executed_reference():
    g = U.fixture()
    assert "executing the reference" in str(g["provenance"])
    cases = U.cases()
    assert len(cases) >= 25
    seen = dict(binary=0, gradient=0, mask=0, resized=0)
    for i, p, clip, color, want, sizes in cases:
        got_sizes = []
        got = _ref(p, clip, color, sizes=got_sizes)
        assert got.shape == want.shape and got.dtype == np.uint8, (i, p)
        assert np.array_equal(got, want), (i, p, int((got != want).sum()))
        assert got_sizes == sizes, (i, p, got_sizes, sizes)
        seen["binary" if p.get("binary_mask") else "gradient"] += 1
        seen["mask"] += bool(p.get("return_mask"))
        seen["resized"] += bool(sizes)
        if p.get("return_mask"):
            assert sizes == [] and want.shape == clip.shape                   # no resize (272 wide with chroma_resize among them), no merge
            proc = want[U.BINARY_FIRST:] if p.get("binary_mask") else want
            assert (proc[..., 0] == proc[..., 1]).all() and (proc[..., 0] == proc[..., 2]).all()
        if p.get("binary_mask"):
            assert np.array_equal(want[:U.BINARY_FIRST], clip[:U.BINARY_FIRST])  # `n < 15`, return_mask included
            if p["clipb_weight"] == 1.0:
                assert not np.array_equal(want[U.BINARY_FIRST:], clip[U.BINARY_FIRST:])
    assert seen["binary"] >= 6 and seen["gradient"] >= 15 and seen["mask"] >= 4 and seen["resized"] >= 2, seen


def test_fixture_has_frames_on_both_sides_of_the_luma_gate():
    g = U.fixture()
    std_g = [U.frame_is_standard(f) for f in g["clip_g"]]
    assert std_g == [True, True, False, False]
    assert [U.frame_is_standard(f) for f in g["clip_b"][15:]] == [True, False] and [U.frame_is_standard(f) for f in g["clip_b2"][15:]] == [False, True]
    assert not U.frame_is_standard(g["clip_r"][1]) and U.frame_is_standard(g["clip_r"][0])


SIZE_TABLE = [(256, None), (272, 256), (640, 256), (704, 272), (1280, 512), (1920, 768), (3840, 768)]


def test_resize_size_rule():
    recorded = {int(w): (int(fs) or None) for w, fs in U.fixture()["size_table"]}          # what the executed reference asked Spline64 for
    assert recorded == dict(SIZE_TABLE)
    for w, fs in SIZE_TABLE:
        assert mcomb.recover_size(w) == fs and U.recover_size(w) == fs, w
    # the resized fixture cases: down twice to fs x fs, up once to W x H
    for i, p, clip, color, want, sizes in U.cases():
        w, h = clip.shape[2], clip.shape[1]
        fs = mcomb.recover_size(w) if p["chroma_resize"] and not p.get("return_mask") else None
        assert sizes == ([] if fs is None else [(fs, fs), (fs, fs), (w, h)]), (i, sizes)
    assert mcomb.recover_size(1920) == 768                                    # HAVC_merge's own rule caps rf at 32: 512 there


def test_signatures_equal_the_reference():
    def pos(fn):
        return [(k, v.default) for k, v in inspect.signature(fn).parameters.items() if v.kind is v.POSITIONAL_OR_KEYWORD]
    assert pos(havc.HAVC_recover_clip_color) == [("clip", None), ("clip_color", None), ("sat", 0.8), ("tht", 30), ("strength", 1.0), ("alpha", 2.0),
                                                 ("mask_weight", 1.0), ("chroma_resize", True), ("return_mask", False), ("binary_mask", False),
                                                 ("algo", 0)]                 # __init__.py:2956-2958
    assert pos(mcomb.chroma_retention_merge_clip) == [("a", inspect.Parameter.empty), ("b", inspect.Parameter.empty), ("sat", 0.8), ("tht", 30),
                                                      ("clipb_weight", 0.9), ("alpha", 2.0), ("mask_weight", 0.0), ("chroma_resize", True),
                                                      ("return_mask", False), ("binary_mask", False), ("algo", 0), ("first_frame", 0),
                                                      ("device_index", 0)]   # mcomb.py:450-453
    import vsdeoldify_amd
    assert vsdeoldify_amd.HAVC_recover_clip_color is havc.HAVC_recover_clip_color
    assert "HAVC_recover_clip_color" in havc.__doc__


def test_refusals_come_before_any_gpu_work(monkeypatch):
    def no_gpu(*a, **k):
        raise AssertionError("GPU work was started")
    monkeypatch.setattr(havc, "get_context", no_gpu)
    monkeypatch.setattr(mcomb, "get_context", no_gpu)
    c = np.zeros((2, 16, 16, 3), np.uint8)
    E = havc.HAVCError
    for bad in (None, [[1, 2, 3]], "clip"):
        with pytest.raises(E, match="^HAVC_merge: this is not a clip: clip_color$"):      # __init__.py:2983-2984: the reference's own text
            havc.HAVC_recover_clip_color(c, bad)
        with pytest.raises(E, match="this is not a clip"):
            havc.HAVC_recover_clip_color(bad, c)
    with pytest.raises(E, match="differ in size"):
        havc.HAVC_recover_clip_color(c, np.zeros((2, 16, 24, 3), np.uint8))
    with pytest.raises(E, match="differ in size"):
        havc.HAVC_recover_clip_color(c, c[0])
    with pytest.raises(E, match="RGB24"):
        havc.HAVC_recover_clip_color(np.zeros((2, 16, 16, 4), np.uint8), np.zeros((2, 16, 16, 4), np.uint8))
    with pytest.raises(E, match="RGB24"):
        havc.HAVC_recover_clip_color(c.astype(np.float32), c.astype(np.float32))
    with pytest.raises(E, match="RGB24"):
        havc.HAVC_recover_clip_color(c[0, 0], c[0, 0])
    for algo in (-1, 3, 1.5, None):
        with pytest.raises(E, match="algo"):
            havc.HAVC_recover_clip_color(c, c, algo=algo)


def test_struct_layout_and_symbol_equal_the_header():
    src = open(HEADER).read()
    body = re.search(r"typedef struct havc_recover_params \{(.*?)\} havc_recover_params;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), {"int": ctypes.c_int, "double": ctypes.c_double}[ctype]) for n in names.split(",")]
    assert fields == list(nat.RecoverParams._fields_)
    assert [n for n, _ in fields] == ["width", "height", "n_frames", "first_frame", "sat", "tht", "algo", "weight", "alpha", "binary_mask", "return_mask"]
    assert ctypes.sizeof(nat.RecoverParams) == 56
    assert re.search(r"int havc_recover_color_clip\(havc_ctx\* ctx, const uint8_t\* gray, const uint8_t\* color, uint8_t\* out, const havc_recover_params\* params\);", src)
    assert ("havc_recover_color_clip", ctypes.c_int, [ctypes.c_void_p] * 5) in nat.SYMBOLS


# ---- the CPU reference can fail: one rule switched, and fixture cases break ----
def _broken(rule):
    return [i for i, p, clip, color, want, _ in U.cases() if not np.array_equal(_ref(p, clip, color, rules=(rule,)), want)]


def test_flipping_the_gate_breaks_cases_of_both_paths():
    bad = _broken("flip_gate")
    kinds = {bool(U.cases()[i][1].get("binary_mask")) for i in bad}
    assert kinds == {False, True}, bad


def test_dropping_the_n15_rule_breaks_binary_cases_only():
    bad = _broken("no_n15")
    binary = [i for i, p, *_ in U.cases() if p.get("binary_mask")]
    # (a standard frame merged back with weight 1.0 is the gray frame again: such a case cannot tell)
    assert set(bad) <= set(binary) and len(bad) >= len(binary) - 2 and len(bad) >= 5, (bad, binary)
    assert any(U.cases()[i][1].get("return_mask") for i in bad)                # "before everything else, return_mask included"


def test_swapping_the_binary_sign_convention_breaks_the_weighted_binary_cases():
    bad = _broken("swap_sign")
    # every binary case merges -- a non-zero weight, or a frame outside the band (weight = min(weight, -0.8)); never a mask or a gradient case
    want = [i for i, p, *_ in U.cases() if p.get("binary_mask") and not p.get("return_mask")]
    assert bad == want and len(bad) >= 6, (bad, want)
