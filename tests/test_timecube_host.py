"""CPU: the host half of HAVC_TimeCube (vsdeoldify_amd/timecube.py) -- the .cube reader with every refusal, the axis tables against float64, the plan against
every record of tests/golden/timecube.npz (the reference's own Python, executed by tools/gen_golden_timecube.py), the public signatures, and the identity
property of the numpy definition (tests/timecube_util.py) on 2 359 296 inputs."""
import inspect
import json
import os

import numpy as np
import pytest

from tests import timecube_util as U
from vsdeoldify_amd import havc
from vsdeoldify_amd import timecube as TC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "timecube.npz")
ROWS8 = "\n".join(f"{r} {g} {b}" for b in (0, 1) for g in (0, 1) for r in (0, 1))


def _records():
    return json.loads(str(np.load(GOLDEN)["records"]))


# ---- the reader --------------------------------------------------------------------------------------------------------------------------------------------
def test_reader_takes_comments_title_domains_and_crlf(tmp_path):
    cube = U.random_cube(3, domain_min=(0.1, 0.0, -0.5), domain_max=(0.9, 1.0, 2.0))
    for line_end in ("\n", "\r\n"):
        path = U.write_cube(tmp_path / f"a{len(line_end)}.cube", cube, line_end=line_end)
        got = TC.parse_cube(path)
        assert got.size == 3 and got.title == "random 0" and got.domain_min == (0.1, 0.0, -0.5) and got.domain_max == (0.9, 1.0, 2.0)
        assert got.table.dtype == np.float32 and got.table.shape == (3, 3, 3, 3) and np.array_equal(got.table, cube.table)
        assert np.array_equal(TC.parse_cube(U.cube_text(cube, line_end=line_end)).table, cube.table)      # the text itself
        assert np.array_equal(TC.parse_cube(os.fsencode(path)).table, cube.table) and np.array_equal(TC.parse_cube(tmp_path / f"a{len(line_end)}.cube").table, cube.table)
    got = TC.parse_cube("# c\n\nTITLE \"t t\"\n  LUT_3D_SIZE 2\n# another\nLUT_3D_INPUT_RANGE 0.25 4\n\n" + ROWS8 + "\n\n")
    assert got.size == 2 and got.title == "t t" and got.domain_min == (0.25,) * 3 and got.domain_max == (4.0,) * 3
    assert got.table[1, 0, 1].tolist() == [1.0, 0.0, 1.0]                                                  # red is the fastest index, blue the slowest
    assert TC.parse_cube("LUT_3D_SIZE 2\n" + ROWS8 + "\n").domain_max == (1.0, 1.0, 1.0)


@pytest.mark.parametrize("text,line,why", [
    ("LUT_1D_SIZE 4\n0 0 0\n", 1, "LUT_1D_SIZE"),
    ("TITLE \"x\"\n" + ROWS8 + "\n", 2, "in front of LUT_3D_SIZE"),
    ("# only a comment\nTITLE \"x\"\n", 2, "no LUT_3D_SIZE"),
    ("LUT_3D_SIZE 2\nLUT_3D_SIZE 2\n" + ROWS8 + "\n", 2, "second LUT_3D_SIZE"),
    ("LUT_3D_SIZE 1\n0 0 0\n", 1, "2..256"),
    ("LUT_3D_SIZE 257\n", 1, "2..256"),
    ("LUT_3D_SIZE 2.5\n", 1, "2..256"),
    ("LUT_3D_SIZE 2\n" + ROWS8 + "\n0 0 0\n", 10, "more than 8 rows"),
    ("LUT_3D_SIZE 2\n" + ROWS8.rsplit("\n", 1)[0] + "\n", 8, "7 rows"),
    ("LUT_3D_SIZE 2\n0 0\n", 2, "3 numbers"),
    ("LUT_3D_SIZE 2\n0 0 0 0\n", 2, "3 numbers"),
    ("LUT_3D_SIZE 2\n0 x 0\n", 2, "3 numbers"),
    ("LUT_3D_SIZE 2\n0 inf 0\n", 2, "not finite"),
    ("LUT_3D_SIZE 2\nnan 0 0\n", 2, "not finite"),
    ("LUT_3D_SIZE 2\n0 0 1e39\n" + ROWS8.split("\n", 1)[1] + "\n", 9, "not finite in float32"),
    ("LUT_3D_SIZE 2\nDOMAIN_MIN 0 0 0\nDOMAIN_MAX 1 0 1\n" + ROWS8 + "\n", 11, "DOMAIN_MAX"),
    ("LUT_3D_SIZE 2\nDOMAIN_MIN 0 0.5 0\nDOMAIN_MAX 1 0.25 1\n" + ROWS8 + "\n", 11, "DOMAIN_MAX"),
    ("LUT_3D_SIZE 2\nDOMAIN_MIN 0 0\n" + ROWS8 + "\n", 2, "DOMAIN_MIN needs 3 numbers"),
    ("LUT_3D_SIZE 2\nLUT_3D_INPUT_RANGE 1 1\n" + ROWS8 + "\n", 10, "DOMAIN_MAX"),
    ("LUT_3D_SIZE 2\nLUT_IN_VIDEO_RANGE\n" + ROWS8 + "\n", 2, "unknown keyword LUT_IN_VIDEO_RANGE"),
])
def test_reader_refuses_with_file_and_line(tmp_path, text, line, why):
    with pytest.raises(havc.HAVCError) as e:
        TC.parse_cube(text)
    assert f"<text>, line {line}: " in str(e.value) and why in str(e.value), str(e.value)
    path = tmp_path / "bad.cube"
    path.write_text(text)
    with pytest.raises(havc.HAVCError) as e:
        TC.parse_cube(str(path))
    assert f"{path}, line {line}: " in str(e.value) and why in str(e.value), str(e.value)


# ---- the axis tables ---------------------------------------------------------------------------------------------------------------------------------------
def _axis_bound(size, dmin, dmax):
    """What float32 can hold of t = (s / 255 - dmin) / (dmax - dmin) * (N - 1), worked out, not measured: every one of the four operations and the two
    constants rounds by at most 2^-24 relative; the errors of x and dmin in front of the subtraction are scaled by (N - 1) / (dmax - dmin) and the later ones by
    t <= N - 1: at most 2^-24 * (N - 1) * ((1 + |dmin| + max |x - dmin|) / span + 4), x in [0, 1].  On the default domain that is 7 * 2^-24 * (N - 1): below
    1e-6 for N = 2 and 3 and above it from N = 5 on, as it must be: half an ulp of t itself is 9.5e-7 at t = 16."""
    span = dmax - dmin
    return 2.0 ** -24 * (size - 1) * ((1.0 + abs(dmin) + max(abs(dmin), abs(1.0 - dmin))) / span + 4.0)


@pytest.mark.parametrize("dmin,dmax", [((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)), ((0.1, 0.1, 0.1), (0.9, 0.9, 0.9))])
@pytest.mark.parametrize("size", [2, 3, 5, 17, 33, 65, 256])
def test_axis_tables_against_float64(size, dmin, dmax):
    """cells EQUAL at every size; fractions within 1e-6 wherever float32 can hold that (see _axis_bound), and within float32's own bound at the larger sizes"""
    cube = TC.Cube(size, dmin, dmax, None, "")
    idx, frac = TC.axis_tables(cube)
    assert idx.dtype == np.int32 and frac.dtype == np.float32 and idx.shape == frac.shape == (3, 256)
    assert idx.min() >= 0 and idx.max() <= size - 2 and frac.min() >= 0 and frac.max() <= 1
    s = np.arange(256, dtype=np.float64)
    for c in range(3):
        t = np.clip((s / 255 - dmin[c]) / (dmax[c] - dmin[c]) * (size - 1), 0, size - 1)
        want = np.minimum(np.floor(t), size - 2)
        assert np.array_equal(idx[c], want.astype(np.int32)), (size, c)
        err = float(np.abs(frac[c] - (t - want)).max())
        bound = _axis_bound(size, dmin[c], dmax[c])
        print(f"axis tables N = {size}, domain {dmin[c]} .. {dmax[c]}: largest fraction error {err:.3e}, float32 bound {bound:.3e}")
        assert err <= (1e-6 if bound <= 1e-6 else bound), (size, c, err, bound)


# ---- the plan against the reference ------------------------------------------------------------------------------------------------------------------------
def test_plan_against_every_golden_record():
    records = _records()
    assert len(records) == 51 and {r["args"].get("lut_effect", 0) for r in records} == set(range(12))
    for r in records:
        a = r["args"]
        plan = TC.timecube_plan(a.get("strength", 1.0), a.get("lut_effect", 0), a.get("factors"), "LUTDIR")
        calls = []
        if not plan["identity"]:
            rel = os.path.relpath(plan["file"], "LUTDIR").replace(os.sep, "/")
            calls.append(["timecube.Cube", dict(clip="source", dir=os.path.dirname(rel), file=os.path.basename(rel))])
            calls.append(["vs_tweak", dict(clip="lut", **plan["tweak"])])
            if plan["merge"] is not None and plan["merge"][0] == "combine_models":
                kw = plan["merge"][1]
                calls.append(["vs_combine_models", dict(clip_a="source", clip_b="tweaked", method=kw["method"], clipb_weight=kw["w"], CMC_p=kw["cmc_p"])])
            elif plan["merge"] is not None:
                calls.append(["std.Merge", dict(clipa="source", clipb="tweaked", weight=plan["merge"][1])])
        assert calls == r["calls"], (a, calls, r["calls"])
        assert r["result"] == ("source" if plan["identity"] else "tweaked" if plan["merge"] is None else "merged")


def test_plan_refusals_and_cube_override(tmp_path, monkeypatch):
    for kw, why in ((dict(lut_effect=12), "lut_effect = 12"), (dict(lut_effect=-1), "lut_effect = -1"), (dict(lut_effect=2.0), "lut_effect"),
                    (dict(strength=1.5), "strength = 1.5"), (dict(strength=-0.1), "strength = -0.1")):
        with pytest.raises(havc.HAVCError) as e:
            TC.timecube_plan(**{"lut_dir": "d", **kw})
        assert why in str(e.value)
    with pytest.raises(havc.HAVCError) as e:
        TC.timecube_plan(0.5, 2)
    assert "HAVC_LUT_DIR" in str(e.value) and "lut_dir" in str(e.value) and "cube=" in str(e.value)
    assert TC.timecube_plan(0, 99)["identity"]                                                            # strength 0 looks at nothing else
    cube = U.identity_cube(2)
    plan = TC.timecube_plan(0.5, 8, None, None, cube)
    assert plan["file"] is None and plan["tweak"]["sat"] == 0.40 and plan["merge"][0] == "combine_models" and TC.load_cube(plan, cube) is cube
    assert TC.timecube_plan(1, 40, None, None, cube)["tweak"] == dict(hue=0, sat=1, bright=0, cont=1, gamma=1)      # no effect: the reference's match falls through
    # the public function: a directory without the file, no directory at all, the environment variable
    clip = np.zeros((1, 4, 4, 3), np.uint8)
    monkeypatch.delenv("HAVC_LUT_DIR", raising=False)
    with pytest.raises(havc.HAVCError) as e:
        havc.HAVC_TimeCube(clip, 1.0, 2)
    assert "HAVC_LUT_DIR" in str(e.value)
    missing = os.path.normpath(os.path.join(str(tmp_path), "color", "Presetpro - Exploration.cube"))
    for how in ("argument", "environment"):
        if how == "environment":
            monkeypatch.setenv("HAVC_LUT_DIR", str(tmp_path))
        with pytest.raises(havc.HAVCError) as e:
            havc.HAVC_TimeCube(clip, 1.0, 2, **(dict(lut_dir=str(tmp_path)) if how == "argument" else {}))
        assert missing in str(e.value) and "not found" in str(e.value), (how, str(e.value))
    with pytest.raises(havc.HAVCError):
        havc.HAVC_TimeCube(clip, 1.0, 0, cube=str(tmp_path / "nowhere.cube"))
    with pytest.raises(havc.HAVCError) as e:                                                              # an odd frame with a tweak: the existing refusal
        havc.HAVC_TimeCube(np.zeros((1, 3, 5, 3), np.uint8), 1.0, 0, cube=cube)
    assert "must be even" in str(e.value)
    with pytest.raises(havc.HAVCError):
        havc.HAVC_TimeCube("clip.mp4")
    assert havc.HAVC_TimeCube(clip, 0, 5) is clip                                                         # strength 0: before any file is looked for


def test_signatures_start_with_the_reference_argument_lists():
    sig = inspect.signature(havc.HAVC_TimeCube)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[:4]] == [("clip", inspect.Parameter.empty), ("strength", 1.0), ("lut_effect", 0),
                                                                               ("factors", None)]
    assert [p.name for p in sig.parameters.values() if p.kind is inspect.Parameter.KEYWORD_ONLY] == ["lut_dir", "cube", "device_index"]
    sig = inspect.signature(havc.HAVC_clip_overlay)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[:9]] == [
        ("base", inspect.Parameter.empty), ("overlay", inspect.Parameter.empty), ("x", 0), ("y", 0), ("mask", None), ("opacity", 1.0), ("mode", "normal"),
        ("planes", None), ("mask_first_plane", True)]
    assert [p.name for p in sig.parameters.values() if p.kind is inspect.Parameter.KEYWORD_ONLY] == ["device_index"]
    import vsdeoldify_amd
    assert vsdeoldify_amd.HAVC_TimeCube is havc.HAVC_TimeCube and vsdeoldify_amd.HAVC_clip_overlay is havc.HAVC_clip_overlay


# ---- the definition ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rotation", [0, 2])
def test_identity_cube_returns_its_input_on_the_sweep(rotation):
    frame = U.sweep_frame(rotation)
    assert frame.shape == (256, 9216, 3) and frame.shape[0] * frame.shape[1] == U.SWEEP_INPUTS == 2359296
    assert len(np.unique(frame.reshape(-1, 3), axis=0)) == U.SWEEP_INPUTS
    for size in (2, 3, 17, 33, 65):
        assert np.array_equal(U.lut3d(frame, U.identity_cube(size)), frame), size


def test_definition_by_hand_on_a_two_point_cube():
    table = np.zeros((2, 2, 2, 3), np.float32)
    table[..., 0] = np.array([0.0, 1.0], np.float32)[None, None, :]                                       # red out = red in
    table[..., 1] = np.array([1.0, 0.0], np.float32)[None, :, None]                                       # green out = 1 - green in
    table[..., 2] = np.array([-1.0, 2.0], np.float32)[:, None, None]                                      # blue out = 3 blue in - 1, clamped
    cube = TC.Cube(2, (0.0,) * 3, (1.0,) * 3, table, "")
    px = np.array([[0, 0, 0], [255, 255, 255], [51, 102, 85], [10, 20, 170], [200, 1, 84]], np.uint8)
    want = [[0, 255, 0], [255, 0, 255], [51, 153, 0], [10, 235, 255], [200, 254, 0]]
    assert U.lut3d(px, cube).tolist() == want
