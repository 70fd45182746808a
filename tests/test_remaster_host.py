"""CPU: the host side of DeepRemaster (vsdeoldify_amd/remaster_net.py, remaster_render.py, havc.HAVC_DeepRemaster): state-dict spec, plan emission, the
(3,3,3) weight repack, frame / still geometry, the reference window, the reference list, every refusal -- and that the plans of the other models are
the op lists they were before the new ops existed.  Geometry figures and the window trace come from executing the reference (tools/gen_golden_remaster.py,
tests/golden/remaster_render.npz; the literals below were printed by the reference's resize_for_inference / addMergin / get_ref_num)."""
import hashlib
import json
import os

import numpy as np
import pytest

from vsdeoldify_amd import _native as nat
from vsdeoldify_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def model():
    from vsdeoldify_amd.remaster_net import RemasterColorNet
    return RemasterColorNet(synth.synth_remaster_state_dict(5))


def test_synthetic_state_dict_matches_the_reference_spec_key_for_key():
    with open(os.path.join(GOLDEN, "spec_remaster.json")) as f:
        spec = json.load(f)
    sd = synth.synth_remaster_state_dict(5)
    assert list(sd) == list(spec)
    for k, shape in spec.items():
        assert list(np.asarray(sd[k]).shape) == shape, k
    assert sum(int(np.prod(s)) for k, s in spec.items() if not k.endswith("num_batches_tracked")) == 54303374      # NetworkC: 54.3 M weights and BatchNorm statistics
    for p in ("stattn1", "stattn2", "selfattn1", "selfattn2"):
        assert float(sd[p + ".gamma"][0]) != 0.0                     # the reference's initial 0 would hide the attention path
    assert synth.synth_remaster_state_dict(5) is sd and not np.array_equal(synth.synth_remaster_state_dict(6)["conv1.conv3d.weight"], sd["conv1.conv3d.weight"])


def test_plan_has_the_expected_ops_and_slices(model):
    P = model.plan(5, 64, 96, (40, 57), 6)
    t = [int(x) for x in P.ops["type"]]
    n_tconv, n_temporal, n_attn = 9 + 2 + 2 + 1 + 1 + 1 + 5 + 9 + 3, 8, 4            # TempConv / Upsample modules; (3,3,3) kernels (up1, conv2, up2-up4); attention modules
    assert t.count(nat.OP_CONV) == n_tconv + 1 + 3 * n_attn                          # + up4.1 + query / key / value convs
    assert t.count(nat.OP_ELU) == n_tconv
    assert t.count(nat.OP_TSTACK) == n_temporal
    assert t.count(nat.OP_SRCREF_ATTN) == n_attn and t.count(nat.OP_EW) == 4
    assert t.count(nat.OP_PREP_REMASTER) == 2 and t.count(nat.OP_REMASTER_OUT) == 1 and len(t) == 98
    assert P.encode == (0, 29) and P.colorize == (29, 69)
    enc = P.ops[:29]
    assert not np.isin(enc["type"], (nat.OP_TSTACK, nat.OP_SRCREF_ATTN)).any()      # the per-still slice has no op that looks at another frame
    att = P.ops[P.ops["type"] == nat.OP_SRCREF_ATTN]
    assert [int(a["kw"]) for a in att] == [6, 6, 0, 0]                               # stattn1 / stattn2 read the six ring slots, the self-attentions the window
    assert [(int(a["Ho"]), int(a["Wo"])) for a in att] == [(5, 8), (3, 4), (4, 6), (8, 12)] and all(int(a["Kc"]) % 64 == 0 for a in att)
    assert {k: v[1] for k, v in P.ring.items()} == {"k1": 40 * 64 * 2, "v1": 512 * 64 * 2, "k2": 12 * 64 * 2, "v2": 512 * 64 * 2}
    # without references both source-reference attentions go, and with them the per-still slice
    Q = model.plan(2, 32, 48)
    assert Q.encode == (0, 0) and len(Q.ops) == 65 and list(Q.ops["type"]).count(nat.OP_SRCREF_ATTN) == 2 and not Q.ring
    # the same weights whatever the size: offsets of a second plan point into the blob packed once
    assert int(P.ops["w_off"].max()) < len(model.blob)
    with pytest.raises(AssertionError):
        model.plan(2, 40, 48)                                                        # frames are multiples of 16


def test_temporal_weight_repack_equals_a_direct_3d_convolution():
    from vsdeoldify_amd.remaster_net import repack_temporal
    r = np.random.default_rng(0)
    T, C, Co, H, W = 4, 4, 3, 5, 6
    x = r.standard_normal((C, T, H, W))
    w = r.standard_normal((Co, C, 3, 3, 3))
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (1, 1)))
    direct = np.zeros((Co, T, H, W))
    for kt in range(3):
        for kh in range(3):
            for kw in range(3):
                direct += np.einsum("oc,cthw->othw", w[:, :, kt, kh, kw], xp[:, kt:kt + T, kh:kh + H, kw:kw + W])
    # HAVC_OP_TSTACK: channel kt * C + c of frame t = channel c of frame t + kt - 1, zeros outside the window; then a 2-D conv per frame
    w2 = repack_temporal(w)
    assert w2.shape == (Co, 3 * C, 3, 3)
    xt = np.pad(x, ((0, 0), (1, 1), (0, 0), (0, 0)))
    stacked = np.concatenate([xt[:, kt:kt + T] for kt in range(3)], 0)              # [3 C][T][H][W]
    sp = np.pad(stacked, ((0, 0), (0, 0), (1, 1), (1, 1)))
    got = np.zeros((Co, T, H, W))
    for kh in range(3):
        for kw in range(3):
            got += np.einsum("oc,cthw->othw", w2[:, :, kh, kw], sp[:, :, kh:kh + H, kw:kw + W])
    assert np.allclose(got, direct, rtol=0, atol=1e-12)
    assert repack_temporal(w[:, :, 1:2]).shape == (Co, C, 3, 3)                      # (1,3,3) kernels: the 2-D weight itself


def test_frame_and_still_geometry_on_odd_aspect_ratios():
    from vsdeoldify_amd import remaster_render as rr
    for (w, h, m), want in (((1920, 1080, 320), (576, 320)), ((720, 576, 320), (400, 320)), ((1000, 562, 320), (576, 320)), ((562, 1000, 320), (320, 576)),
                            ((640, 480, 480), (640, 480)), ((100, 100, 320), (320, 320)), ((1920, 804, 320), (768, 320))):
        assert rr.resize_for_inference_size(w, h, m) == want, (w, h, m)
    # (still size, ref_minedge) -> target size, box of the pasted content [x0, x1) x [y0, y1)
    for (w, h, m), tgt, box in (((568, 320, 256), (454, 256), (3, 451, 8, 248)), ((320, 568, 256), (256, 454), (8, 248, 3, 451)),
                                ((300, 300, 256), (256, 256), (0, 256, 0, 256)), ((1000, 562, 256), (455, 256), (3, 451, 8, 248)),
                                ((60, 36, 24), (40, 24), (4, 36, 4, 20))):
        assert rr.target_size(w, h, m) == tgt
        g = rr.margin_geometry(w, h, *tgt)
        got = (0, tgt[0], 0, tgt[1]) if g is None else (g[2], g[2] + g[0], g[3], g[3] + g[1])
        assert got == box, (w, h, m, g)
        assert g is None or (g[0] % 16 == 0 and g[1] % 16 == 0)
    assert [rr.normalize_buffer_size(n) for n in (20, 21, 3, 0, 7, 1000, 5)] == [20, 20, 4, 4, 6, 200, 4]


@pytest.mark.parametrize("length", [2, 5])
def test_reference_window_follows_the_reference_trace(length):
    from vsdeoldify_amd.remaster_render import ReferenceWindow
    fx = np.load(os.path.join(GOLDEN, "remaster_render.npz"))
    nums, N = [int(n) for n in fx["ref_nums"]], len(fx["clip"])
    w = ReferenceWindow(nums, int(fx["params"][2]))
    trace, moves = [], 0
    for n0 in range(0, N, length):
        moves += w.advance(min(n0 + length - 1, N - 1)) is not None
        trace.append(w.numbers())
        assert sorted(w.slots) == list(range(w.last_idx - w.size + 1, w.last_idx + 1))       # the ring holds a contiguous run of stills, in any slot order
    assert trace == fx[f"trace_L{length}"].tolist() and moves == 2
    # fewer stills than slots: the window is all of them and never moves
    w = ReferenceWindow([3, 9], 4)
    assert (w.size, w.half_idx, w.advance(100), w.numbers()) == (2, 0, None, [3, 9])


def test_reference_list_naming(tmp_path):
    from vsdeoldify_amd import remaster_render as rr
    assert [rr.get_ref_num(n) for n in ("ref_000012.png", "a_b_7.jpg", "/x/y_z/ref_0005.v2.png")] == [12, 7, 5]
    assert rr.get_ref_num("/home/a.b_c/pytest-1/refs_x/ref_000003.png") == 3        # dots and underscores in directory names are not part of the number
    for name in ("ref_000010.png", "ref_000002.jpg", "notes.txt", "ref_000007.PNG", "ref_000001.gif"):
        (tmp_path / name).write_bytes(b"x")
    (tmp_path / "ref_000099.png").mkdir()
    files, nums = rr.get_ref_list(str(tmp_path))
    assert [os.path.basename(f) for f in files] == ["ref_000002.jpg", "ref_000007.PNG", "ref_000010.png"] and nums == [2, 7, 10]
    r = rr.RemasterRender(ref_buffer_size=21)
    assert r.ref_buffer_size == 20
    r = rr.RemasterRender(ref_minedge=24)
    assert r.load_refs([np.zeros((36, 60, 3), np.uint8)], [5]) == 2 and r.window.nums == [5, 5] and (r.target_w, r.target_h) == (40, 24)


def test_precise_mode_is_refused_not_approximated(monkeypatch):
    from vsdeoldify_amd.remaster_net import RemasterColorNet
    from vsdeoldify_amd.remaster_render import RemasterRender
    monkeypatch.delenv("HAVC_PRECISION", raising=False)
    assert RemasterRender().ref_buffer_size == 20                                    # "fast" is this class's default whatever the package default
    with pytest.raises(NotImplementedError, match="precise"):
        RemasterRender(precision="precise")
    monkeypatch.setenv("HAVC_PRECISION", "precise")
    with pytest.raises(NotImplementedError, match="precise"):
        RemasterRender()
    assert RemasterRender(precision="fast").length == 2
    with pytest.raises(ValueError):
        RemasterRender(precision="exact")
    with pytest.raises(NotImplementedError):
        RemasterColorNet({}, precision="precise")


def test_deep_remaster_refusals_and_error_texts(tmp_path):
    from vsdeoldify_amd import HAVC_DeepRemaster
    from vsdeoldify_amd.havc import HAVCError
    clip = np.zeros((3, 48, 80, 3), np.uint8)
    empty = tmp_path / "empty"
    empty.mkdir()
    refs = tmp_path / "refs"
    refs.mkdir()
    (refs / "ref_000000.png").write_bytes(b"x")
    for kw, exc, text in ((dict(clip=None, ref_dir=str(refs)), HAVCError, "HAVC_DeepRemaster: this is not a clip"),
                          (dict(clip=[1, 2], ref_dir=str(refs)), HAVCError, "HAVC_DeepRemaster: this is not a clip"),
                          (dict(clip=clip), HAVCError, "HAVC_DeepRemaster: ref_dir is unset"),
                          (dict(clip=clip, ref_dir=str(tmp_path / "nope")), HAVCError, f"HAVC_DeepRemaster: '{tmp_path / 'nope'}' is not a valid directory"),
                          (dict(clip=clip, ref_dir=str(refs), length=1), HAVCError, "HAVC_DeepRemaster: length must be at least 2"),
                          (dict(clip=clip, ref_dir=str(empty)), HAVCError, f"HAVC_DeepRemaster: no reference frames found in {empty}"),
                          (dict(clip=clip, ref_dir=str(refs), mode=1), NotImplementedError, "mode = 1"),
                          (dict(clip=clip, ref_dir=str(refs), render_vivid=True), NotImplementedError, "render_vivid is vs_tweak"),
                          (dict(clip=np.zeros((3, 48, 80), np.uint8), ref_dir=str(refs)), HAVCError, "only RGB24 clips")):
        with pytest.raises(exc) as e:
            HAVC_DeepRemaster(**kw)
        assert text in str(e.value), (kw.keys(), str(e.value))
    import inspect
    sig = inspect.signature(HAVC_DeepRemaster)
    want = dict(length=2, render_vivid=False, ref_dir=None, ref_minedge=256, frame_mindim=320, ref_buffer_size=20, device_index=0, inference_mode=False, mode=0)
    pos = [p for p in sig.parameters.values() if p.kind == p.POSITIONAL_OR_KEYWORD]
    assert [p.name for p in pos] == ["clip"] + list(want) and {p.name: p.default for p in pos[1:]} == want


def test_deepex_still_refuses_the_remaster_model():
    from vsdeoldify_amd import HAVC_deepex
    with pytest.raises(NotImplementedError, match="ex_model 1-3"):
        HAVC_deepex(np.zeros((2, 32, 32, 3), np.uint8), sc_framedir="x", method=3, ex_model=2)


# sha1 of ops.tobytes() + bufs.tobytes() at the commit before the DeepRemaster ops were appended to the op enum: nothing was renumbered
PLAN_HASHES = {"zhang eccv16 fast": "0e2606ef8e3350b5aac73c4be5a7a77e2418f106", "zhang eccv16 precise": "4c0eba049fb60b4becf5652e07bc5948d93df7ea",
               "zhang siggraph17 fast": "3275c78b0c963da90e4296f76385f8e206d6d012", "zhang siggraph17 precise": "3a4be475bd35a20b711f8e4b321b3941598e4c04",
               "deoldify deep fast": "c869e8c5d34c16c3c6201d6151d5b7fc9a0fa5a3", "ddcolor small fast": "e1969a3ed4bf816a0bab366ae7a630b1cdea5c90",
               "colormnet": "547e6ad3558431d74c73c31946764c79bf5ad536"}


def _hash(ops, bufs):
    return hashlib.sha1(np.ascontiguousarray(ops).tobytes() + np.ascontiguousarray(bufs).tobytes()).hexdigest()


@pytest.mark.parametrize("name", list(PLAN_HASHES))
def test_plans_of_the_other_models_are_unchanged(name, monkeypatch):
    for v in ("HAVC_DD_FUSE_TAIL", "HAVC_DD_FUSE_SKIPNORM"):
        monkeypatch.delenv(v, raising=False)
    kind, *rest = name.split()
    if kind == "zhang":
        from vsdeoldify_amd.zhang_net import ZhangGenerator
        p = ZhangGenerator(synth.synth_zhang_state_dict(rest[0], 1), rest[0], precision=rest[1]).plan(64)
    elif kind == "deoldify":
        from vsdeoldify_amd.deoldify_net import DeoldifyGenerator
        p = DeoldifyGenerator(synth.synth_state_dict("deep", 1), "deep", precision="fast").plan(64)
    elif kind == "ddcolor":
        from vsdeoldify_amd.ddcolor_net import DDColorGenerator
        small = dict(depths=(1, 1, 2, 1), dec_layers=3)
        p = DDColorGenerator(synth.synth_ddcolor_state_dict(1, **small), depths=small["depths"], dec_layers=3).plan(64)
    else:
        from vsdeoldify_amd.colormnet_net import ColorMNetPlan
        p = ColorMNetPlan(synth.synth_colormnet_state_dict(1)).plan(112, 112)
    assert _hash(p[0], p[1]) == PLAN_HASHES[name]
