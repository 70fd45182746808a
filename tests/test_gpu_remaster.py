"""GPU: the DeepRemaster colour network (vsdeoldify_amd/remaster_net.py, csrc/remaster.hip) against tests/golden/remaster_net.npz, which holds the reference's
own NetworkC executed on the CPU with the seeded synthetic weights (tools/gen_golden_remaster.py).

Shapes (the smallest at which each mechanism can still go wrong):
  t2     T = 2, 32 x 48, 2 references of 24 x 33: every frame is a temporal boundary; a 3 x 5 key grid = 15 keys per still, under one 64-key tile (mask)
  t3     T = 3, 48 x 32, 5 references of 33 x 24: one interior frame; 75 keys in all
  t5     T = 5, 64 x 96, 6 references of 40 x 57: 240 keys; selfattn2 has 480 tokens = several 64-query blocks
  t1     one frame: doubled to T = 2, one frame returned        noref   x_refs = None
  t3adv  t3 with references 1-4: the window a 4-slot ring holds after one advance

Limits come from the fixture, not from the code under test: next to the fp32 run the fixture holds the "fp16 floor", the reference with the input and weight of
every Conv3d rounded to fp16.  For every tap and for `ab` the GPU's max-abs and mean-abs error against the fp32 run may be at most 3 x the floor's (the factor
covers what the floor does not emulate: P rounded to fp16, another accumulation order, __expf, the fp16 store of every activation).  The u8 frames are compared
with CIEDE2000: mean and p99 at most 3 x the floor run's.  HAVC_REMASTER_ACCURACY_OUT=<file> writes the measured figures (profiles/remaster_accuracy.txt)."""
import os

import numpy as np
import pytest

from oracle import imaging
from vsdeoldify_amd.synth import synth_remaster_state_dict

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TAPS = ("down1", "stattn1", "flat", "stattn2", "selfattn1", "up1", "selfattn2", "conv2", "ab")
FACTOR = 3.0
REPORT = []


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "remaster_net.npz"))


@pytest.fixture(scope="module")
def model(fx):
    from vsdeoldify_amd.remaster_net import RemasterColorNet
    return RemasterColorNet(synth_remaster_state_dict(int(fx["seed"])))


@pytest.fixture(scope="module")
def weights(ctx, model):
    from vsdeoldify_amd import _native as nat
    w = nat.Weights(ctx, model.blob)
    yield w
    w.close()
    out = os.environ.get("HAVC_REMASTER_ACCURACY_OUT")
    if out and REPORT:
        with open(out, "w") as f:
            f.write("DeepRemaster colour network on the GPU against the reference's fp32 run (tests/test_gpu_remaster.py; tests/golden/remaster_net.npz).\n"
                    "error = |GPU - fp32 reference| on the fixture's sub-sample; floor = the reference with fp16 conv operands against the same run; limit = 3 x floor.\n\n")
            f.write("\n".join(REPORT) + "\n")


def session(ctx, model, weights, frames, refs, slots=None):
    from vsdeoldify_amd.remaster_net import RemasterSession
    T, H, W = max(len(frames), 2), frames.shape[1], frames.shape[2]
    if refs is None:
        return RemasterSession(ctx, model, T, H, W, weights=weights)
    s = RemasterSession(ctx, model, T, H, W, refs.shape[1:3], len(refs), weights=weights)
    for i, r in enumerate(refs):
        s.encode_reference(i if slots is None else slots[i], np.ascontiguousarray(r))
    return s


def check(fx, key, s, rgb, label=None, taps=TAPS):
    """every tap the fixture holds for `key` and the u8 frames, each within FACTOR x the floor's error; figures go to REPORT before anything is asserted"""
    label, bad = label or key, []
    n = max(len(rgb), 2)
    for t in taps:
        if f"{key}_{t}" not in fx.files:
            continue
        k, ref, floor = int(fx[f"{key}_{t}_stride"]), fx[f"{key}_{t}"].astype(np.float64), fx[f"{key}_{t}_floor"].astype(np.float64)
        got_full = s.tap(t, n)
        assert got_full.shape == tuple(fx[f"{key}_{t}_shape"]), (t, got_full.shape)
        got = got_full.reshape(-1)[::k].astype(np.float64)
        e, f = np.abs(got - ref), np.abs(floor - ref)
        line = f"{label:8s} {t:10s} max {e.max():.3e} (floor {f.max():.3e}, x{e.max() / f.max():.2f})   mean {e.mean():.3e} (floor {f.mean():.3e}, x{e.mean() / f.mean():.2f})"
        REPORT.append(line)
        print(line)
        if not (e.max() <= FACTOR * f.max() and e.mean() <= FACTOR * f.mean()):
            bad.append(line)
    de = imaging.delta_e00_images(rgb, fx[key + "_rgb"])
    fl, st = fx[key + "_rgb_floor_de"], fx[key + "_rgb_step_de"]
    lim = [FACTOR * (fl[i] if fl[i] > 0 else st[i]) for i in (0, 1)]
    mean, p99 = float(de.mean()), float(np.percentile(de, 99))
    line = f"{label:8s} u8 dE00    mean {mean:.4f} (limit {lim[0]:.4f})   p99 {p99:.4f} (limit {lim[1]:.4f})   max {de.max():.3f}"
    REPORT.append(line)
    print(line)
    if not (mean <= lim[0] and p99 <= lim[1]):
        bad.append(line)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("key", ["t2", "t3", "t5"])
def test_network_with_references_matches_the_reference_within_three_times_the_fp16_floor(ctx, fx, model, weights, key):
    frames, refs = fx[key + "_frames"], fx[key + "_refs"]
    s = session(ctx, model, weights, frames, refs)
    rgb = s.colorize(frames)
    check(fx, key, s, rgb)
    s.close()


def test_network_without_references_skips_both_source_reference_attentions(ctx, fx, model, weights):
    frames = fx["noref_frames"]
    s = session(ctx, model, weights, frames, None)
    assert "stattn1" not in s.plan.taps and "stattn2" not in s.plan.taps
    rgb = s.colorize(frames)
    check(fx, "noref", s, rgb)
    s.close()


def test_single_frame_is_doubled_and_one_frame_comes_back(ctx, fx, model, weights):
    frames, refs = fx["t2_frames"][:1], fx["t2_refs"]
    s = session(ctx, model, weights, frames, refs)
    rgb = s.colorize(frames)
    assert rgb.shape == (1,) + frames.shape[1:]
    check(fx, "t1", s, rgb)
    s.close()


def test_ring_slot_order_does_not_matter(ctx, fx, model, weights):
    """the same stills in rotated slots: another key order for the online softmax, the same result within the limits"""
    frames, refs = fx["t3_frames"], fx["t3_refs"]
    n = len(refs)
    s = session(ctx, model, weights, frames, refs, slots=[(i + 2) % n for i in range(n)])
    rgb = s.colorize(frames)
    check(fx, "t3", s, rgb, label="t3 rot")
    s.close()


def test_ring_advance_equals_a_fresh_window(ctx, fx, model, weights):
    """a 4-slot ring on stills 0-3, then still 4 over the oldest slot: the window 1-4, which the fixture holds as a render of its own; a fresh session on that
    window gives the same frames up to the key order"""
    frames, refs = fx["t3_frames"], fx["t3_refs"]
    s = session(ctx, model, weights, frames, refs[:4])
    first = s.colorize(frames)
    s.encode_reference(0, np.ascontiguousarray(refs[4]))
    rgb = s.colorize(frames)
    assert not np.array_equal(rgb, first)                       # the new still is seen
    check(fx, "t3adv", s, rgb, label="t3 adv")
    ab = s.tap("ab", 3)
    s.close()
    s2 = session(ctx, model, weights, frames, refs[1:5])
    rgb2 = s2.colorize(frames)
    check(fx, "t3adv", s2, rgb2, label="t3 fresh")
    assert np.abs(ab - s2.tap("ab", 3)).max() <= FACTOR * np.abs(fx["t3adv_ab_floor"] - fx["t3adv_ab"]).max()
    s2.close()


# ---- RemasterRender and HAVC_DeepRemaster on the 9-frame fixture (tests/golden/remaster_render.npz: the reference's RemasterEngine on the CPU) ----
@pytest.fixture(scope="module")
def rfx():
    return np.load(os.path.join(GOLDEN, "remaster_render.npz"))


@pytest.fixture(scope="module")
def ref_dir(rfx, tmp_path_factory):
    from PIL import Image
    d = tmp_path_factory.mktemp("remaster_refs")
    for img, n in zip(rfx["refs"], rfx["ref_nums"]):
        Image.fromarray(img).save(os.path.join(str(d), "ref_%06d.png" % int(n)))
    return str(d)


def check_u8(rfx, name, got, label):
    de = imaging.delta_e00_images(got, rfx[name])
    fl, st = rfx[name + "_floor_de"], rfx[name + "_step_de"]
    lim = [FACTOR * (fl[i] if fl[i] > 0 else st[i]) for i in (0, 1)]
    mean, p99 = float(de.mean()), float(np.percentile(de, 99))
    line = f"{label:18s} u8 dE00 mean {mean:.4f} (limit {lim[0]:.4f})   p99 {p99:.4f} (limit {lim[1]:.4f})   max {de.max():.3f}"
    REPORT.append(line)
    print(line)
    assert mean <= lim[0] and p99 <= lim[1], line


@pytest.mark.parametrize("length", [2, 5])
def test_render_follows_the_reference_engine_over_a_clip(ctx, rfx, model, weights, ref_dir, length):
    """batches of `length` frames (the last one shorter: one frame at length 2), stills from a directory, the window advancing twice"""
    from vsdeoldify_amd.remaster_render import RemasterRender
    small, N = rfx["small"], len(rfx["small"])
    r = RemasterRender(ref_minedge=int(rfx["params"][1]), ref_buffer_size=int(rfx["params"][2]), length=length, model=model)
    assert r.load_ref_dir(ref_dir) == len(rfx["ref_nums"]) and (r.target_w, r.target_h) == tuple(rfx["target_wh"])
    outs, trace = [], []
    for n0 in range(0, N, length):
        outs.append(r.process_frames(small[n0:n0 + length], last_frame_idx=min(n0 + length - 1, N - 1)))
        trace.append(r.window.numbers())
    r.close()
    assert trace == rfx[f"trace_L{length}"].tolist()
    check_u8(rfx, f"out_L{length}", np.concatenate(outs), f"render length {length}")


def test_deep_remaster_end_to_end_host_and_device_give_the_same_bytes(ctx, rfx, model, ref_dir):
    from vsdeoldify_amd import DeviceImage, HAVC_DeepRemaster
    kw = dict(length=2, ref_dir=ref_dir, ref_minedge=int(rfx["params"][1]), frame_mindim=int(rfx["params"][0]), ref_buffer_size=int(rfx["params"][2]), model=model)
    clip = rfx["clip"]
    out = HAVC_DeepRemaster(clip, **kw)
    assert out.shape == clip.shape and out.dtype == np.uint8
    check_u8(rfx, "final_L2", out, "HAVC_DeepRemaster")
    dev = HAVC_DeepRemaster(DeviceImage.from_numpy(ctx, clip), **kw)
    assert isinstance(dev, DeviceImage) and np.array_equal(dev.numpy(), out)
    one = HAVC_DeepRemaster(clip[0], **kw)                       # a single frame in, a single frame out
    assert one.shape == clip.shape[1:]
