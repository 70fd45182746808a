"""CPU: which weight file a DeOldify render reads, per arithmetic (vsdeoldify_amd/render.py choose_weight_file, tools/convert_weights.py --precision).
A .havc blob holds ONE arithmetic (its "precision" field): the package default is "precise", so a deployment that ships only converted blobs must be able
to convert and load precise ones, and a blob of the other mode must never be fed to a net (precise convs read three K segments per weight row)."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from vsdeoldify_amd.deoldify_net import DeoldifyGenerator
from vsdeoldify_amd.render import choose_weight_file
from vsdeoldify_amd.synth import synth_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _save_pth(path, sd):
    import torch
    torch.save({"model": {k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()}, "opt": {}}, path)


@pytest.fixture(scope="module")
def blobs(tmp_path_factory):
    """ColorizeArtistic_gen.pth (deep, seed 3) converted twice: without a switch in a process that has no HAVC_PRECISION (-> the package default), and with --precision fast"""
    d = tmp_path_factory.mktemp("weights")
    pth = d / "ColorizeArtistic_gen.pth"
    _save_pth(str(pth), synth_state_dict("deep", 3))
    env = {k: v for k, v in os.environ.items() if k != "HAVC_PRECISION"}
    conv = [sys.executable, os.path.join(ROOT, "tools", "convert_weights.py"), str(pth)]
    subprocess.check_call(conv + [str(d / "default.havc")], env=env)
    subprocess.check_call(conv + [str(d / "fast.havc"), "--precision", "fast"], env=env)
    return d, pth


def test_converter_writes_the_blob_of_the_requested_mode_and_load_keeps_it(blobs):
    d, _ = blobs
    assert DeoldifyGenerator.stored_precision(str(d / "default.havc")) == "precise"           # precision.resolve: no argument, no environment -> "precise"
    assert DeoldifyGenerator.stored_precision(str(d / "fast.havc")) == "fast"
    sd = synth_state_dict("deep", 3)
    for name, mode in (("default.havc", "precise"), ("fast.havc", "fast")):
        want, got = DeoldifyGenerator(sd, "deep", precision=mode), DeoldifyGenerator.load(str(d / name))
        assert got.precise == (mode == "precise") and got.arch == "deep" and got.blob == want.blob, name
        for S in (64, 80):
            (oa, ba, ia, outa, na), (ob, bb, ib, outb, nb) = want.plan(S), got.plan(S)
            assert na == nb and (ia, outa) == (ib, outb) and oa.tobytes() == ob.tobytes() and ba.tobytes() == bb.tobytes(), (name, S)
        # save -> load -> save keeps the field
        again = d / ("again_" + name)
        got.save(str(again))
        assert DeoldifyGenerator.stored_precision(str(again)) == mode
    with pytest.raises(subprocess.CalledProcessError):
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "convert_weights.py"), str(blobs[1]), "--precision", "double"], stderr=subprocess.DEVNULL)


def test_a_packed_file_is_used_only_for_its_own_mode(blobs, tmp_path):
    d, pth = blobs
    models = tmp_path / "models"
    models.mkdir()
    path, packed = str(models / "ColorizeArtistic_gen.pth"), str(models / "ColorizeArtistic_gen.havc")
    with pytest.raises(FileNotFoundError, match="DeOldify weights not found"):
        choose_weight_file(path, packed, "precise")
    for stored, other in (("precise", "fast"), ("fast", "precise")):
        blob = d / ("default.havc" if stored == "precise" else "fast.havc")
        # the blob alone: served in its own mode, an explanatory error in the other
        if os.path.exists(path):
            os.remove(path)
        with open(packed, "wb") as f:
            f.write(blob.read_bytes())
        assert choose_weight_file(path, packed, stored) == ("havc", packed)
        with pytest.raises(FileNotFoundError) as e:
            choose_weight_file(path, packed, other)
        msg = str(e.value)
        assert repr(stored) in msg and repr(other) in msg and packed in msg and "--precision " + other in msg, msg
        # blob + an OLDER .pth: the blob for its own mode, the .pth for the other one
        with open(path, "wb") as f:
            f.write(pth.read_bytes())
        old = time.time() - 100
        os.utime(path, (old, old))
        assert choose_weight_file(path, packed, stored) == ("havc", packed)
        assert choose_weight_file(path, packed, other) == ("pth", path)
        # a .pth NEWER than the blob wins in every mode (the blob is stale)
        os.utime(packed, (old - 100, old - 100))
        assert choose_weight_file(path, packed, stored) == ("pth", path) and choose_weight_file(path, packed, other) == ("pth", path)
    # a stray file under the blob's name next to a valid .pth: not a blob, the .pth is read; alone, it is reported for what it is
    with open(packed, "wb") as f:
        f.write(b"not a packed model")
    assert choose_weight_file(path, packed, "precise") == ("pth", path) and choose_weight_file(path, packed, "fast") == ("pth", path)
    os.remove(path)
    with pytest.raises(Exception) as e:
        choose_weight_file(path, packed, "precise")
    assert not isinstance(e.value, FileNotFoundError) or packed in str(e.value)
    # an empty .pth is no checkpoint
    os.remove(packed)
    open(path, "wb").close()
    with pytest.raises(FileNotFoundError):
        choose_weight_file(path, packed, "fast")
