"""CPU (-m "not gpu"): HAVC_deepex's argument errors (the reference's, in its order: vsdeoldify/__init__.py:1540-1590) and refusals, all before any GPU
context exists; its argument list and defaults; DeepExColorMNet's and stabilize_np's new arguments are optional."""
import inspect

import numpy as np
import pytest

from vsdeoldify_amd import havc
from vsdeoldify_amd import scdetect as SD


def _scenes(n=3, threshold=0.10, frequency=0):
    return SD.SceneInfo(np.ones(n, np.int8), np.zeros(n, np.int8), np.full(n, 0.5), np.zeros(n), threshold, frequency)


def test_argument_errors_and_refusals_in_the_reference_order(monkeypatch):
    def no_gpu(*a, **k):
        raise AssertionError("GPU work was started")
    import vsdeoldify_amd.colormnet_render as cr
    monkeypatch.setattr(havc, "get_context", no_gpu)
    monkeypatch.setattr(cr, "DeepExColorMNet", no_gpu)
    c = np.zeros((3, 8, 8, 3), np.uint8)
    sc = _scenes()
    E, R = havc.HAVCError, NotImplementedError
    cases = [
        (dict(clip=None, clip_ref=c), E, "not a clip"),
        (dict(only_ref_frames=True, method=1), E, "only_ref_frames is enabled but sc_framedir is unset"),            # first check wins over method != 0
        (dict(only_ref_frames=True, sc_framedir="d", method=1), E, r"only_ref_frames is enabled but method != 0"),
        (dict(method=1), E, "method != 0 but sc_framedir is unset"),
        (dict(method=9), E, "method != 0 but sc_framedir is unset"),                                                   # ... and over the range check
        (dict(method=3, sc_framedir="d"), E, r"method in \(3, 4\) but clip_ref is set"),
        (dict(clip_ref=None), E, "clip_ref is unset"),
        (dict(clip_ref=[1]), E, "not a clip: clip_ref"),
        (dict(method=7, sc_framedir="d"), E, r"method must be in range \[0-6\]"),
        (dict(ref_merge=6), E, r"ref_merge must be in range \[0-5\]"),
        (dict(ref_merge=2, method=2, sc_framedir="d"), E, r"method must be in \(0, 1, 5\)"),
        (dict(scenes=None), E, "sc_threshold and sc_frequency are not set"),
        (dict(scenes=_scenes(3, 0, 0)), E, "sc_threshold and sc_frequency are not set"),
        (dict(scenes=_scenes(3, 0.1, 1), only_ref_frames=True, sc_framedir="d"), E, "sc_frequency == 1"),
        (dict(ref_merge=2), E, "ref_merge > 0 but sc_frequency != 1"),
        (dict(ex_model=2), E, "DeepRemaster cannot be used with methods: 0, 1, 2"),
        (dict(ex_model=1), R, "Deep-Exemplar"), (dict(ex_model=3, ref_merge=2), R, "DESIGN.md"),
        (dict(ex_model=2, method=5, sc_framedir="d"), R, "DeepRemaster"),
        (dict(ex_model=4), E, "unknown exemplar model id: 4"),
        (dict(method=1, sc_framedir="d"), R, "directory or a video"), (dict(method=5, sc_framedir="d"), R, "HAVC_restore_video"),
        (dict(method=4, sc_framedir="d", clip_ref=None), R, "directory or a video"),
        (dict(sc_framedir="d"), R, "write the reference frames to files"),
        (dict(sc_framedir="d", only_ref_frames=True), R, "write the reference frames to files"),
        (dict(encode_mode=2), R, "encode_mode = 2"), (dict(encode_mode=3), E, "encode_mode"),
        (dict(bogus=1), TypeError, "bogus"),
        (dict(render_speed="warp"), E, "unknown render_speed"), (dict(render_speed=3), E, "must be strings"), (dict(colormap=None), E, "must be strings"),
        (dict(bogus=1, method=9), TypeError, "bogus"),
        (dict(colormap="purple->green"), E, "ColorMap choice is invalid"),
        (dict(clip_ref=c[:2]), E, "must have the frames and the size"),
        (dict(scenes=_scenes(5)), E, "5 entries for a clip of 3 frames"),
    ]
    for kw, exc, text in cases:
        args = dict(clip=c, clip_ref=c, scenes=sc)
        args.update(kw)
        with pytest.raises(exc, match=text):
            havc.HAVC_deepex(**args)


def test_argument_list_and_optional_extensions():
    sig = inspect.signature(havc.HAVC_deepex)
    pos = [(k, v.default) for k, v in sig.parameters.items() if v.kind is v.POSITIONAL_OR_KEYWORD]
    assert pos == [("clip", None), ("clip_ref", None), ("method", 0), ("render_speed", "medium"), ("render_vivid", True), ("ref_merge", 0),
                   ("sc_framedir", None), ("ref_norm", False), ("only_ref_frames", False), ("dark", False), ("dark_p", (0.2, 0.8)), ("smooth", False),
                   ("smooth_p", (0.3, 0.7, 0.9, 0.0, "none")), ("colormap", "none"), ("ref_weight", None), ("ref_thresh", None), ("ref_freq", None),
                   ("ex_model", 0), ("encode_mode", 0), ("max_memory_frames", 0), ("torch_dir", None)]          # __init__.py:1421-1426
    assert sig.parameters["scenes"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["scenes"].default is None
    assert havc._REFMERGE_WEIGHT == [0.0, 0.3, 0.4, 0.5, 0.6, 0.7]
    from vsdeoldify_amd.colormnet_render import DeepExColorMNet
    from vsdeoldify_amd.stabilizer import stabilize_np
    p = inspect.signature(DeepExColorMNet.colorize_frame).parameters
    assert list(p)[:6] == ["self", "frame", "ref", "_small", "_slot", "_next_plain"] and p["ref_small"].default is None and p["blend"].default is None
    assert inspect.signature(stabilize_np).parameters["order"].default == ("dark", "smooth", "colormap")
