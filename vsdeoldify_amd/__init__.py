"""vsdeoldify_amd — MI355X-native per-frame colorization inference behind the HAVC (vs-deoldify) API.

Only the hot path lives here: the DeOldify generators, the Zhang colorizers, DDColor and the per-pixel
merge / tweak filters, as hand-written HIP kernels for gfx950 behind a C ABI (include/havc_mi355.h, lib/libhavc_mi355.so),
plus the thin Python mirror of the reference's adapter classes.  No CPU fallback: see _native.py.
"""
__version__ = "0.2.0"

from ._native import HavcOutOfMemory, NativeLibraryError  # noqa: F401


def __getattr__(name):
    if name == "ModelImageRender":
        from .render import ModelImageRender
        return ModelImageRender
    if name == "ModelColorization":
        from .colorization import ModelColorization
        return ModelColorization
    if name == "DDColorRender":
        from .ddcolor import DDColorRender
        return DDColorRender
    if name in ("HAVC_colorizer", "HAVC_merge", "HAVC_ddeoldify", "ddeoldify", "HAVC_stabilizer", "HAVC_stabilizer_scenes", "HAVCFrameColorizer", "HAVC_clip_slice",
                "HAVC_clip_reconstruct", "ClipTiles", "tiled_preset_params", "HAVC_SceneDetect", "HAVC_deepex", "HAVC_auto_levels", "HAVC_bw_tune",
                "HAVC_DeepRemaster", "HAVC_extract_reference_frames", "HAVC_export_reference_frames", "HAVC_export_list_frames",
                "HAVC_recover_clip_color", "HAVC_restore_video", "HAVC_retinex", "HAVC_SceneDetectEdges", "HAVC_tweak", "HAVC_adjust_rgb", "HAVC_rgb_denoise",
                "HAVC_TimeCube", "HAVC_clip_overlay"):
        from . import havc
        return getattr(havc, name)
    if name in ("VideoClip", "ClipInfo", "DevicePlane", "convert_format_RGB24", "restore_format"):
        from . import vformat
        return getattr(vformat, name)
    if name in ("clip_delta_e", "DeltaEReport"):
        from . import metrics
        return getattr(metrics, name)
    if name in ("RemasterRender", "RemasterClipRender"):
        from . import remaster_render
        return getattr(remaster_render, name)
    if name in ("SceneInfo", "scene_flags"):
        from . import scdetect
        return getattr(scdetect, name)
    if name == "EdgeSceneInfo":
        from .scdetect_edge import EdgeSceneInfo
        return EdgeSceneInfo
    if name == "DeviceImage":
        from .device import DeviceImage
        return DeviceImage
    if name in ("image_weighted_merge", "chroma_post_process", "chroma_stabilizer"):
        from . import imfilters
        return getattr(imfilters, name)
    raise AttributeError(name)
