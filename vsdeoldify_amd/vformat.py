"""Clips in their native video format: convert_format_RGB24 / restore_format (vsdeoldify/havc_utils.py:57-237), the first and the last step of every public
function of the reference, on the planes a decoder hands over -- without VapourSynth.

    clip = VideoClip((y, u, v), "YUV420P10", matrix="709", color_range="limited")
    rgb, info = convert_format_RGB24(clip, rgb_on_device=True)       # the upload is the planes (1.5 .. 3 B / pixel at 4:2:0), not RGB24 (3 B / pixel)
    ... HAVC_* on rgb ...
    out = restore_format(rgb, info)                                  # a VideoClip in the original's format, on the device because rgb is

PINNED -- the reference's Python, restated here as PLANS: `convert_calls`, `restore_calls` and `clip_info_fields` give the ordered resize.Bicubic calls with
their arguments and the ClipInfo fields for a format, a matrix prop and a range prop (either may be missing).  tests/golden/vformat.json records the same by
EXECUTING the reference against a recording vapoursynth stand-in (tools/gen_golden_vformat.py); tests/test_vformat_host.py compares them case by case.
`convert_steps` / `restore_steps` turn a plan into the fields of `havc_vformat`.  The quirks that are kept, each pinned by that fixture:
  * a missing matrix prop becomes 709, a missing range prop limited (:76-82), in the props of the clip AND in ClipInfo;
  * a clip of more than 8 bit first goes to 8 bit in a call of its own (:129-130) that names neither range nor dither: it takes the clip's OWN range from the
    props and does not dither -- a 10-bit clip loses two bits before the matrix step;
  * the YUV -> RGB24 call always says range_in_s="limited" (:136-143), whatever the range prop says, with dither_type="error_diffusion": a full-range clip is
    stretched as if it were limited;
  * GRAY -> RGB24 is limited -> full without a dither (:144-150);
  * restore_format sends a YUV original back to its own format, matrix and range with error diffusion (:191-207);
  * a GRAY original comes back as YUV420P8, BT.709, in the ORIGINAL's range (:208-222);
  * a clip that is not RGB24 is refused by restore_format with the reference's text (:181-182); an RGB24 clip passes both functions as it is.

UNPINNED -- resize.Bicubic itself is zimg's and cannot be executed where the fixtures are made.  tests/vformat_util.py restates it in numpy, on top of
tests/tweak_util.py, and is THE DEFINITION for this project (matrix constants, limited / full scaling per depth, the depth step, the Mitchell chroma
resampler, mirroring, Floyd - Steinberg error diffusion); the kernels (csrc/vformat.hip) equal it byte for byte.

Refused with NotImplementedError: chroma_resize=True (HAVC_clip_reconstruct already has a different stand-in of resize_to_chroma; reconciling the two is a
separate decision), RGB formats other than RGB24, float formats, 4:1:0 / 4:1:1 / 4:4:0 and other depths than 8 / 10 / 12 / 16, matrices other than "709",
"470bg", "170m", "2020ncl".  Everything malformed raises HAVCError before a context exists: plane shapes or dtypes that do not fit the format, an odd width
with 4:2:x, an odd height with 4:2:0, a side above 4096.

The planes of a VideoClip are numpy arrays or `DevicePlane`s (HBM, this module); DeviceImage stays what it is, an RGB container.  The HAVC_* functions are not
routed through this pair: they keep taking RGB24 arrays.
"""
import ctypes as C
import dataclasses
import re

import numpy as np

MAX_SIDE = 4096                                                # csrc/kernels.h TW_MAX_SIDE
MATRIX_CODES = {"709": 1, "470bg": 5, "170m": 6, "2020ncl": 9}                                     # H.273, VapourSynth's MatrixCoefficients
MATRIX_NAMES = {v: k for k, v in MATRIX_CODES.items()}
RANGE_FULL, RANGE_LIMITED = 0, 1                                                                   # VapourSynth's Range
RANGE_CODES = {"full": RANGE_FULL, "limited": RANGE_LIMITED}
FORMATS = {"RGB24": dict(family="RGB", sub_w=0, sub_h=0, bits=8)}
for _sub, (_sw, _sh) in {"420": (1, 1), "422": (1, 0), "444": (0, 0)}.items():
    for _bits in (8, 10, 12, 16):
        FORMATS[f"YUV{_sub}P{_bits}"] = dict(family="YUV", sub_w=_sw, sub_h=_sh, bits=_bits)
FORMATS.update(GRAY8=dict(family="GRAY", sub_w=0, sub_h=0, bits=8), GRAY16=dict(family="GRAY", sub_w=0, sub_h=0, bits=16))
_VS_NAME = re.compile(r"^(YUV4[0-4][0-4]P|GRAY|RGB)(\d{1,2}|S|H)$")
NOT_RGB24 = "restore_format: Input clip must be RGB24."                                            # havc_utils.py:182


def _err(msg):
    from .havc import HAVCError
    return HAVCError(msg)


def check_format(name):
    """-> the entry of FORMATS; a VapourSynth format outside it: NotImplementedError; anything else: HAVCError"""
    if name in FORMATS:
        return FORMATS[name]
    m = _VS_NAME.match(name) if isinstance(name, str) else None
    if not m:
        raise _err(f"VideoClip: {name!r} is not a VapourSynth format name")
    if m.group(2) in ("S", "H"):
        raise NotImplementedError(f"VideoClip: float formats ({name}) are not supported")
    if m.group(1) == "RGB":
        raise NotImplementedError(f"VideoClip: {name}: the only RGB format supported is RGB24")
    if m.group(1) in ("YUV410P", "YUV411P"):
        raise NotImplementedError(f"VideoClip: {name}: 4:1:0 and 4:1:1 are not supported")
    raise NotImplementedError(f"VideoClip: {name} is not supported (YUV 4:2:0 / 4:2:2 / 4:4:4 at 8, 10, 12, 16 bit, GRAY8, GRAY16)")


def check_props(matrix, color_range):
    if matrix is not None and matrix not in MATRIX_CODES:
        raise NotImplementedError(f'VideoClip: matrix {matrix!r}: only "709", "470bg", "170m", "2020ncl" or None are supported')
    if color_range is not None and color_range not in RANGE_CODES:
        raise _err(f'VideoClip: color_range {color_range!r} must be "limited", "full" or None')


# ---- the reference's Python as plans (pinned by tests/golden/vformat.json) -------------------------------------------------------------------------------------
def clip_info_fields(fmt, matrix=None, color_range=None):
    """the ClipInfo convert_format_RGB24 returns (:91-126), clip_orig aside: the props as the ORIGINAL clip has them, 709 / limited where one is missing"""
    f = check_format(fmt)
    check_props(matrix, color_range)
    return dict(format_id=fmt, color_family=f["family"], bits_per_sample=f["bits"], matrix=MATRIX_CODES[matrix or "709"],
                color_range=RANGE_CODES[color_range or "limited"], chroma_resize=False)


def _props(matrix, color_range):
    """the frame props behind :76-82"""
    return {"_Matrix": MATRIX_CODES[matrix or "709"], "_Range": RANGE_CODES[color_range or "limited"]}


def convert_calls(fmt, matrix=None, color_range=None):
    """the resize.Bicubic calls of convert_format_RGB24 in order, each [arguments, the frame props the call sees]"""
    f = check_format(fmt)
    check_props(matrix, color_range)
    if f["family"] == "RGB":
        return []
    props, calls = _props(matrix, color_range), []
    if f["bits"] != 8:
        calls.append([dict(format=fmt[:-len(str(f["bits"]))] + "8"), dict(props)])                               # :129-130
    if f["family"] == "YUV":
        calls.append([dict(format="RGB24", matrix_in=props["_Matrix"], range_in_s="limited", range_s="full", dither_type="error_diffusion"), dict(props)])
    else:
        calls.append([dict(format="RGB24", range_in_s="limited", range_s="full"), dict(props)])                   # :144-150
    return calls


def restore_calls(info):
    """the resize.Bicubic calls of restore_format for a ClipInfo (or its fields as a dict), each [arguments, the props of the RGB24 clip it gets]"""
    info = dataclasses.asdict(info) if dataclasses.is_dataclass(info) else info
    if info["format_id"] == "RGB24":
        return []                                                                                                  # :188-189
    props = {"_Matrix": info["matrix"], "_Range": RANGE_FULL}                                                      # :158-162
    range_s = "limited"
    if info["color_range"] is not None:
        range_s = "full" if info["color_range"] == RANGE_FULL else "limited"
    if info["color_family"] == "YUV":
        matrix = info["matrix"] if info["matrix"] is not None else MATRIX_CODES["709"]
        return [[dict(format=info["format_id"], matrix_in=MATRIX_CODES["709"], matrix=matrix, range_in_s="full", range_s=range_s,
                      dither_type="error_diffusion"), props]]
    return [[dict(format="YUV420P8", matrix=MATRIX_CODES["709"], range_in_s="full", range_s=range_s, dither_type="error_diffusion"), props]]


# ---- plans -> what the library is asked for --------------------------------------------------------------------------------------------------------------------
def convert_steps(fmt, matrix=None, color_range=None):
    """the calls of convert_calls as the fields of one havc_planes_to_rgb24: the depth step's range comes from the props that call sees, the matrix step's
    from its own range_in_s"""
    calls = convert_calls(fmt, matrix, color_range)
    last_args, last_props = calls[-1]
    depth_props = calls[0][1] if len(calls) == 2 else last_props
    return dict(matrix=MATRIX_NAMES[last_args.get("matrix_in", last_props["_Matrix"])], full_range=last_args["range_in_s"] == "full",
                depth_full_range=depth_props["_Range"] == RANGE_FULL, dither=last_args.get("dither_type") == "error_diffusion")


def restore_steps(fmt, matrix=None, color_range=None, info=None):
    """the one call of restore_calls as the fields of havc_rgb24_to_planes: the destination format, its matrix, its range, the dither"""
    (args, _), = restore_calls(info if info is not None else clip_info_fields(fmt, matrix, color_range))
    return dict(format=args["format"], matrix=MATRIX_NAMES[args["matrix"]], full_range=args["range_s"] == "full", dither=args.get("dither_type") == "error_diffusion")


# ---- the containers ----------------------------------------------------------------------------------------------------------------------------------------
class DevicePlane:
    """one plane stack [n, h, w] of uint8 or uint16 in HBM, from the context's buffer pool (device.py)"""

    def __init__(self, ctx, shape, dtype):
        from .device import pool_alloc
        self.ctx, self.shape, self.dtype = ctx, tuple(int(s) for s in shape), np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        self.ptr = pool_alloc(ctx, self.nbytes)

    def __del__(self):
        try:
            if self.ptr is not None and self.ctx.h:
                from .device import pool_release
                pool_release(self.ctx, self.ptr, self.nbytes)
        except Exception:
            pass
        self.ptr = None

    @classmethod
    def from_numpy(cls, ctx, arr):
        arr = np.ascontiguousarray(arr)
        d = cls(ctx, arr.shape, arr.dtype)
        ctx.dev_upload(d.ptr, arr)
        return d

    def numpy(self):
        out = np.empty(self.shape, self.dtype)
        self.ctx.dev_download(out, self.ptr)                    # orders behind everything queued on the ctx stream
        return out


def _plane_ptr(p):
    from . import _native as nat
    return p.ptr if isinstance(p, DevicePlane) else nat.as_ptr(p)


class VideoClip:
    """a clip's planes in a VapourSynth format: `planes` [n, h, w] arrays (ndarray or DevicePlane), one for GRAY, three for YUV with the chroma planes at the
    subsampled size; uint8 for 8 bit, uint16 above; matrix "709" / "470bg" / "170m" / "2020ncl" / None, color_range "limited" / "full" / None (the frame
    props, None: missing).  Everything that does not fit is refused here, before anything touches the GPU."""

    def __init__(self, planes, format, matrix=None, color_range=None):
        f = check_format(format)
        check_props(matrix, color_range)
        if f["family"] == "RGB":
            raise _err("VideoClip: an RGB24 clip is a uint8 [n, h, w, 3] array or a DeviceImage, not a VideoClip")
        planes = tuple(planes) if isinstance(planes, (list, tuple)) else (planes,)
        want = 1 if f["family"] == "GRAY" else 3
        if len(planes) != want:
            raise _err(f"VideoClip: {format} has {want} plane(s), got {len(planes)}")
        dtype = np.dtype(np.uint8 if f["bits"] == 8 else np.uint16)
        planes = tuple(p if isinstance(p, DevicePlane) else np.asarray(p) for p in planes)
        shape = tuple(planes[0].shape)
        if len(shape) != 3 or min(shape) < 1:
            raise _err(f"VideoClip: planes are [n, h, w] arrays, got {shape}")
        n, h, w = shape
        if h > MAX_SIDE or w > MAX_SIDE:
            raise _err(f"VideoClip: frames of {w} x {h} are larger than {MAX_SIDE} x {MAX_SIDE}")
        if (f["sub_w"] and w % 2) or (f["sub_h"] and h % 2):
            raise _err(f"VideoClip: a frame of {w} x {h} cannot be {format}: 4:2:x needs an even width, 4:2:0 an even height (VapourSynth refuses it too)")
        shapes = [shape] + [(n, h >> f["sub_h"], w >> f["sub_w"])] * (want - 1)
        for p, s in zip(planes, shapes):
            if tuple(p.shape) != s or np.dtype(p.dtype) != dtype:
                raise _err(f"VideoClip: {format} at {w} x {h} needs {dtype.name} planes {shapes}, got {np.dtype(p.dtype).name} {tuple(p.shape)}")
        self.planes = tuple(p if isinstance(p, DevicePlane) else np.ascontiguousarray(p) for p in planes)
        self.format, self.matrix, self.color_range = format, matrix, color_range
        self.num_frames, self.height, self.width = n, h, w

    @property
    def on_device(self):
        return any(isinstance(p, DevicePlane) for p in self.planes)

    def numpy(self):
        """the planes as ndarrays (a device plane is downloaded)"""
        return tuple(p.numpy() if isinstance(p, DevicePlane) else p for p in self.planes)


@dataclasses.dataclass
class ClipInfo:
    """havc_utils.py:36-44; format_id is VapourSynth's name, color_family "YUV" / "GRAY" / "RGB", matrix and color_range VapourSynth's integers"""
    clip_orig: object
    format_id: str
    color_family: str
    bits_per_sample: int
    matrix: int
    color_range: int
    chroma_resize: bool


def _is_rgb24(clip):
    from .device import is_device
    if is_device(clip):
        return len(clip.shape) == 4
    return isinstance(clip, np.ndarray) and clip.ndim == 4 and clip.shape[-1] == 3 and clip.dtype == np.uint8 and min(clip.shape) >= 1


def _vformat(f, n, h, w, steps, depth_full_range=False, chunk_frames=0):
    from . import _native as nat
    return nat.VFormat(width=w, height=h, n_frames=n, family=1 if f["family"] == "GRAY" else 0, sub_w=f["sub_w"], sub_h=f["sub_h"], bits=f["bits"],
                       matrix=MATRIX_CODES[steps["matrix"]], full_range=int(steps["full_range"]), depth_full_range=int(depth_full_range),
                       dither=int(steps["dither"]), chunk_frames=int(chunk_frames))


def check_rgb_size(fmt, h, w):
    f = FORMATS[fmt]
    if (f["sub_w"] and w % 2) or (f["sub_h"] and h % 2) or h > MAX_SIDE or w > MAX_SIDE:
        raise _err(f"restore_format: a frame of {w} x {h} cannot be {fmt} (even sides where the chroma is subsampled, at most {MAX_SIDE} x {MAX_SIDE})")


def planes_to_rgb24_np(ctx, clip, steps, device=False, chunk_frames=0):
    """havc_planes_to_rgb24 on a VideoClip with the fields of convert_steps -> RGB24, an ndarray or (device) a DeviceImage"""
    from . import _native as nat
    from .device import DeviceImage, operand_ptr
    f = FORMATS[clip.format]
    n, h, w = clip.num_frames, clip.height, clip.width
    p = _vformat(f, n, h, w, steps, steps["depth_full_range"], chunk_frames)
    out = DeviceImage(ctx, (n, h, w, 3)) if device else np.empty((n, h, w, 3), np.uint8)
    ptrs = [_plane_ptr(q) for q in clip.planes] + [None] * (3 - len(clip.planes))
    nat.check(ctx.lib.havc_planes_to_rgb24(ctx.h, ptrs[0], ptrs[1], ptrs[2], operand_ptr(out), C.byref(p)), ctx.h)
    return out


def rgb24_to_planes_np(ctx, rgb, fmt, steps, device=False, chunk_frames=0):
    """havc_rgb24_to_planes: RGB24 [n, h, w, 3] (ndarray or DeviceImage) -> the three planes of `fmt`, ndarrays or (device) DevicePlanes"""
    from . import _native as nat
    from .device import is_device, operand_ptr
    f = FORMATS[fmt]
    n, h, w = rgb.shape[:3]
    check_rgb_size(fmt, h, w)
    if not is_device(rgb):
        rgb = np.ascontiguousarray(rgb)
    dtype = np.uint8 if f["bits"] == 8 else np.uint16
    shapes = [(n, h, w)] + [(n, h >> f["sub_h"], w >> f["sub_w"])] * 2
    planes = [DevicePlane(ctx, s, dtype) if device else np.empty(s, dtype) for s in shapes]
    p = _vformat(f, n, h, w, steps, False, chunk_frames)
    nat.check(ctx.lib.havc_rgb24_to_planes(ctx.h, operand_ptr(rgb), _plane_ptr(planes[0]), _plane_ptr(planes[1]), _plane_ptr(planes[2]), C.byref(p)), ctx.h)
    return tuple(planes)


# ---- the two functions ---------------------------------------------------------------------------------------------------------------------------------------
def convert_format_RGB24(clip, chroma_resize=False, *, device_index=0, rgb_on_device=False):
    """havc_utils.py:57-164 -> (rgb, ClipInfo).  clip: a VideoClip, or an RGB24 clip (uint8 [n, h, w, 3] ndarray or DeviceImage), which passes as it is.  The
    result is a DeviceImage when a plane of the clip is on the device or rgb_on_device is set (host planes are then uploaded as planes), else an ndarray."""
    if chroma_resize:
        raise NotImplementedError("convert_format_RGB24: chroma_resize=True is not supported (HAVC_clip_reconstruct has its own stand-in of resize_to_chroma)")
    if _is_rgb24(clip):
        return clip, ClipInfo(clip_orig=None, **clip_info_fields("RGB24"))
    if not isinstance(clip, VideoClip):
        raise _err("convert_format_RGB24: Input is not a valid clip.")                                            # :69
    info = ClipInfo(clip_orig=None, **clip_info_fields(clip.format, clip.matrix, clip.color_range))
    from .render import get_context
    ctx = get_context(device_index)
    steps = convert_steps(clip.format, clip.matrix, clip.color_range)
    return planes_to_rgb24_np(ctx, clip, steps, device=rgb_on_device or clip.on_device), info


def restore_format(rgb, clip_info, *, device_index=0):
    """havc_utils.py:167-237: the RGB24 clip in the format clip_info remembers -> a VideoClip (planes on the device when rgb is a DeviceImage), or rgb itself
    when the original was RGB24"""
    from .device import is_device
    if isinstance(rgb, VideoClip):
        raise _err(NOT_RGB24)
    if not _is_rgb24(rgb):
        raise _err("restore_format: Input is not a valid clip.")                                                  # :179
    if clip_info.chroma_resize:
        raise NotImplementedError("restore_format: chroma_resize=True is not supported")
    if clip_info.format_id == "RGB24":
        return rgb
    steps = restore_steps(None, info=clip_info)
    check_rgb_size(steps["format"], rgb.shape[1], rgb.shape[2])
    from .render import get_context
    ctx = get_context(device_index)
    planes = rgb24_to_planes_np(ctx, rgb, steps["format"], steps, device=is_device(rgb))
    return VideoClip(planes, steps["format"], MATRIX_NAMES[MATRIX_CODES[steps["matrix"]]], "full" if steps["full_range"] else "limited")
