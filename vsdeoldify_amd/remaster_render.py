"""RemasterRender: the host side of DeepRemaster, the mirror of the reference's RemasterEngine / RemasterColorizer
(vsdeoldify/remaster/remaster_render.py:51-451) on the MI355X.

Restated from the reference: the reference list (get_ref_list, remaster_utils.py:111-131), the buffer-size rule, the target size of the stills and
addMergin (remaster_utils.py:46-59), the window rule (ref_buffer_adjust: at most one advance per process_frames call) and the doubling of a single frame.
What differs is where the stills' features live: the reference pushes every still of the window through reffeatnet1 / reffeatnet2 on every call; here a
still is encoded once, when it enters the window, into a slot of the reference ring (remaster_net.RemasterSession), and an advance overwrites the slot of
the oldest still.  Both are exact: the two stacks are per-frame, and a softmax does not depend on the order of its keys.

RemasterClipRender / ClipReferenceWindow are the clip mode (RemasterColorizer, remaster_render.py:51-277; HAVC_restore_video with ex_model = 2): the stills
are the frames of a reference clip that scene-change flags mark, found by scanning the flags lazily in chunks of 500 frames.
"""
import math
import os

import numpy as np

from . import _native as nat
from .device import DeviceImage, is_device
from .remaster_net import RemasterColorNet, RemasterSession
from .render import get_context

DEF_MAX_RF_FRAMES, DEF_MIN_RF_FRAMES, DEF_FUTURE_FRAME_WEIGHT = 200, 4, 0.5       # vsslib/constants.py:65-74
DEF_MAX_BUFFER_SIZE = 500                                                          # vsslib/constants.py:68: frames per scan for reference frames
IMG_EXTENSIONS = ('.png', '.PNG', '.jpg', '.JPG', '.jpeg', '.JPEG', '.ppm', '.PPM', '.bmp', '.BMP')
LANCZOS, BICUBIC = 1, 3


def get_ref_num(filename):
    """remaster_utils.py:111-114: the integer after the last '_' of the file name up to its first '.'.  The reference splits the whole path, so a '.'
    anywhere in a directory name makes it raise; here only the file's own name is parsed (the same number wherever the reference returns one)."""
    return int(os.path.basename(filename).split(".")[0].split("_")[-1])


def get_ref_list(img_dir):
    """remaster_utils.py:127-131: sorted image files of the directory and their frame numbers"""
    files = sorted(os.path.join(img_dir, f) for f in os.listdir(img_dir)
                   if os.path.isfile(os.path.join(img_dir, f)) and any(f.endswith(e) for e in IMG_EXTENSIONS))
    return files, [get_ref_num(f) for f in files]


def normalize_buffer_size(n):
    """remaster_render.py:326: a multiple of 2 within [4, 200]"""
    return max(min(math.trunc(n / 2) * 2, DEF_MAX_RF_FRAMES), DEF_MIN_RF_FRAMES)


def target_size(w, h, ref_minedge):
    """remaster_render.py:366-369, from the first still: (target_w, target_h)"""
    aspect = w / h
    return (int(ref_minedge * aspect) if aspect > 1 else ref_minedge), (ref_minedge if aspect >= 1 else int(ref_minedge / aspect))


def margin_geometry(w, h, target_w, target_h):
    """addMergin (remaster_utils.py:46-59): size the still is resized to and where it is pasted; None = the still already has the target size"""
    if w == target_w and h == target_h:
        return None
    scale = max(target_w, target_h) / max(w, h)
    rw, rh = int(w * scale / 16.) * 16, int(h * scale / 16.) * 16
    return rw, rh, (target_w - rw) // 2, (target_h - rh) // 2


def resize_for_inference_size(w, h, frame_mindim):
    """remaster_utils.py:134-143: the size the clip is brought to for inference"""
    minwh = min(w, h)
    scale = 1 if minwh == frame_mindim else frame_mindim / minwh
    return round(w * scale / 16.) * 16, round(h * scale / 16.) * 16


class ReferenceWindow:
    """Which stills the window holds (host logic only).  slots[i] = index into the reference list of the still in ring slot i."""

    def __init__(self, ref_num_list, ref_buffer_size):
        self.nums = list(ref_num_list)
        self.size = min(ref_buffer_size, len(self.nums))
        self.half_idx = round(self.size * (1 - DEF_FUTURE_FRAME_WEIGHT)) - 1
        self.last_idx = self.size - 1
        self.slots = list(range(self.size))

    def advance(self, frame_n):
        """ref_buffer_adjust (remaster_render.py:387-408): -> (slot, index of the still that enters it) or None"""
        if self.last_idx == len(self.nums) - 1 or frame_n <= self.nums[self.half_idx]:
            return None
        self.last_idx += 1
        self.half_idx += 1
        slot = self.slots.index(self.last_idx - self.size)           # the oldest still
        self.slots[slot] = self.last_idx
        return slot, self.last_idx

    def numbers(self):
        """frame numbers of the stills in the window, in the reference's order (oldest first)"""
        return [self.nums[i] for i in sorted(self.slots)]


class ClipReferenceWindow(ReferenceWindow):
    """The reference list of RemasterColorizer (clip mode, remaster_render.py:122-231): the frames whose _SceneChangePrev flag is 1, found by scanning
    the flags lazily in chunks of max_buffer_size frames.  get_clip_ref_list: the first scan covers min(n, 500) frames and up to ten extensions follow
    while fewer references than the buffer size are known; fewer than DEF_MIN_RF_FRAMES then raise (the message says "at least 2", as there).  The
    window size (ref_storage_size) is fixed from what that found.  ref_buffer_adjust: every call first extends the list once when frame_n >=
    clip_last_frame - clip_buffer_size, then applies the window rule of ReferenceWindow with the count known at that moment.  fast_refs (ref_step in
    2..4) is never on through HAVC_restore_video and is not built."""

    def __init__(self, flags, ref_buffer_size, max_buffer_size=DEF_MAX_BUFFER_SIZE):
        self.flags = flags                                   # _SceneChangePrev per frame of clip_sc: anything indexable with a length
        self.max_buffer_size = max_buffer_size
        self.clip_total_frames = len(flags)
        self.clip_buffer_size = min(self.clip_total_frames, max_buffer_size)
        self.nums = [i for i in range(self.clip_buffer_size) if flags[i] == 1]
        self.clip_last_frame = self.clip_buffer_size - 1
        for _ in range(10):
            if len(self.nums) < ref_buffer_size and self.clip_last_frame < self.clip_total_frames - 1:
                self.extend()
            else:
                break
        if len(self.nums) < DEF_MIN_RF_FRAMES:
            from .havc import HAVCError
            raise HAVCError(f"RemasterColorizer(): number of reference frames must be at least 2, found  {len(self.nums)}")   # HAVC_LogMessage joins with a blank
        super().__init__(self.nums, ref_buffer_size)

    def extend(self):
        """extend_clip_ref_list: the flags of the next max_buffer_size frames"""
        if self.clip_last_frame == self.clip_total_frames - 1:
            return
        num_frames = min(self.clip_total_frames - self.clip_last_frame - 1, self.max_buffer_size)
        batch_size = self.clip_last_frame + num_frames + 1
        self.nums.extend(i for i in range(self.clip_last_frame + 1, batch_size) if self.flags[i] == 1)
        self.clip_last_frame = batch_size - 1

    def advance(self, frame_n):
        if frame_n >= self.clip_last_frame - self.clip_buffer_size:
            self.extend()
        return super().advance(frame_n)


class RemasterRender:
    def __init__(self, device_index=0, ref_minedge=256, ref_buffer_size=20, length=2, model_dir=None, state_dict=None, model=None, precision=None):
        """length: frames per process_frames call the plan is built for (2-5; shorter calls run on the same plan).  Weights: a built RemasterColorNet, a
        state dict of NetworkC (or {'modelC': ...}), or model_dir/remasternet.pth.tar.  precision: "fast" only (this class's default whatever the package
        default is); an explicit "precise" -- the argument or HAVC_PRECISION -- raises NotImplementedError."""
        p = precision or os.environ.get("HAVC_PRECISION") or "fast"
        if p == "precise":
            raise NotImplementedError("RemasterRender: precision 'precise' is not built for DeepRemaster (fast mode only: fp16 activations, fp32 accumulation)")
        if p != "fast":
            raise ValueError(f"precision must be 'fast' or 'precise', got {p!r}")
        if length < 2:
            raise ValueError("RemasterRender: length must be at least 2")
        self.device_index, self.ref_minedge, self.length = device_index, ref_minedge, int(length)
        self.ref_buffer_size = normalize_buffer_size(ref_buffer_size)
        self._model, self._state_dict, self._model_dir = model, state_dict, model_dir
        self.ctx = None
        self.window, self.target_w, self.target_h = None, None, None
        self._session = self._weights = self._images = None

    # ---- references ----
    def load_ref_dir(self, rf_dir):
        """RemasterEngine.load_ref_dir: the image files of a directory; fewer than two -> the last one repeated.  Returns the number of stills."""
        from PIL import Image
        files, nums = get_ref_list(rf_dir)
        if not files:
            return 0
        return self.load_refs([np.asarray(Image.open(f).convert('RGB')) for f in files], nums)

    def load_refs(self, images, frame_numbers):
        """stills as u8 RGB arrays (any size) with their frame numbers, in the order of the reference list"""
        images, nums = [np.ascontiguousarray(i, dtype=np.uint8) for i in images], [int(n) for n in frame_numbers]
        assert len(images) == len(nums) and images
        if len(images) < 2:
            images.append(images[-1])
            nums.append(nums[-1])
        self._close_session()
        self.window = ReferenceWindow(nums, self.ref_buffer_size)
        h, w = images[0].shape[:2]
        self.target_w, self.target_h = target_size(w, h, self.ref_minedge)
        self._images = images
        return len(images)

    def add_margin(self, img):
        """addMergin: PIL BICUBIC to the 16-aligned size, centred paste on black (Image.paste clips what does not fit)"""
        from .colorization import pil_resize_np
        g = margin_geometry(img.shape[1], img.shape[0], self.target_w, self.target_h)
        if g is None:
            return img
        rw, rh, xp, yp = g
        small = pil_resize_np(self._ctx(), img, (rw, rh), BICUBIC)
        out = np.zeros((self.target_h, self.target_w, 3), np.uint8)
        x0, y0, x1, y1 = max(xp, 0), max(yp, 0), min(xp + rw, self.target_w), min(yp + rh, self.target_h)
        out[y0:y1, x0:x1] = small[y0 - yp:y1 - yp, x0 - xp:x1 - xp]
        return out

    def _ref_image(self, idx):
        return np.ascontiguousarray(self.add_margin(self._images[idx]))

    # ---- device side ----
    def _ctx(self):
        if self.ctx is None:
            self.ctx = get_context(self.device_index)
        return self.ctx

    def _net_model(self):
        if self._model is None:
            sd = self._state_dict
            if sd is None:
                import torch
                path = os.path.join(self._model_dir or os.path.join(os.path.dirname(os.path.abspath(__file__)), "models"), "remasternet.pth.tar")
                sd = torch.load(path, map_location="cpu")
            self._model = RemasterColorNet(sd)
        return self._model

    def _close_session(self):
        if self._session is not None:
            self._session.close()
            self._session = None

    def close(self):
        self._close_session()
        if self._weights is not None:
            self._weights.close()
            self._weights = None

    def _get_session(self, H, W):
        s = self._session
        if s is not None and (s.plan.H, s.plan.W) == (H, W):
            return s
        self._close_session()
        ctx, model = self._ctx(), self._net_model()
        if self._weights is None:
            self._weights = nat.Weights(ctx, model.blob)
        if self.window is None:
            s = RemasterSession(ctx, model, self.length, H, W, weights=self._weights)
        else:
            s = RemasterSession(ctx, model, self.length, H, W, (self.target_h, self.target_w), self.window.size, weights=self._weights)
            for slot, idx in enumerate(self.window.slots):
                s.encode_reference(slot, self._ref_image(idx))
        self._session = s
        return s

    def process_frames(self, frames, last_frame_idx=0):
        """RemasterEngine.process_frames: 1..length frames of one size (u8 [n][h][w][3] array, a list of [h][w][3] arrays, or a DeviceImage) -> the
        coloured frames in the same form.  last_frame_idx moves the reference window (at most one still per call)."""
        dev = is_device(frames)
        if not dev:
            frames = np.ascontiguousarray(np.stack(frames) if isinstance(frames, (list, tuple)) else frames, dtype=np.uint8)
        if frames.ndim != 4 or frames.shape[3] != 3 or not 1 <= frames.shape[0] <= self.length:
            raise ValueError(f"RemasterRender.process_frames: 1..{self.length} RGB frames [n, h, w, 3], got {tuple(frames.shape)}")
        n, H, W = frames.shape[:3]
        s = self._get_session(H, W)
        if self.window is not None:
            moved = self.window.advance(last_frame_idx)
            if moved is not None:
                s.encode_reference(moved[0], self._ref_image(moved[1]))
        if not dev:
            return s.colorize(frames)
        out = DeviceImage(self.ctx, frames.shape)
        src = frames
        if n == 1:                                  # the reference doubles a single frame and returns one
            src = DeviceImage(self.ctx, (2, H, W, 3))
            src.frame(0).copy_from(frames.frame(0))
            src.frame(1).copy_from(frames.frame(0))
        tmp = out if n > 1 else DeviceImage(self.ctx, (2, H, W, 3))
        s.colorize(src.ptr, tmp.ptr, n=max(n, 2))
        if n == 1:
            out.frame(0).copy_from(tmp.frame(0))
            self.ctx.synchronize()                  # src / tmp go back to the pool when this returns
        return out


class RemasterClipRender(RemasterRender):
    """RemasterColorizer (remaster_render.py:51-277): RemasterRender with its stills taken from a reference CLIP -- the frames of clip_ref that the
    scene-change flags of clip_sc mark (ClipReferenceWindow).  clip_ref is a u8 [n][h][w][3] array or a DeviceImage; the stills of a device-resident
    clip_ref are resized (Pillow BICUBIC), pasted on black and encoded without leaving HBM.  The ring of encoded stills is RemasterRender's."""

    _clip_ref = _still = None

    def load_clip_ref(self, clip_ref, flags):
        """load_clip_ref: flags = _SceneChangePrev per frame of clip_sc (clip_ref's own scenes when the caller has no clip_sc).  Returns the number of
        references the first scans found."""
        if not is_device(clip_ref):
            clip_ref = np.ascontiguousarray(clip_ref, dtype=np.uint8)
        if clip_ref.ndim != 4 or clip_ref.shape[3] != 3 or len(flags) != clip_ref.shape[0]:
            raise ValueError(f"RemasterClipRender.load_clip_ref: clip_ref [n, h, w, 3] with one flag per frame, got {tuple(clip_ref.shape)} and {len(flags)} flags")
        self._close_session()
        self.window = ClipReferenceWindow(flags, self.ref_buffer_size)
        h, w = clip_ref.shape[1:3]
        self.target_w, self.target_h = target_size(w, h, self.ref_minedge)
        self._clip_ref = clip_ref
        return len(self.window.nums)

    def _ref_image(self, idx):
        n = self.window.nums[idx]
        if not is_device(self._clip_ref):
            return np.ascontiguousarray(self.add_margin(self._clip_ref[n]))
        self._still = self._add_margin_dev(self._clip_ref.frame(n))          # alive until the (blocking) encode has run
        return self._still.ptr

    def _add_margin_dev(self, frame):
        """addMergin on a device frame: the same resize entry point on device operands, a pitched device copy for the paste"""
        ctx = self._ctx()
        h, w = frame.shape[:2]
        g = margin_geometry(w, h, self.target_w, self.target_h)
        if g is None:
            return frame
        rw, rh, xp, yp = g
        small = DeviceImage(ctx, (rh, rw, 3))
        nat.check(ctx.lib.havc_pil_resize(ctx.h, frame.ptr, w, h, small.ptr, rw, rh, BICUBIC), ctx.h)
        out = DeviceImage(ctx, (self.target_h, self.target_w, 3))
        nat.check(ctx.lib.havc_dev_memset(ctx.h, out.ptr, 0, out.nbytes), ctx.h)
        x0, y0, x1, y1 = max(xp, 0), max(yp, 0), min(xp + rw, self.target_w), min(yp + rh, self.target_h)
        if x1 > x0 and y1 > y0:
            nat.check(ctx.lib.havc_dev_copy_2d(ctx.h, out.ptr.value + (y0 * self.target_w + x0) * 3, self.target_w * 3,
                                               small.ptr.value + ((y0 - yp) * rw + (x0 - xp)) * 3, rw * 3, (x1 - x0) * 3, y1 - y0), ctx.h)
        ctx.synchronize()                                                     # `small` goes back to the pool when this returns
        return out

    def process_clip_frames(self, frames, first_frame, last_frame_idx, merge_weight=1.0):
        """color_remaster / color_merge_remaster (remaster/__init__.py:123-173): process_frames on the frames first_frame.. of the clip; with
        0 < merge_weight < 1 every coloured frame is blended (Image.blend) with its own clip_ref frame, brought to its size with Pillow LANCZOS."""
        out = self.process_frames(frames, last_frame_idx)
        if not 0 < merge_weight < 1:
            return out
        from . import imfilters as F
        ctx, dev = self._ctx(), is_device(out)
        n, H, W = out.shape[:3]
        cr = self._clip_ref
        ref = cr.frames(first_frame, first_frame + n) if is_device(cr) else cr[first_frame:first_frame + n]
        if tuple(ref.shape[1:3]) != (H, W):
            ref = lanczos_resize(ctx, ref, W, H, device=dev)                  # the batch's frames in one call: one pair of coefficient tables
        if dev:
            ref = ref if is_device(ref) else DeviceImage.from_numpy(ctx, ref)
            merged = F.blend_np(ctx, out, ref, merge_weight)                  # per pixel: the batch as one tall image
            ctx.synchronize()                                                 # `ref` goes back to the pool when this returns
            return merged
        return F.blend_np(ctx, out.reshape(n * H, W, 3), np.ascontiguousarray(ref).reshape(n * H, W, 3), merge_weight).reshape(out.shape)


def lanczos_resize(ctx, img, w, h, device=None):
    """Pillow Image.resize((w, h), LANCZOS) of one u8 frame [h][w][3] or of n frames [n][h][w][3] in one call, host or device operand; device=True / False
    chooses where the result lives (default: where the operand is)"""
    dev_in = is_device(img)
    device = dev_in if device is None else device
    if not dev_in:
        img = np.ascontiguousarray(img, dtype=np.uint8)
    n = img.shape[0] if img.ndim == 4 else 1
    shape = (n, h, w, 3) if img.ndim == 4 else (h, w, 3)
    out = DeviceImage(ctx, shape) if device else np.empty(shape, np.uint8)
    nat.check(ctx.lib.havc_pil_resize_n(ctx.h, img.ptr if dev_in else nat.as_ptr(img), img.shape[-2], img.shape[-3],
                                        out.ptr if device else nat.as_ptr(out), w, h, LANCZOS, n), ctx.h)
    return out
