"""RemasterRender: the host side of DeepRemaster, the mirror of the reference's RemasterEngine / RemasterColorizer
(vsdeoldify/remaster/remaster_render.py:51-451) on the MI355X.

Restated from the reference: the reference list (get_ref_list, remaster_utils.py:111-131), the buffer-size rule, the target size of the stills and
addMergin (remaster_utils.py:46-59), the window rule (ref_buffer_adjust: at most one advance per process_frames call) and the doubling of a single frame.
What differs is where the stills' features live: the reference pushes every still of the window through reffeatnet1 / reffeatnet2 on every call; here a
still is encoded once, when it enters the window, into a slot of the reference ring (remaster_net.RemasterSession), and an advance overwrites the slot of
the oldest still.  Both are exact: the two stacks are per-frame, and a softmax does not depend on the order of its keys.
"""
import math
import os

import numpy as np

from . import _native as nat
from .device import DeviceImage, is_device
from .remaster_net import RemasterColorNet, RemasterSession
from .render import get_context

DEF_MAX_RF_FRAMES, DEF_MIN_RF_FRAMES, DEF_FUTURE_FRAME_WEIGHT = 200, 4, 0.5       # vsslib/constants.py:65-74
IMG_EXTENSIONS = ('.png', '.PNG', '.jpg', '.JPG', '.jpeg', '.JPEG', '.ppm', '.PPM', '.bmp', '.BMP')
BICUBIC = 3


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
