"""Import shims that let the reference's DeepRemaster package (vsdeoldify/remaster) run on the CPU-only build container.
Build container only (needs the reference tree); nothing here ships reference code.  On top of tools/refshim.install():

  cv2.cvtColor(img, COLOR_RGB2GRAY)        -> OpenCV's published 8-bit formula (4899 R + 9617 G + 1868 B + 8192) >> 14 (cv2 is absent: PARITY UNPINNED at
                                              LSB level, like the YUV stand-in of oracle.cvcolor)
  skimage.color.lab2rgb / rgb2lab          -> oracle.zhang (CIE formulas in fp64; skimage absent: PARITY UNPINNED)
  torchvision.transforms.Resize / ToTensor -> PIL Image.resize(BICUBIC) / uint8 HWC -> float32 CHW / 255 (what torchvision does for PIL inputs)
  vapoursynth                              -> the empty module of tools/refshim.py plus the constants vsslib/vsutils.py reads at import time
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import refshim  # noqa: E402

COLOR_RGB2GRAY = 7


def rgb2gray_u8(img):
    a = np.asarray(img).astype(np.int64)
    return ((4899 * a[..., 0] + 9617 * a[..., 1] + 1868 * a[..., 2] + 8192) >> 14).astype(np.uint8)


def install():
    refshim.install()
    from oracle import zhang

    vs = sys.modules["vapoursynth"]
    for i, n in enumerate(("DEBUG", "INFORMATION", "WARNING", "CRITICAL", "FATAL")):
        setattr(vs, "MESSAGE_TYPE_" + n, i)

    cv2 = sys.modules["cv2"]
    yuv = cv2.cvtColor
    cv2.COLOR_RGB2GRAY = COLOR_RGB2GRAY
    cv2.cvtColor = lambda src, code: rgb2gray_u8(src) if code == COLOR_RGB2GRAY else yuv(src, code)

    class Resize:
        def __init__(self, size, interpolation=3):
            self.size, self.interpolation = size, interpolation

        def __call__(self, img):
            h, w = self.size
            return img.resize((w, h), resample=self.interpolation)

    class ToTensor:
        def __call__(self, pic):
            a = np.asarray(pic)
            if a.ndim == 2:
                a = a[:, :, None]
            t = torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1)))
            return t.float().div(255) if t.dtype == torch.uint8 else t

    tvt = sys.modules["torchvision.transforms"]
    tvt.Resize, tvt.ToTensor = Resize, ToTensor
    sys.modules["torchvision"].transforms = tvt

    sk = types.ModuleType("skimage")
    skc = types.ModuleType("skimage.color")
    skc.rgb2lab = lambda img: zhang.rgb2lab(np.asarray(img))
    skc.lab2rgb = lambda lab: zhang.lab2rgb(lab)
    sk.color = skc
    sys.modules["skimage"], sys.modules["skimage.color"] = sk, skc

    torch.cuda.empty_cache = lambda: None
    ref = refshim.REF_ROOT + "/vsdeoldify"
    for pkg in (".remaster", ".remaster.model"):
        m = types.ModuleType("vsdeoldify" + pkg)
        m.__path__ = [ref + pkg.replace(".", "/")]
        sys.modules["vsdeoldify" + pkg] = m


def build_network():
    """the reference's NetworkC (remaster/model/remasternet.py:103-187), constructor-initialised, eval mode"""
    install()
    from vsdeoldify.remaster.model.remasternet import NetworkC
    return NetworkC().eval()
