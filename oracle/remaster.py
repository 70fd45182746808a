"""DeepRemaster's non-conv operations in plain float64 numpy, each restated from its definition (tests/test_gpu_remaster_ops.py holds the HIP kernels of
vsdeoldify_amd/csrc/remaster.hip against these, one op at a time).

  srcref_attention   SourceReferenceAttention.forward: out = gamma * softmax(q k^T) v + x over ALL keys of all stills; no 1 / sqrt(d)
  tstack             the temporal neighbours t-1, t, t+1 side by side in the channels (what a (3,3,3) kernel with zero padding in time sees)
  conv3d_same        direct 3-D convolution, kernel (3,3,3), zero padding 1, for the tstack + 3 x 3 conv composite
  elu                x > 0 ? x : expm1(x)
  gray_u8            OpenCV's 8-bit COLOR_RGB2GRAY: (4899 R + 9617 G + 1868 B + 8192) >> 14
  prep_frames / prep_refs    the network's gray input with its replicate border / the reference stills
  sigmoid, lab_from_sigmoid  the output stage up to Lab; lab_from_sigmoid is the ONE float32 function here: it restates the float32 steps the reference
                     takes between the sigmoid and skimage's lab2rgb (numpy float32 arithmetic, which the kernel reproduces because remaster.o is
                     built without contraction), so that the float64 Lab -> RGB chain after it starts from the very same values
"""
import numpy as np


def softmax(s):
    s = np.asarray(s, np.float64)
    e = np.exp(s - s.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def srcref_attention(x, q, k, v, gamma):
    """x [NQ, 512], q [NQ, 64], k [NK, 64], v [NK, 512] -> (out [NQ, 512], A [NQ, 512]); A = softmax . |v|, the attention-weighted mean of |v|"""
    x, q, k, v = (np.asarray(a, np.float64) for a in (x, q, k, v))
    p = softmax(q @ k.T)
    return float(gamma) * (p @ v) + x, p @ np.abs(v)


def tstack(x):
    """[T, P, C] -> [T, P, 3 C]: channel kt * C + c of frame t is channel c of frame t + kt - 1, zeros outside [0, T)"""
    x = np.asarray(x)
    T, P, C = x.shape
    y = np.zeros((T, P, 3 * C), x.dtype)
    for t in range(T):
        for kt in range(3):
            if 0 <= t + kt - 1 < T:
                y[t, :, kt * C:(kt + 1) * C] = x[t + kt - 1]
    return y


def conv3d_same(x, w, bias=None):
    """x [Ci, T, H, W], w [Co, Ci, 3, 3, 3], zero padding 1 in t, y and x -> (y [Co, T, H, W], sum |w x| [Co, T, H, W]) in float64"""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    Ci, T, H, W = x.shape
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (1, 1)))
    y = np.zeros((w.shape[0], T, H, W))
    mag = np.zeros_like(y)
    for kt in range(3):
        for kh in range(3):
            for kw in range(3):
                win = xp[:, kt:kt + T, kh:kh + H, kw:kw + W]
                y += np.einsum("oc,cthw->othw", w[:, :, kt, kh, kw], win)
                mag += np.einsum("oc,cthw->othw", np.abs(w[:, :, kt, kh, kw]), np.abs(win))
    if bias is not None:
        b = np.asarray(bias, np.float64).reshape(-1, 1, 1, 1)
        y, mag = y + b, mag + np.abs(b)
    return y, mag


def elu(x):
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.where(x > 0, x, np.expm1(np.where(x > 0, 0.0, x)))


def gray_u8(rgb):
    """uint8 [..., 3] -> uint8 [...]"""
    c = np.asarray(rgb).astype(np.int64)
    return ((4899 * c[..., 0] + 9617 * c[..., 1] + 1868 * c[..., 2] + 8192) >> 14).astype(np.uint8)


def prep_frames(rgb):
    """uint8 [B, H, W, 3] -> float64 [B, H + 2, W + 2]: gray / 255 - 0.4462414 with a 1-pixel replicate border"""
    g = gray_u8(rgb).astype(np.float64) / 255.0 - 0.4462414
    return np.pad(g, ((0, 0), (1, 1), (1, 1)), mode="edge")


def prep_refs(rgb):
    """uint8 [B, H, W, 3] -> float64 [B, H, W, 3]: rgb / 255 - 0.48"""
    return np.asarray(rgb).astype(np.float64) / 255.0 - 0.48


def sigmoid(x):
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-x))


def lab_from_sigmoid(gray, sa, sb):
    """gray uint8 [...], sa / sb float32 [...] -> float32 Lab [..., 3] in float32 steps: L = gray / 255 * 100, a = clip(sa * 255 - 128, -100, 100), b likewise"""
    f = np.float32
    L = np.asarray(gray).astype(f) / f(255.0) * f(100.0)
    a = np.clip(np.asarray(sa, f) * f(255.0) - f(128.0), f(-100.0), f(100.0))
    b = np.clip(np.asarray(sb, f) * f(255.0) - f(128.0), f(-100.0), f(100.0))
    out = np.stack([L, a, b], -1)
    assert out.dtype == np.float32
    return out
