"""DeepRemaster's colour network (vsdeoldify/remaster/model/remasternet.py:103-187, NetworkC) as a libhavc_mi355 weight blob + execution plan.

The 5-D tensors of the reference ([B = 1][C][T][H][W]) are NHWC fp16 buffers whose batch entries are the T frames of the window, so
  * TempConv with kernel (1,3,3) = the 2-D conv of HAVC_OP_CONV at batch T, BatchNorm3d (eval) in the epilogue's affine, ELU as HAVC_OP_ELU;
  * kernel (3,3,3), pad (1,1,1) = HAVC_OP_TSTACK (frames t-1, t, t+1 side by side, zeros outside the window) + a 3 x 3 conv over 3 Ci channels with the
    weight repacked [Co][Ci][kt][3][3] -> [Co][kt * Ci][3][3] (repack_temporal);
  * F.interpolate(scale (1,2,2), trilinear, align_corners=False) = the bilinear mode of HAVC_OP_EW per frame (a temporal scale of 1 is the identity);
  * SourceReferenceAttention = HAVC_OP_SRCREF_ATTN; selfattn1 / selfattn2 are the same op with the window as its own reference.

One plan, two slices.  `encode` runs reffeatnet1 / reffeatnet2 and the key / value convs of stattn1 / stattn2 for ONE reference still: every layer of the two
stacks has a (1,3,3) kernel, so a still's features do not depend on the other stills, and its keys / values are written once into a slot of the
reference ring (RemasterSession).  `colorize` runs everything else at batch T and reads all slots; the softmax does not depend on the order of the keys,
so a new still may overwrite the oldest slot in place.
"""
from dataclasses import dataclass, field

import numpy as np

from . import _native as nat
from .plan import PlanBuilder, View, WeightPack, bn_scale_shift, pack_conv, pad_to, pitch_for, to_np

ENC = ((2, 0), (1, 1), (1, 1), (2, 1), (1, 1), (1, 1), (2, 1), (1, 1), (1, 1))       # (stride, pad) of down1.1-9; reffeatnet1 has pad 1 throughout


def repack_temporal(w):
    """Conv3d weight [Co][Ci][kt][kh][kw] -> [Co][kt * Ci][kh][kw]: input channel kt * Ci + c of the stacked tensor is channel c of frame t + kt - 1"""
    co, ci, kt, kh, kw = w.shape
    return np.ascontiguousarray(np.asarray(w).transpose(0, 2, 1, 3, 4).reshape(co, kt * ci, kh, kw))


@dataclass
class RemasterPlan:
    ops: np.ndarray
    bufs: np.ndarray
    names: list
    T: int
    H: int
    W: int
    ref_hw: tuple                 # (Hr, Wr) or None
    ref_frames: int
    in_buf: int = -1
    out_buf: int = -1
    ab_buf: int = -1
    ref_in: int = -1
    encode: tuple = (0, 0)        # (first op, count) of the per-still slice
    colorize: tuple = (0, 0)
    ring: dict = field(default_factory=dict)      # name -> (buffer id, bytes per slot): k1, v1, k2, v2
    taps: dict = field(default_factory=dict)      # name -> View of the tensors the fixtures record


class RemasterColorNet:
    def __init__(self, state_dict, precision="fast"):
        if precision != "fast":
            raise NotImplementedError("DeepRemaster exists in fast mode only (fp16 activations, fp32 accumulation); a hi / lo-pair plan is not built")
        sd = to_np(state_dict)
        self.sd = sd["modelC"] if "modelC" in sd and isinstance(sd["modelC"], dict) else sd      # remasternet.pth.tar holds {'modelC': ...}
        self.sd = to_np(self.sd)
        self.pack, self._pc = WeightPack(), {}
        self._frozen = False
        self.plan(2, 32, 32, (32, 32), 2)              # packs every weight once
        self.blob = self.pack.blob()
        self._frozen = True

    # ---- layers ----
    def _packed(self, key, make):
        if key not in self._pc:
            assert not self._frozen, key
            self._pc[key] = make()
        return self._pc[key]

    def _conv(self, b, p, x, bn=None, stride=1, pad=1, y=None, elu=True, flags=0, Co=None, aux0=0):
        """nn.Conv3d `p` on view x [-> BatchNorm3d `bn` -> ELU].  A (3,3,3) kernel first stacks the window's frames."""
        sd = self.sd
        w = sd[p + ".weight"].astype(np.float32)
        kt = w.shape[2]
        if kt == 3:
            pitch = pitch_for(3 * x.span)
            xs = View(b.buf(x.H * x.W * pitch), 0, pitch, x.H, x.W, 3 * x.span, 3 * x.span)
            b.tstack(p + ".tstack", x, xs)
            cmap = np.concatenate([k * x.span + x.cmap for k in range(3)])
            x = xs
        else:
            cmap = x.cmap

        def make():
            kw = {}
            if bn:
                kw["scale"], kw["shift"] = bn_scale_shift(sd, bn)
            return pack_conv(self.pack, repack_temporal(w), cmap, x.span, bias=sd[p + ".bias"], **kw)
        pc = self._packed(p, make)
        if y is None:
            Ho = (x.H + 2 * pad - 3) // stride + 1 if pc.kh == 3 else x.H
            Wo = (x.W + 2 * pad - 3) // stride + 1 if pc.kh == 3 else x.W
            y = b.tensor(Ho, Wo, pc.Cout)
        b.conv(p, pc, x, y, stride=stride, pad=pad if pc.kh == 3 else 0, flags=flags | (nat.F_AFFINE if bn else 0), Co=Co, aux0=aux0)
        if elu:
            b.elu(p + ".elu", y)
        return y

    def _tconv(self, b, p, x, **kw):
        return self._conv(b, p + ".conv3d", x, bn=p + ".bn", **kw)

    def _up(self, b, name, x, y=None):
        y = y or b.tensor(2 * x.H, 2 * x.W, x.C)
        b.ew(name, x, y, mode=1, ratio=(0.5, 0.5))
        return y

    def _kv(self, b, p, x):
        """key_conv / value_conv of attention `p` on the reference features x: (key buffer, transposed value buffer, value pitch)"""
        k = self._conv(b, p + ".key_conv", x, elu=False)
        npitch = pad_to(x.H * x.W, 64)
        vT = b.buf(x.C * npitch, 2, zero_init=True)
        self._conv(b, p + ".value_conv", x, elu=False, y=vT, flags=nat.F_OUT_TRANSPOSED, Co=x.C, aux0=npitch)
        return k.buf, vT, npitch

    def _attn(self, b, p, x, kv=None, ref_hw=None, ref_frames=0):
        q = self._conv(b, p + ".query_conv", x, elu=False)
        if kv is None:
            kv, ref_hw = self._kv(b, p, x), (x.H, x.W)
        y = b.tensor(x.H, x.W, x.C)
        b.srcref_attn(p, x, q, kv[0], kv[1], kv[2], ref_hw, y, float(self.sd[p + ".gamma"].reshape(-1)[0]), ref_frames)
        return y

    # ---- plan ----
    def plan(self, T, H, W, ref_hw=None, ref_frames=0):
        """T frames of H x W (multiples of 16) per call; ref_hw / ref_frames: size of the reference stills and slots of the ring (None / 0: the network
        without references, x_refs=None in the reference)."""
        assert T >= 2 and H % 16 == 0 and W % 16 == 0 and H >= 32 and W >= 32, (T, H, W)
        use_refs = bool(ref_hw) and ref_frames > 0
        b = PlanBuilder()
        P = RemasterPlan(None, None, b.names, T, H, W, tuple(ref_hw) if use_refs else None, ref_frames if use_refs else 0)
        P.in_buf, P.out_buf, P.ab_buf = b.buf(H * W * 3, 1), b.buf(H * W * 3, 1), b.buf(H * W * 2, 4)
        kv1 = kv2 = None
        if use_refs:
            Hr, Wr = ref_hw
            P.ref_in = b.buf(Hr * Wr * 3, 1)
            r = b.tensor(Hr, Wr, 3, zero_init=False)
            b.prep_remaster("prep_ref", P.ref_in, Hr, Wr, r, refs=True)
            for i, (stride, _) in enumerate(ENC):
                r = self._tconv(b, f"reffeatnet1.{i}", r, stride=stride)
            kv1, hw1 = self._kv(b, "stattn1", r), (r.H, r.W)
            r = self._tconv(b, "reffeatnet2.0", r, stride=2)
            r = self._tconv(b, "reffeatnet2.1", r)
            r = self._tconv(b, "reffeatnet2.2", r)
            kv2, hw2 = self._kv(b, "stattn2", r), (r.H, r.W)
            for name, kv, hw in (("1", kv1, hw1), ("2", kv2, hw2)):
                P.ring["k" + name] = (kv[0], hw[0] * hw[1] * 64 * 2)
                P.ring["v" + name] = (kv[1], 512 * kv[2] * 2)
            P.encode = (0, len(b.ops))
        first = len(b.ops)
        x = b.tensor(H + 2, W + 2, 1, zero_init=False)
        b.prep_remaster("prep_frames", P.in_buf, H, W, x)
        for i, (stride, pad) in enumerate(ENC):
            x = self._tconv(b, f"down1.{i + 1}", x, stride=stride, pad=pad)
        P.taps["down1"] = x
        if use_refs:
            x = self._attn(b, "stattn1", x, kv1, hw1, ref_frames)
            P.taps["stattn1"] = x
        # x2 = flat(x1) lands in the upper half of up1's concatenated input
        cat = b.tensor(x.H, x.W, 1024)
        x2 = View(cat.buf, 512, cat.cpitch, x.H, x.W, 512, 512)
        f = self._tconv(b, "flat.0", x)
        self._tconv(b, "flat.1", f, y=x2)
        P.taps["flat"] = x2
        o = self._tconv(b, "down2.0", x, stride=2)
        o = self._tconv(b, "down2.1", o)
        if use_refs:
            o = self._attn(b, "stattn2", o, kv2, hw2, ref_frames)
            P.taps["stattn2"] = o
        o = self._tconv(b, "conv1", o)
        o = self._attn(b, "selfattn1", o)
        P.taps["selfattn1"] = o
        self._up(b, "up1.up", o, View(cat.buf, 0, cat.cpitch, cat.H, cat.W, 512, 512))
        o = self._tconv(b, "up1.conv3d", cat)
        P.taps["up1"] = o
        o = self._attn(b, "selfattn2", o)
        P.taps["selfattn2"] = o
        o = self._tconv(b, "conv2", o)
        P.taps["conv2"] = o
        for p in ("up2", "up3"):
            o = self._tconv(b, p + ".0", self._up(b, p + ".up", o))
            o = self._tconv(b, p + ".1", o)
        o = self._tconv(b, "up4.0", self._up(b, "up4.up", o))
        o = self._conv(b, "up4.1", o, elu=False)
        b.remaster_out("sigmoid_lab2rgb", o, P.in_buf, P.out_buf, P.ab_buf)
        P.colorize = (first, len(b.ops) - first)
        P.ops, P.bufs = b.finish()
        return P


class RemasterSession:
    """A plan on one GPU context: the net, its weights and the reference ring (one slot of keys / values per reference still, in device memory
    of its own; the plan's key / value buffers are pointed at a slot for `encode_reference` and at the whole ring for `colorize`)."""

    def __init__(self, ctx, model, T, H, W, ref_hw=None, ref_frames=0, weights=None):
        self.ctx, self.model = ctx, model
        self.weights = weights or nat.Weights(ctx, model.blob)
        self.plan = P = model.plan(T, H, W, ref_hw, ref_frames)
        self.net = nat.Net(ctx, self.weights, P.ops, P.bufs, P.in_buf, P.out_buf, H, T)
        self._ring = {}
        for name, (buf, slot_bytes) in P.ring.items():
            n = slot_bytes * P.ref_frames
            d = ctx.dev_alloc(n + 256)
            ctx.dev_upload(d, np.zeros(n + 256, np.uint8))          # the value rows must be zero beyond a still's keys
            self._ring[name] = (buf, d, slot_bytes)
        self._bound_slot = None

    def close(self):
        if getattr(self, "net", None):
            self.net.close()
            self.net = None
            for _, d, _ in self._ring.values():
                self.ctx.dev_free(d)
            self._ring = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _bind(self, slot):
        if self._bound_slot != slot:
            for buf, d, slot_bytes in self._ring.values():
                self.net.bind(buf, (d.value or 0) + (0 if slot is None else slot * slot_bytes))
            self._bound_slot = slot

    def encode_reference(self, slot, ref, sync=True):
        """reffeatnet1 / reffeatnet2 + the key / value convs of stattn1 / stattn2 for one still (u8 RGB [Hr][Wr][3] array, or a device pointer) -> ring slot"""
        P = self.plan
        assert P.ref_frames and 0 <= slot < P.ref_frames
        if isinstance(ref, np.ndarray):
            assert ref.shape == (P.ref_hw[0], P.ref_hw[1], 3) and ref.dtype == np.uint8, ref.shape
            self.net.bind(P.ref_in, None)
            self.net.upload(P.ref_in, ref)
        else:
            self.net.bind(P.ref_in, ref)
        self._bind(slot)
        (self.net.run_ops if sync else self.net.enqueue_ops)(P.encode[0], P.encode[1], 1)

    def colorize(self, frames, d_out=None, sync=True, n=None):
        """frames: u8 RGB [n][H][W][3] array (n <= T; a single frame is doubled, as the reference does, and one frame comes back) or a device pointer
        to n frames (2 <= n <= T, default T).  Returns the u8 RGB frames (array input) or None (device pointers: the result is in d_out)."""
        P = self.plan
        self._bind(None)
        if isinstance(frames, np.ndarray):
            n = frames.shape[0]
            assert frames.shape[1:] == (P.H, P.W, 3) and frames.dtype == np.uint8 and 1 <= n <= P.T, frames.shape
            fr = np.concatenate([frames, frames]) if n == 1 else frames
            self.net.bind(P.in_buf, None)
            self.net.bind(P.out_buf, None)
            self.net.upload(P.in_buf, fr)
            self.net.run_ops(P.colorize[0], P.colorize[1], fr.shape[0])
            return self.net.download(P.out_buf, (fr.shape[0], P.H, P.W, 3), np.uint8)[:n]
        self.net.bind(P.in_buf, frames)
        self.net.bind(P.out_buf, d_out)
        n = P.T if n is None else int(n)
        assert 2 <= n <= P.T, n
        (self.net.run_ops if sync else self.net.enqueue_ops)(P.colorize[0], P.colorize[1], n)
        return None

    def tap(self, name, n_frames):
        """the recorded tensor `name` of the last colorize call as float32 [C][T][H][W] (the reference's layout); 'ab' = the sigmoid output"""
        P = self.plan
        if name == "ab":
            a = self.net.download(P.ab_buf, (n_frames, P.H, P.W, 2), np.float32)
            return a.transpose(3, 0, 1, 2)
        v = P.taps[name]
        per = int(P.bufs[v.buf]["elems_per_frame"])
        a = self.net.download(v.buf, (n_frames, per), np.float16)[:, :v.H * v.W * v.cpitch].reshape(n_frames, v.H, v.W, v.cpitch)
        return a[..., v.coff:v.coff + v.C].astype(np.float32).transpose(3, 0, 1, 2)
